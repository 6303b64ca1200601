"""Mirror of the reference's data_processing/convert_to_scaled_obj.py: the step between the meshes ``--test`` writes (grid
space, ``*_predicted.obj``) and util/evaluate.py, which compares meshes in the unit cube.

``normalize_meshes(folder, scale_factor=1, pattern="*_predicted.obj")`` writes ``<name>_normed.obj`` next to every match:
vertices ``(v - dims / 2) / dims`` with ``dims = (139, 104, 112) / scale_factor`` -- NOT rounded, unlike the trainers'
lattice: the reference divides and leaves it there -- computed in float64 and rounded once to the float32 the .obj writer
stores.  Faces are kept.  Returns the written paths.  Read through mesh_occupancies.load_obj, written through svr_write_obj
(no trimesh).

``python -m svr_amd.data_processing.convert_to_scaled_obj --experiment NAME [--scale_factor S] [--verbose]`` works on
results/NAME, as the reference's script."""
import argparse
import glob
import os
from pathlib import Path

import numpy as np

from ..util.visualize import export_obj
from .mesh_occupancies import load_obj


def normalize_meshes(folder, scale_factor=1, pattern="*_predicted.obj", verbose=False):
    dims = np.array([139, 104, 112], dtype=np.float64) / np.round(scale_factor).astype(np.int64)
    meshes = sorted(glob.glob(str(Path(folder) / pattern)))
    written = []
    for i, path in enumerate(meshes):
        if verbose:
            print(f"reading mesh: {i}/{len(meshes)}")
        mesh = load_obj(path)
        vertices = (mesh.vertices - dims / 2) / dims
        out = path[:-4] + "_normed.obj"
        export_obj(vertices.astype(np.float32), mesh.faces, out)
        written.append(out)
    return written


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Convert meshes to scaled and centered meshes")
    parser.add_argument("--experiment", type=str, default="asd")
    parser.add_argument("--verbose", dest="verbose", action="store_true", help="Verbose")
    parser.add_argument("--scale_factor", type=int, default=1, help="Down scale the voxel grid input.")
    _args = parser.parse_args()
    normalize_meshes(os.path.join("results", _args.experiment), _args.scale_factor, verbose=_args.verbose)
