"""Mirror of the reference's data_processing/process_sample.py: a raw view (distance.exr, distance_field.df,
intrinsic.txt) -> what the trainers load (depth_grid.npz, mesh.obj, target.df, occupancy_0.01.npz, occupancy_0.10.npz).

Same files, keys and dtypes as process_sample.py:10-30.  The work runs on the device: the distance map goes through one
kernel to the marked grid (distance_to_depth.depth_grid), the distance field through marching cubes
(util.visualize.marching_cubes, level 1.0), and the mesh goes to mesh_occupancies.sample_points in memory -- mesh.obj is
written but not read back.  Only the finished arrays cross to the host.

Out-of-range pixels.  The reference indexes a numpy grid with the rounded coordinates: an index >= dim raises IndexError
(which process_sample_pipeline catches to quarantine the view), an index in [-dim, 0) silently wraps to the other side of
the grid.  Here every pixel whose voxel lies outside [0, dim) on any axis -- the wrapped range and NaN / inf distances
included -- counts as out of range, and a non-zero count raises IndexError.

An empty mesh (marching cubes finds no face) raises EmptyMeshError, an AttributeError like the one the reference's
trimesh path ends in; the pipeline quarantines that view too."""
import os
from pathlib import Path
from shutil import copyfile, move

import numpy as np
import torch

from ..util.visualize import export_obj, marching_cubes
from .distance_to_depth import depth_grid
from .mesh_occupancies import sample_points
from .volume_reader import read_df
from . import sample_io

SIGMAS = (0.01, 0.1)


class EmptyMeshError(AttributeError):
    pass


def sample_dims(down_scale_factor=1):
    return (round(139 / down_scale_factor), round(104 / down_scale_factor), round(112 / down_scale_factor))


def _ensure_distance_field(sample, scene_mesh, down_scale_factor):
    """`scene_mesh` given and no distance_field.df in the view: compute it from <sample>/<scene_mesh> (grid units of the
    down_scale_factor's lattice) and write it next to the raw files.  An existing file is not touched."""
    target = sample / "distance_field.df"
    if scene_mesh is None or target.exists():
        return
    from .mesh_to_df import mesh_to_df          # imports this module for EmptyMeshError / sample_dims
    mesh_to_df(sample / scene_mesh, target, dims=sample_dims(down_scale_factor))


def _ensure_view(sample, scene_mesh, intrinsic_path, down_scale_factor):
    """`scene_mesh` given and no distance.exr in the view: ray-cast <sample>/<scene_mesh> through the view's camera
    (data_processing.render_view) and write distance.exr -- and rgb.png when that is absent too -- next to the raw files.
    Existing files are not touched."""
    if scene_mesh is None or (sample / "distance.exr").exists():
        return
    from .render_view import render_view        # imports this module (through mesh_to_df) for EmptyMeshError
    render_view(sample / scene_mesh, sample, intrinsic=intrinsic_path, scale_factor=down_scale_factor,
                write_rgb=not (sample / "rgb.png").exists())


def _process_view(sample, out, intrinsic_path, down_scale_factor, sample_num, generator, copy_target, scene_mesh=None,
                  render_missing=False):
    dims = sample_dims(down_scale_factor)
    if render_missing:
        _ensure_view(sample, scene_mesh, intrinsic_path, down_scale_factor)
    _ensure_distance_field(sample, scene_mesh, down_scale_factor)
    distance = sample_io.exr_read(sample / "distance.exr", "R")
    grid, out_of_range = depth_grid(distance, dims, intrinsic_path, down_scale_factor)
    n_out = int(out_of_range.item())
    if n_out:
        raise IndexError(f"{sample / 'distance.exr'}: {n_out} pixels unproject outside the {dims[0]} x {dims[1]} x {dims[2]} grid")
    np.savez_compressed(out / "depth_grid", grid=grid.cpu().numpy().astype(np.float64))

    df = read_df(str(sample / "distance_field.df"), down_scale_factor)
    vertices, faces = marching_cubes(torch.from_numpy(np.ascontiguousarray(df, dtype=np.float32)).cuda(), 1.0)
    if faces.shape[0] == 0:
        raise EmptyMeshError(f"{sample / 'distance_field.df'}: no surface at level 1.0")
    mesh = (vertices.cpu().numpy(), faces.cpu().numpy())
    export_obj(mesh[0], mesh[1], sample / "mesh.obj")
    if copy_target:
        copyfile(str(sample / "distance_field.df"), out / "target.df")

    for sigma in SIGMAS:
        boundary_points, occupancies, grid_coords = sample_points(mesh, dims, sample_num, sigma, generator=generator)
        np.savez(out / f"occupancy_{sigma:.02f}", points=boundary_points.cpu().numpy(), occupancies=occupancies.cpu().numpy(),
                 grid_coords=grid_coords.cpu().numpy())


def process_sample(dataset_path, splitsdir, sample_name, down_scale_factor=1, sample_num=100000, generator=None, scene_mesh=None,
                   render_missing=False):
    """raw/<splitsdir>/<sample_name> -> processed/<splitsdir>/<sample_name> (+ mesh.obj next to the raw files).
    `generator`: a torch.Generator for sample_points' draws.

    `scene_mesh` (default None: nothing changes): the name of a triangle mesh in the view's directory, e.g. "scene.obj", in
    grid units of the down_scale_factor's lattice.  A view without distance_field.df gets one computed from it
    (data_processing.mesh_to_df) and written next to the raw files before the unchanged rest runs; a view that already has
    the file is not touched.  A mesh without a face that has an area raises EmptyMeshError.  mesh.obj stays what it is
    today -- the level-1.0 surface of the field -- and is NOT the input mesh, so `scene_mesh` must not be "mesh.obj".
    The written file has the extents sample_dims(down_scale_factor); the unchanged rest reads it like any
    distance_field.df, i.e. read_df block-averages it by down_scale_factor once more -- so with a factor other than 1 write
    the full-resolution field yourself (mesh_to_df with the mesh in full-resolution grid units) instead of using
    `scene_mesh`.

    `render_missing` (default False: nothing changes): with `scene_mesh`, a view without distance.exr gets one ray-cast from
    the mesh through the view's intrinsic.txt first (data_processing.render_view), and a grey stand-in rgb.png when that
    is absent too; existing files are not touched."""
    if scene_mesh == "mesh.obj":
        raise ValueError("process_sample: scene_mesh must not be mesh.obj, the file this function writes")
    sample = Path(dataset_path) / "raw" / splitsdir / sample_name
    out = Path(dataset_path) / "processed" / splitsdir / sample_name
    out.mkdir(exist_ok=True, parents=True)
    _process_view(sample, out, sample / "intrinsic.txt", down_scale_factor, sample_num, generator, True, scene_mesh, render_missing)


def process_sample_pipeline(dataset_path, splitsdir, down_scale_factor=1, sample_num=100000, generator=None, scene_mesh=None,
                            render_missing=False):
    """Every <dataset_path>/<splitsdir>/<scene>/<view>, processed in place with <dataset_path>/intrinsics.txt
    (process_sample.py:32-72; like there, no target.df copy).  A view with out-of-range depth (IndexError) or an empty
    mesh (AttributeError; an empty `scene_mesh` included) is moved to <dataset_path>/quarantine/<splitsdir>/<scene>/<view>.
    `scene_mesh`, `render_missing`: as for process_sample (the camera is <dataset_path>/intrinsics.txt).  -> the quarantined
    paths."""
    if scene_mesh == "mesh.obj":
        raise ValueError("process_sample_pipeline: scene_mesh must not be mesh.obj, the file this function writes")
    d_path = Path(dataset_path) / splitsdir
    quarantined = []
    for scene in sorted(os.listdir(d_path)):
        for view in sorted(os.listdir(d_path / scene)):
            sample = d_path / scene / view
            try:
                _process_view(sample, sample, Path(dataset_path) / "intrinsics.txt", down_scale_factor, sample_num, generator, False,
                              scene_mesh, render_missing)
            except (IndexError, AttributeError) as e:
                quarantine = Path(dataset_path) / "quarantine" / splitsdir / scene / view
                print(f"{type(e).__name__}: {e}; moving {sample} to {quarantine}")
                quarantine.parent.mkdir(exist_ok=True, parents=True)
                move(str(sample), str(quarantine))
                quarantined.append(quarantine)
    return quarantined
