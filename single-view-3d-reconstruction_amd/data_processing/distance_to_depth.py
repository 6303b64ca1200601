"""Mirror of the reference's data_processing/distance_to_depth.py on the device (raw_sample.hip, projection.hip).

``FromDistanceToDepth(focal_length)(distance_image)``: a ray-length map -> a z-depth map, (H, W) or (B, H, W); the rule
and its rounding are in include/svr_hip.h (svr_distance_to_depth).  Like the reference it centres on the integers
rows - H//2 and cols - W//2, not on the intrinsic's cx / cy.  A numpy array is uploaded; the result is a device tensor.

``depthmap_to_gridspace(depthmap, intrinsic_path=None, down_scale_factor=1)``: depth -> un-normalised grid-space
coordinates through svr_unproject_fwd with the constants of model.projection._camera_to_grid.  (H, W) gives (H*W, 3); a
leading batch axis gives (B, H*W, 3).

The flattened shape is the contract.  The reference's function sets ``bs = depthmap.shape[0]`` and reshapes to
(bs, -1, 3), so for the 2-D map that process_sample hands it the result is (240, 320, 3) and ``[:, 0]`` selects 240
points: 66 marked voxels.  The depth_grid.npz the reference ships (5 466 ones) is what the flattened (H*W, 3) form gives,
and that is what this module returns.

``depth_to_gridspace(distance_map_path, intrinsic_path=None, down_scale_factor=1)``: channel R of the .exr (native
reader) -> depth with the intrinsic's focal length -> grid space.  ``depth_grid`` is the fused form process_sample uses:
one kernel from the map to the marked uint8 grid and the count of pixels that fall outside it."""
import ctypes as C

import torch

from .. import _lib, ops
from .._lib import check, ptr, stream, to_device
from ..model.projection import _camera_to_grid, project
from . import sample_io


def get_intrinsic(intrinsic_path=None):
    """4x4 float32 intrinsic: the parser of model.projection.project.get_intrinsic; None = the constants of
    data/raw/overfit/00000/intrinsic.txt (the reference reads that file relative to the working directory)."""
    return project.get_intrinsic(intrinsic_path)


def _device_map(a, what):
    a, _ = to_device(a, what, torch.float32)
    if a.dim() not in (2, 3):
        raise ValueError(f"{what}: expected (H, W) or (B, H, W), got {tuple(a.shape)}")
    return a


def _grid_consts(intrinsic, down_scale_factor, dims=(0, 0, 0)):
    """The 12 constants of svr_unproject_fwd for (intrinsic, scale): project._consts without a module instance."""
    K = intrinsic.cpu()
    _, inv, t = _camera_to_grid(K, down_scale_factor)
    return [float(K[0, 0]), float(K[0, 2]), float(K[1, 2]), float(inv), float(t[0]), float(inv), float(t[1]), float(inv),
            float(t[2]), float(dims[0]), float(dims[1]), float(dims[2])]


class FromDistanceToDepth:
    def __init__(self, focal_length):
        self.focal_length = float(focal_length)

    def __call__(self, distance_image):
        d = _device_map(distance_image, "FromDistanceToDepth")
        out = torch.empty_like(d)
        B = 1 if d.dim() == 2 else d.shape[0]
        check(_lib.lib().svr_distance_to_depth(ptr(d), ptr(out), B, d.shape[-2], d.shape[-1], self.focal_length, stream()),
              "distance_to_depth")
        return out


def depthmap_to_gridspace(depthmap, intrinsic_path=None, down_scale_factor=1):
    d = _device_map(depthmap, "depthmap_to_gridspace")
    consts = _grid_consts(get_intrinsic(intrinsic_path), down_scale_factor)
    pc = ops.unproject(d if d.dim() == 3 else d.unsqueeze(0), consts, False)
    return pc if d.dim() == 3 else pc[0]


def depth_to_gridspace(distance_map_path, intrinsic_path=None, down_scale_factor=1):
    distance = sample_io.exr_read(distance_map_path, "R")
    focal_length = get_intrinsic(intrinsic_path)[0][0]
    depthmap = FromDistanceToDepth(focal_length)(distance)
    return depthmap_to_gridspace(depthmap, intrinsic_path, down_scale_factor)


def depth_grid(image, dims, intrinsic_path=None, down_scale_factor=1, is_distance=True, return_coords=False):
    """One (H, W) distance map (or depth map, is_distance=False) -> (grid uint8 `dims`, out_of_range int32 (1,)[, coords
    (H*W, 3)]) on the device, in one kernel: the voxel np.round(coordinate) of every pixel is set to 1; pixels whose voxel
    lies outside the grid (NaN / inf, and the negative indices numpy would wrap) are skipped and counted."""
    m = _device_map(image, "depth_grid")
    if m.dim() != 2:
        raise ValueError(f"depth_grid: one (H, W) map per call, got {tuple(m.shape)}")
    K = get_intrinsic(intrinsic_path)
    D0, D1, D2 = (int(v) for v in dims)
    consts = (C.c_float * 12)(*_grid_consts(K, down_scale_factor, (D0, D1, D2)))
    grid = torch.zeros(D0, D1, D2, device=m.device, dtype=torch.uint8)
    count = torch.zeros(1, device=m.device, dtype=torch.int32)
    coords = torch.empty(m.numel(), 3, device=m.device, dtype=torch.float32) if return_coords else None
    check(_lib.lib().svr_depth_grid_mark(ptr(m), int(is_distance), float(K[0, 0]), m.shape[0], m.shape[1], consts, ptr(grid),
                                         D0, D1, D2, ptr(count), ptr(coords), stream()), "depth_grid_mark")
    return (grid, count, coords) if return_coords else (grid, count)
