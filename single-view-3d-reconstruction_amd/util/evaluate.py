"""Mirror of the reference's util/evaluate.py:9-119 (eval_mesh, eval_pointcloud, distance_p2p) on the library's mesh
evaluation kernels (include/svr_hip.h, "Mesh evaluation"): same names, argument order and
dictionary keys.  The reference needs trimesh (mesh.sample, face_normals) and pykdtree (KDTree.query) and runs on the
CPU; here the face table is built by the library's C++ host code, and sampling, the exact nearest-neighbour search, the
normal dot products, the occupancy labels and every sum run on the device.  Only the final scalars cross to the host.

Point clouds and normals: CUDA tensors in -> CUDA tensors out; numpy in -> numpy out (the convention of
check_mesh_contains / marching_cubes); CPU tensors are refused like everywhere on the HIP path.  Points are float32
(the reference casts its samples with .astype(np.float32) before the tree); anything else is cast.

A mesh is anything data_processing.mesh_occupancies accepts (object with .vertices / .faces, a (V, F) pair, an .obj
path) or the device (vertices, faces) pair implicit_to_mesh returns.  Face normals always come from the face table.

Random numbers: `generator` (a torch.Generator; a CPU generator seeds a device generator) drives every draw, on the
device, in float64, in this order (eval_mesh_draws): (n_points, 3) uniforms for the predicted mesh's surface samples,
(n_points, 3) for the ground-truth mesh's, (10 * n_points, 3) for the box samples of the IoU.  The reference draws from
numpy's global RNG, so its samples differ one by one; the estimator is the same."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr as _p, stream as _stream, to_device as _to_device

KEYS = ("completeness", "accuracy", "normals completeness", "normals accuracy", "normals", "completeness2", "accuracy2",
        "chamfer_l2", "iou")


def _points(a, what):
    t, as_numpy = _to_device(a, what, torch.float32)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: expected (N, 3) points, got {tuple(t.shape)}")
    return t, as_numpy


def nn_search(queries, targets):
    """Exact nearest target of every query (svr_nn_search: float32, ties to the lowest index): device tensors
    (Q,3), (T,3) float32 -> (dist (Q,) float32, idx (Q,) int32)."""
    l = _lib.lib()
    Q, T = int(queries.shape[0]), int(targets.shape[0])
    dist = torch.empty(Q, device=queries.device, dtype=torch.float32)
    idx = torch.empty(Q, device=queries.device, dtype=torch.int32)
    ws_bytes = int(l.svr_nn_search_workspace(Q))
    ws = torch.empty(max(ws_bytes, 8), device=queries.device, dtype=torch.uint8)
    check(l.svr_nn_search(_p(queries), Q, _p(targets), T, _p(dist), _p(idx), _p(ws), ws_bytes, _stream()), "nn_search")
    return dist, idx


def _normals_dot(normals_q, normals_t, idx):
    if normals_q.dtype != normals_t.dtype or normals_q.dtype not in (torch.float32, torch.float64):
        normals_q, normals_t = normals_q.double(), normals_t.double()
    normals_q, normals_t = normals_q.contiguous(), normals_t.contiguous()
    Q, T = int(normals_q.shape[0]), int(normals_t.shape[0])
    out = torch.empty(Q, device=idx.device, dtype=torch.float64)
    check(_lib.lib().svr_nn_normals_dot(_p(normals_q), _p(normals_t), int(normals_q.dtype == torch.float64), _p(idx), Q, T,
                                        _p(out), _stream()), "nn_normals_dot")
    return out


def _distance_p2p_device(pred, gt, normals_pred, normals_gt):
    dist, idx = nn_search(pred, gt)
    if normals_pred is None:
        return dist, None, idx
    if normals_pred.shape[0] != pred.shape[0] or normals_gt.shape[0] != gt.shape[0]:
        raise ValueError("distance_p2p: one normal per point is needed")
    return dist, _normals_dot(normals_pred, normals_gt, idx), idx


def distance_p2p(pointcloud_pred, pointcloud_gt, normals_pred, normals_gt, return_index=False):
    """For every point of `pointcloud_pred` the distance to its nearest point of `pointcloud_gt` and, with normals,
    |n_pred . n_gt[nearest]| of the normalised normals -> (dist, normals_dot | None) (+ the indices, int32, when
    `return_index`).  dist is float32, normals_dot float64."""
    pred, np_out = _points(pointcloud_pred, "distance_p2p")
    gt, _ = _points(pointcloud_gt, "distance_p2p")
    if normals_pred is not None:
        normals_pred, _ = _to_device(normals_pred, "distance_p2p")
        normals_gt, _ = _to_device(normals_gt, "distance_p2p")
    dist, dot, idx = _distance_p2p_device(pred, gt, normals_pred, normals_gt)
    out = (dist, dot, idx) if return_index else (dist, dot)
    if np_out:
        out = tuple(None if o is None else o.cpu().numpy() for o in out)
    return out


def _sums(dist, dot, out):
    """out (3,) float64 on the device = sum d, sum d^2, sum dot (NaN without dot), in the library's fixed order."""
    ws = torch.empty(_lib.EVAL_SUMS_WORKSPACE_BYTES, device=dist.device, dtype=torch.uint8)
    check(_lib.lib().svr_eval_sums(_p(dist), _p(dot), int(dist.shape[0]), _p(out), _p(ws),
                                   int(ws.numel()), _stream()), "eval_sums")


def _eval_pointcloud_device(pred, gt, normals_pred, normals_gt):
    sums = torch.empty((2, 3), device=pred.device, dtype=torch.float64)
    # completeness: ground truth -> prediction; accuracy: prediction -> ground truth
    c_dist, c_dot, _ = _distance_p2p_device(gt, pred, normals_gt, normals_pred)
    _sums(c_dist, c_dot, sums[0])
    a_dist, a_dot, _ = _distance_p2p_device(pred, gt, normals_pred, normals_gt)
    _sums(a_dist, a_dot, sums[1])
    (cs, cs2, cn), (as_, as2, an) = sums.tolist()                 # the only device -> host copy
    nc, na = gt.shape[0], pred.shape[0]
    div = lambda s, n: s / n if n else float("nan")               # noqa: E731  (numpy's mean of an empty array)
    completeness, completeness2, accuracy, accuracy2 = div(cs, nc), div(cs2, nc), div(as_, na), div(as2, na)
    nan = float("nan")
    cn, an = (div(cn, nc), div(an, na)) if normals_pred is not None else (nan, nan)
    return {
        "completeness": completeness,
        "accuracy": accuracy,
        "normals completeness": cn,
        "normals accuracy": an,
        "normals": 0.5 * cn + 0.5 * an,
        "completeness2": completeness2,
        "accuracy2": accuracy2,
        "chamfer_l2": 0.5 * completeness2 + 0.5 * accuracy2,
        "iou": nan,
    }


def eval_pointcloud(pointcloud_pred, pointcloud_gt, normals_pred=None, normals_gt=None):
    """-> dict of Python floats with the reference's keys (`KEYS`); the normal entries are NaN without normals, `iou` is
    always NaN here (eval_mesh fills it)."""
    pred, _ = _points(pointcloud_pred, "eval_pointcloud")
    gt, _ = _points(pointcloud_gt, "eval_pointcloud")
    if normals_pred is not None:
        normals_pred, _ = _to_device(normals_pred, "eval_pointcloud")
        normals_gt, _ = _to_device(normals_gt, "eval_pointcloud")
    return _eval_pointcloud_device(pred, gt, normals_pred, normals_gt)


class EvalMesh:
    """A mesh prepared for sampling: host vertices (float64) / faces (int32) for the triangle hash, and on the device the
    face table of svr_mesh_face_table (unit `face_normals`, running `cum_area`) and the corner table `tri` (F,3,3)."""

    def __init__(self, mesh, device=None):
        from ..data_processing.mesh_occupancies import _as_mesh
        if isinstance(mesh, (tuple, list)) and len(mesh) == 2 and any(torch.is_tensor(m) for m in mesh):
            if device is None and torch.is_tensor(mesh[0]) and mesh[0].is_cuda:
                device = mesh[0].device
            mesh = SimpleNamespace(vertices=_host(mesh[0]), faces=_host(mesh[1]))
        mesh = _as_mesh(mesh)
        self.vertices = np.ascontiguousarray(_host(mesh.vertices), dtype=np.float64)
        self.faces = np.ascontiguousarray(_host(mesh.faces), dtype=np.int32)
        v, f = self.vertices, self.faces
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or len(f) == 0:
            raise ValueError(f"mesh: vertices {v.shape}, faces {f.shape}")
        normals = np.empty((len(f), 3), dtype=np.float64)
        cum = np.empty(len(f), dtype=np.float64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)               # noqa: E731
        check(_lib.lib().svr_mesh_face_table(vp(v), len(v), vp(f), len(f), vp(normals), vp(cum)), "mesh_face_table")
        dev = torch.device(device if device is not None else "cuda")
        self.face_normals = torch.from_numpy(normals).to(dev)
        self.cum_area = torch.from_numpy(cum).to(dev)
        self.tri = torch.from_numpy(v[f]).to(dev)
        self.area = float(cum[-1])
        self.device = dev


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _prepared(mesh):
    return mesh if isinstance(mesh, EvalMesh) else EvalMesh(mesh)


def _device_generator(generator, device):
    if generator is None or generator.device.type == "cuda":
        return generator
    g = torch.Generator(device=device)
    g.manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=generator)))
    return g


def sample_with_uniforms(mesh, uniforms):
    """The sampler as a pure function: `uniforms` (n,3) float64 on the device -> (points (n,3) float32, face_index (n,)
    int32, normals (n,3) float64 = face_normals[face_index]).  Rule: include/svr_hip.h, svr_mesh_sample."""
    if not (torch.is_tensor(uniforms) and uniforms.is_cuda):
        raise RuntimeError("sample_with_uniforms HIP path needs GPU tensors (no CPU fallback)")
    m = _prepared(mesh)
    u = uniforms.to(torch.float64).contiguous()
    n = int(u.shape[0])
    pts = torch.empty((n, 3), device=u.device, dtype=torch.float32)
    face = torch.empty(n, device=u.device, dtype=torch.int32)
    if not m.area > 0.0:
        raise ValueError("sample_surface: the mesh has no area")
    check(_lib.lib().svr_mesh_sample(_p(m.tri), _p(m.cum_area), int(m.cum_area.shape[0]), _p(u), n, _p(pts), _p(face), _stream()),
          "mesh_sample")
    return pts, face, m.face_normals[face.long()]


def sample_surface(mesh, n, generator=None):
    """mesh.sample(n, return_index=True) + face_normals[idx] of the reference (area-weighted faces, uniform inside a
    face): -> (points (n,3) float32, face_index (n,) int32, normals (n,3) float64), on the device."""
    m = _prepared(mesh)
    g = _device_generator(generator, m.device)
    return sample_with_uniforms(m, torch.rand((int(n), 3), device=m.device, dtype=torch.float64, generator=g))


def eval_mesh_draws(n_points, generator, device="cuda"):
    """The random numbers of one eval_mesh call, in its order: (u_pred (n,3), u_gt (n,3), u_box (10 n,3)) float64."""
    device = torch.device(device)
    g = _device_generator(generator, device)
    draw = lambda k: torch.rand((k, 3), device=device, dtype=torch.float64, generator=g)      # noqa: E731
    return draw(int(n_points)), draw(int(n_points)), draw(int(n_points) * 10)


def _bound(b, device):
    return b if isinstance(b, (int, float)) else torch.as_tensor(np.asarray(_host(b), dtype=np.float64), device=device)


def eval_mesh(mesh_pred, mesh_gt, bb_min, bb_max, n_points=100000, generator=None):
    """The reference's eval_mesh: eval_pointcloud on n_points surface samples of each mesh with their face normals, and
    `iou` from 10 * n_points uniform samples of the box [bb_min, bb_max], labelled by implicit_waterproofing."""
    from ..data_processing.implicit_waterproofing import implicit_waterproofing
    mp, mg = _prepared(mesh_pred), _prepared(mesh_gt)
    u_pred, u_gt, u_box = eval_mesh_draws(n_points, generator, mp.device)
    pc_pred, _, normals_pred = sample_with_uniforms(mp, u_pred)
    pc_gt, _, normals_gt = sample_with_uniforms(mg, u_gt)
    out = _eval_pointcloud_device(pc_pred, pc_gt, normals_pred, normals_gt)
    bb_min, bb_max = _bound(bb_min, mp.device), _bound(bb_max, mp.device)
    bb_samples = u_box * (bb_max - bb_min) + bb_min
    occ_pred = implicit_waterproofing(mp, bb_samples)[0].to(torch.uint8)
    occ_gt = implicit_waterproofing(mg, bb_samples)[0].to(torch.uint8)
    counts = torch.empty(2, device=mp.device, dtype=torch.int64)
    check(_lib.lib().svr_iou_counts(_p(occ_pred), _p(occ_gt), int(occ_pred.shape[0]), _p(counts), _stream()), "iou_counts")
    inter, union = counts.tolist()
    out["iou"] = inter / union if union else float("nan")
    return out


def main(argv=None):
    """The reference's __main__ loop (:121-180): evaluates the predicted meshes listed in <path_files>/<experiment>
    against <path_files>/normed_gt.txt and writes results/exp_<experiment> in the reference's format."""
    import argparse
    from pathlib import Path

    from ..data_processing.mesh_occupancies import load_obj
    parser = argparse.ArgumentParser(description="Evaluate predicted meshes against ground truth")
    parser.add_argument("--path_files", type=str, default="results/path_files")
    parser.add_argument("--experiment", type=str, default="425_results.txt")
    parser.add_argument("--verbose", dest="verbose", action="store_true", help="verbose")
    args = parser.parse_args(argv)
    results_pth = Path("results")
    path_files = Path(args.path_files)
    with open(str(path_files / args.experiment), "r") as fh:
        paths_predicted = fh.read().splitlines()
    with open(str(path_files / "normed_gt.txt"), "r") as fh:
        paths_gt = fh.read().splitlines()
    performance = {k: [] for k in KEYS}
    for i in range(len(paths_predicted)):
        if args.verbose:
            print("reading mesh: " + str(i) + "/" + str(len(paths_predicted)) + " with names:" + paths_predicted[i] + " " + paths_gt[i])
        out = eval_mesh(load_obj(str(paths_predicted[i])), load_obj(str(paths_gt[i])), -0.5, 0.5, n_points=100000)
        for key in performance:
            performance[key].append(out[key])
    os.makedirs(str(results_pth), exist_ok=True)
    with open(str(results_pth / ("exp_" + args.experiment)), "w") as fh:
        n = len(performance["completeness"])
        fh.write(str(n) + " meshes" + "\n")
        for key in performance:
            mean = np.sum(performance[key]) / n if n else float("nan")
            fh.write("mean " + key + ": " + str(mean) + "\n")
        fh.write("\n")
        for key in performance:
            fh.write(key + ": " + str(performance[key]))
            fh.write("\n")


if __name__ == "__main__":
    main()
