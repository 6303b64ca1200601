"""GPU: the mesh evaluation kernels (csrc/mesh_eval.hip through the C ABI and svr_amd.util.evaluate) against the numpy
oracle (tests/eval_oracle.py: the rules of include/svr_hip.h) -- nearest neighbours and samples bit for bit -- and
against the reference's eval_pointcloud (tests/golden/eval_pointcloud.npz).  numpy + torch only."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import mesh_oracle as M
from tests import eval_oracle as E
from tests import mc_oracle as MC
from tests.test_eval_oracle_cpu import REL, assert_dict_close, golden, ref_dict

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [(1, 1), (63, 1), (1, 5000), (1000, 777), (8192, 8192), (20000, 30011)]
KINDS = ["uniform", "clustered", "offset", "duplicates", "lattice", "nan"]


def _clouds(kind, Q, T, seed):
    rng = np.random.default_rng(seed)
    uni = lambda n: rng.random((n, 3)) - 0.5                                       # noqa: E731
    if kind == "clustered":
        c = rng.normal(size=(5, 3)) * 0.3
        s = np.array([0.001, 0.01, 0.03, 0.1, 0.3])
        draw = lambda n: (lambda k: c[k] + s[k, None] * rng.normal(size=(n, 3)))(rng.integers(0, 5, n))   # noqa: E731
        q, t = draw(Q), draw(T)
    elif kind == "offset":                                                          # cancellation in q - t
        q, t = uni(Q) + 1e3, uni(T) + 1e3
    elif kind == "duplicates":                                                      # exact copies: the lowest index must win
        t = uni(T)
        t[T // 2:] = t[rng.integers(0, max(T // 2, 1), T - T // 2)]
        q = uni(Q)
        q[::3] = t[rng.integers(0, T, len(q[::3]))]                                 # and queries that sit on targets
    elif kind == "lattice":                                                         # many exact ties
        q, t = rng.integers(-4, 5, (Q, 3)) / 8.0, rng.integers(-4, 5, (T, 3)) / 8.0
    else:
        q, t = uni(Q), uni(T)
    q, t = q.astype(np.float32), t.astype(np.float32)
    if kind == "nan":
        t[T // 2, 1] = np.nan                                                       # never returned
    return q, t


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Q,T", SIZES)
def test_nn_search_equals_float32_oracle_bit_for_bit(Q, T, kind):
    import svr_amd  # noqa: F401
    from svr_amd.util.evaluate import distance_p2p
    q, t = _clouds(kind, Q, T, seed=Q * 7 + T)
    od, oi = E.nn_search(q, t)
    d, none, i = distance_p2p(q, t, None, None, return_index=True)                 # numpy in -> numpy out
    assert none is None and d.dtype == np.float32 and i.dtype == np.int32
    assert np.array_equal(i, oi) and np.array_equal(_bits(d), _bits(od))
    if kind == "nan":
        assert (T // 2) not in i.tolist() and ((i >= 0).all() or T == 1)
    if kind in ("duplicates", "lattice") and T > 1000 and Q > 1:
        assert (od == 0).any()
    qd, td = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    d1, _, i1 = distance_p2p(qd, td, None, None, return_index=True)                # device in -> device out
    assert d1.is_cuda and i1.is_cuda
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d2, _, i2 = distance_p2p(qd, td, None, None, return_index=True)
    side.synchronize()
    d3, _, i3 = distance_p2p(qd, td, None, None, return_index=True)                # a second run: bit-identical
    for dd, ii in ((d1, i1), (d2, i2), (d3, i3)):
        assert np.array_equal(ii.cpu().numpy(), oi) and np.array_equal(_bits(dd.cpu().numpy()), _bits(od))


def test_nn_search_full_size_every_50th_query():
    import svr_amd  # noqa: F401
    from svr_amd.util.evaluate import distance_p2p
    rng = np.random.default_rng(100000)
    def surface(n, r):                                                              # noqa: E306
        d = rng.normal(size=(n, 3))
        return (r * d / np.linalg.norm(d, axis=1, keepdims=True) + 0.003 * rng.normal(size=(n, 3))).astype(np.float32)
    q, t = surface(100000, 0.40), surface(100000, 0.41)
    d, _, i = distance_p2p(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), None, None, return_index=True)
    rows = np.arange(0, 100000, 50)
    od, oi = E.nn_search(q, t, rows=rows)
    assert np.array_equal(i.cpu().numpy()[rows], oi) and np.array_equal(_bits(d.cpu().numpy()[rows]), _bits(od))
    assert (i >= 0).all() and (i < 100000).all() and torch.isfinite(d).all()


def _golden_mesh(tag):
    z = np.load(os.path.join(GOLD, f"mesh_{tag}.npz"), allow_pickle=False)
    return np.asarray(z["vertices"], dtype=np.float64), np.asarray(z["faces"], dtype=np.int32)


def _mc_mesh(r=8.0, n=24):
    from svr_amd.util.visualize import marching_cubes
    v, f = marching_cubes(torch.from_numpy(MC.sphere(n, r)).cuda(), 0.0)
    return v, f


def _check_samples(v, f, uniforms, mesh=None):
    """Sampler == oracle for these uniforms: face equal, points bit-equal, every point its triangle's exact point rounded."""
    from svr_amd.util.evaluate import EvalMesh, sample_with_uniforms
    m = EvalMesh((v, f) if mesh is None else mesh)
    on, oc = E.face_table(v, f)
    assert np.array_equal(m.cum_area.cpu().numpy(), oc) and np.array_equal(m.face_normals.cpu().numpy(), on)
    pts, face, normals = sample_with_uniforms(m, torch.from_numpy(uniforms).cuda())
    op, of, exact, w1, w2 = E.sample(v, f, oc, uniforms, return_exact=True)
    pts, face = pts.cpu().numpy(), face.cpu().numpy()
    assert pts.dtype == np.float32 and face.dtype == np.int32
    assert np.array_equal(face, of) and np.array_equal(_bits(pts), _bits(op))
    assert np.array_equal(normals.cpu().numpy(), on[of])
    # inside its triangle within float32 rounding: valid weights, and the stored point is the exact one rounded once
    assert (w1 >= 0).all() and (w2 >= 0).all() and (w1 + w2 <= 1).all()
    assert np.all(np.abs(pts.astype(np.float64) - exact) <= 2.0 ** -24 * np.abs(exact) + 1e-45)
    area = np.diff(np.concatenate([[0.0], oc]))
    assert np.all(area[face] > 0)
    return face, area


@pytest.mark.parametrize("tag", ["sphere", "torus", "openbox", "marching_cubes"])
def test_sampler_equals_oracle_for_the_same_uniforms(tag):
    import svr_amd  # noqa: F401
    g = torch.Generator(device="cuda").manual_seed(17)
    u = torch.rand((100000, 3), device="cuda", dtype=torch.float64, generator=g).cpu().numpy()
    if tag == "marching_cubes":
        dv, df = _mc_mesh()
        v, f = dv.cpu().numpy().astype(np.float64), df.cpu().numpy()
        face, area = _check_samples(v, f, u, mesh=(dv, df))                         # the device pair implicit_to_mesh returns
    else:
        v, f = _golden_mesh(tag)
        face, area = _check_samples(v, f, u)
    assert len(np.unique(face)) > 0.5 * min((area > 0).sum(), 20000)


def test_sampler_never_draws_a_zero_area_face():
    import svr_amd  # noqa: F401
    rng = np.random.default_rng(3)
    v = rng.normal(size=(40, 3))
    f = rng.integers(0, 40, size=(200, 3)).astype(np.int32)
    f[0] = [4, 4, 4]
    f[10] = [5, 5, 9]
    f[12] = f[13] = f[50] = [1, 2, 30]
    f[100:120] = [7, 7, 7]
    f[-1] = [6, 6, 8]
    u = np.concatenate([rng.random((100000, 3)), [[0.0, 0.3, 0.3], [np.nextafter(1.0, 0.0), 0.9, 0.9], [1.0, 0.5, 0.5]]])
    face, area = _check_samples(v, f, u)
    assert (area == 0).sum() >= 23 and face[-1] == np.nonzero(area > 0)[0][-1]


def _chi2_quantile(dof, tail):
    """x with P(chi2_dof > x) = tail: bisection on the regularised upper incomplete gamma function."""
    sf = lambda x: float(torch.special.gammaincc(torch.tensor(dof / 2.0, dtype=torch.float64),      # noqa: E731
                                                 torch.tensor(x / 2.0, dtype=torch.float64)))
    lo, hi = 0.0, 10.0 * dof + 200.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if sf(mid) > tail else (lo, mid)
    return hi


def test_sampler_face_histogram_follows_the_areas():
    import svr_amd  # noqa: F401
    from svr_amd.util.evaluate import sample_surface
    v, f = _golden_mesh("openbox")
    n = 1000000
    _, face, _ = sample_surface((v, f), n, generator=torch.Generator(device="cuda").manual_seed(5))
    _, oc = E.face_table(v, f)
    area = np.diff(np.concatenate([[0.0], oc]))
    counts = np.bincount(face.cpu().numpy(), minlength=len(f)).astype(np.float64)
    nz = area > 0
    assert counts[~nz].sum() == 0
    expected = n * area[nz] / area[nz].sum()
    chi2 = float(((counts[nz] - expected) ** 2 / expected).sum())
    limit = _chi2_quantile(int(nz.sum()) - 1, 1e-6)
    assert expected.min() > 5 and chi2 < limit, (chi2, limit)
    assert abs(_chi2_quantile(10, 0.05) - 18.307) < 1e-2                           # the helper itself, against the tables


def test_eval_pointcloud_on_the_reference_golden():
    import svr_amd  # noqa: F401
    from svr_amd.util.evaluate import distance_p2p, eval_pointcloud
    z = golden()
    pred, gt, npred, ngt = (torch.from_numpy(z[k]).cuda() for k in ("pred", "gt", "normals_pred", "normals_gt"))
    _, a_dot, a_idx = distance_p2p(pred, gt, npred, ngt, return_index=True)
    _, c_dot, c_idx = distance_p2p(gt, pred, ngt, npred, return_index=True)
    assert np.array_equal(a_idx.cpu().numpy(), z["accuracy_idx"]) and np.array_equal(c_idx.cpu().numpy(), z["completeness_idx"])
    assert a_dot.dtype == torch.float64 and float(a_dot.min()) >= 0 and float(a_dot.max()) <= 1 + 1e-12
    assert np.allclose(a_dot.cpu().numpy(), E.normals_dot(z["normals_pred"], z["normals_gt"], z["accuracy_idx"]), rtol=0, atol=1e-15)
    want = ref_dict(z)
    got = eval_pointcloud(pred, gt, npred, ngt)
    assert all(isinstance(x, float) for x in got.values())
    assert_dict_close(got, want)
    assert_dict_close(eval_pointcloud(z["pred"], z["gt"], z["normals_pred"], z["normals_gt"]), want)          # numpy in
    again = eval_pointcloud(pred, gt, npred, ngt)
    assert all(got[k] == again[k] for k in E.KEYS if k != "iou") and np.isnan(again["iou"])                  # bit-reproducible
    nn = eval_pointcloud(pred, gt)
    assert np.isnan(nn["normals"]) and np.isnan(nn["normals accuracy"]) and np.isnan(nn["iou"]) and nn["chamfer_l2"] == got["chamfer_l2"]
    # a cloud against itself
    same = eval_pointcloud(pred, pred, npred, npred)
    d, _ = distance_p2p(pred, pred, None, None)
    assert float(d.abs().max()) == 0.0
    assert same["chamfer_l2"] == 0.0 and same["completeness"] == 0.0 and same["accuracy"] == 0.0
    assert abs(same["normals"] - 1.0) < 1e-6


def _contains(v, f, pts):
    return M.implicit_waterproofing(v, f, pts)[0]


def test_eval_mesh_equals_oracle_pipeline_for_the_same_uniforms():
    import svr_amd  # noqa: F401
    from svr_amd.util.evaluate import eval_mesh, eval_mesh_draws
    v1, f1 = M.icosphere(3, 0.30, (0.02, 0.0, -0.03))
    v2, f2 = M.icosphere(2, 0.33, (0.0, 0.01, 0.0))
    n = 2000
    got = eval_mesh(SimpleNamespace(vertices=v1, faces=f1), (v2, f2), -0.5, 0.5, n_points=n,
                    generator=torch.Generator(device="cuda").manual_seed(33))
    up, ug, ub = (u.cpu().numpy() for u in eval_mesh_draws(n, torch.Generator(device="cuda").manual_seed(33)))
    assert up.shape == (n, 3) and ub.shape == (10 * n, 3)
    want = E.eval_mesh((v1, f1), (v2, f2), -0.5, 0.5, up, ug, ub, _contains)
    assert got["iou"] == want["iou"] and 0.5 < want["iou"] < 0.9                   # integer counts of bit-exact booleans
    assert_dict_close({k: got[k] for k in E.KEYS if k != "iou"} | {"iou": float("nan")},
                      {k: want[k] for k in E.KEYS if k != "iou"} | {"iou": float("nan")})
    # a CPU generator seeds a device generator: reproducible too
    a = eval_mesh((v1, f1), (v2, f2), -0.5, 0.5, n_points=n, generator=torch.Generator().manual_seed(1))
    b = eval_mesh((v1, f1), (v2, f2), -0.5, 0.5, n_points=n, generator=torch.Generator().manual_seed(1))
    assert a == b and a != got


def test_eval_mesh_identity_and_concentric_spheres():
    import svr_amd  # noqa: F401
    from svr_amd.util.evaluate import eval_mesh
    n, r1, r2 = 64, 15.0, 20.0
    m1, m2 = _mc_mesh(r1, n), _mc_mesh(r2, n)                                       # device (vertices, faces) pairs, index space
    g = torch.Generator(device="cuda").manual_seed(2)
    same = eval_mesh(m2, m2, 0.0, float(n - 1), n_points=20000, generator=g)
    assert same["iou"] == 1.0 and same["chamfer_l2"] < 0.5 ** 2 and same["normals"] > 0.95
    out = eval_mesh(m1, m2, 0.0, float(n - 1), n_points=20000, generator=g)
    # whole chain: the slack is the lattice discretisation (a marching-cubes sphere is a polyhedron inscribed within a voxel)
    assert abs(out["iou"] - (r1 / r2) ** 3) < 0.05 * (r1 / r2) ** 3, out
    assert abs(out["completeness"] - (r2 - r1)) < 1.0 and abs(out["accuracy"] - (r2 - r1)) < 1.0, out
    assert out["normals"] > 0.95


def test_sample_points_mirror():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing.implicit_waterproofing import implicit_waterproofing
    from svr_amd.data_processing.mesh_occupancies import sample_points
    dims = (139, 104, 112)
    v, f = M.icosphere(3, 30.0, (139 / 2, 104 / 2, 112 / 2))                        # grid units, like the dataset's mesh.obj
    mesh = SimpleNamespace(vertices=v, faces=f)
    n, sigma = 5000, 0.01
    bp, occ, gc = sample_points(mesh, dims, n, sigma, generator=torch.Generator(device="cuda").manual_seed(4))
    assert bp.is_cuda and tuple(bp.shape) == (n + n // 10, 3) and tuple(gc.shape) == (n + n // 10, 3) and tuple(occ.shape) == (n + n // 10,)
    assert occ.dtype == torch.bool and bp.dtype == torch.float64
    assert torch.equal(gc, 2 * bp.flip(1)) and torch.equal(gc[:, 0], 2 * bp[:, 2]) and torch.equal(gc[:, 1], 2 * bp[:, 1])
    size = np.array(dims)
    norm = SimpleNamespace(vertices=(v + (-size / 2)) * (1 / size), faces=f)
    assert torch.equal(occ, implicit_waterproofing(norm, bp)[0])
    assert np.array_equal(occ.cpu().numpy(), M.implicit_waterproofing(norm.vertices, f, bp.cpu().numpy())[0])
    assert 0.2 < float(occ[:n].float().mean()) < 0.8                                # noise puts about half inside
    r = np.linalg.norm(bp[:n].cpu().numpy() * size - 0, axis=1)                     # surface samples lie near the sphere
    assert np.all(np.abs(r - 30.0) < 30.0 * 0.02 + 6 * sigma * size.max())
    assert float(bp[n:].abs().max()) <= 0.5
    bp2, occ2, gc2 = sample_points(mesh, dims, n, sigma, generator=torch.Generator(device="cuda").manual_seed(4))
    assert torch.equal(bp, bp2) and torch.equal(occ, occ2) and torch.equal(gc, gc2)
    bp3, _, _ = sample_points(mesh, dims, n, sigma, generator=torch.Generator(device="cuda").manual_seed(5))
    assert not torch.equal(bp, bp3)
