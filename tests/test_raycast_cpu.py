"""CPU: the ray-casting oracle (tests/raycast_oracle.py, the numpy restatement of include/svr_hip.h's svr_raycast_* rule)
against an independent routine and an analytic bound, the rule's corner cases, the conservativeness of the face
rectangles, the distance round trip, the pair routine of csrc/raycast_pair.h compiled for the host, and the new
arguments of process_sample."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import raycast_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
CSRC = os.path.join(REPO, "single-view-3d-reconstruction_amd", "csrc")
EPS = np.finfo(np.float64).eps


def _mesh(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z["vertices"].astype(np.float64), z["faces"].astype(np.int32)


def _in_view(name, consts, at=(0.0, 0.0, 2.0)):
    """The committed mesh scaled to a largest |coordinate| of 0.6 m and placed at camera-space `at`, in grid units."""
    V, F = _mesh(name)
    return O.camera_to_grid(V * (0.6 / np.abs(V).max()) + np.asarray(at), consts), F


def _pixels(H, W):
    rows, cols = (a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    return rows, cols


def _norm(x):
    return np.sqrt((x * x).sum(-1))


def _independent(o, d, tri):
    """(P, F): intersect the ray with the face's plane and take the barycentric coordinates of the point from the
    sub-triangle normals.  None of the oracle's p, q, det.  -> z (NaN = no hit), the three coordinates (P, F, 3)."""
    a, b, c = tri[None, :, 0:3], tri[None, :, 3:6], tri[None, :, 6:9]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        z = ((a - o) * n).sum(-1) / (d[:, None, :] * n).sum(-1)
        x = o + z[..., None] * d[:, None, :]
        w = np.stack([(np.cross(b - x, c - x) * n).sum(-1) / nn, (np.cross(c - x, a - x) * n).sum(-1) / nn,
                      (np.cross(a - x, b - x) * n).sum(-1) / nn], axis=-1)
        hit = (w >= 0).all(-1) & (z > 0)
    return np.where(hit, z, np.nan), w


@pytest.mark.parametrize("name", ["mesh_sphere", "mesh_torus", "mesh_openbox"])
def test_oracle_agrees_with_an_independent_routine(name):
    """Every pixel of a 60 x 80 view of the mesh, every face.  With kappa = |d| s' max(|e1|, |e2|) / |det|, s' =
    max(|o - a|, |e1|, |e2|), the conditioning of the pair (1 / kappa is the sine of the angle between ray and face times the
    face's aspect):  a barycentric coordinate is a quotient of a triple product by det, each a chain of at most ~16 rounded
    float64 operations on terms bounded by |d| s' |e|, so each routine's coordinate is within 16 eps kappa of the true
    one; two routines give 32, and the independent routine carries the rounding of its plane point through both factors
    of a cross product: 64 eps kappa.  z = (e2 . q) / det has the same chain with |e1| |e2| s' / |det| in place of kappa, and
    the error of det contributes |z| times its relative error: 64 eps (s' |e1| |e2| + |z| |d| |e1| |e2|) / |det|.
    Pairs both routines accept agree on z within that bound; a pair whose verdicts differ has one of the rule's coordinates
    (bu, bv, 1 - bu - bv) within the bound of 0; the pixels with such a pair are at most 1 % (the share is printed).
    Such pixels are real here, not noise: the torus is seen along its axis and has edges in 40 planes through it, two of
    which hold the image's diagonals, so the diagonal pixels' rays run through edges exactly (coordinates of 1e-16) and
    the two routines round them to different sides.  They are a one-dimensional set: 1.33 % of a 30 x 40 view, 0.60 % of
    this one."""
    H, W = 60, 80
    consts = O.make_consts(H, W)
    V, F = _in_view(name, consts)
    tri = O.triangle_table(V, F)
    rows, cols = _pixels(H, W)
    o, d = O.ray_directions(cols, rows, consts)
    z, det, bu, bv = O.pair_details(o, d, tri)
    zi, _ = _independent(o, d, tri)
    e1, e2, s = tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3], o - tri[:, 0:3]
    sp = np.maximum(_norm(s), np.maximum(_norm(e1), _norm(e2)))[None, :]
    dn = _norm(d)[:, None]
    with np.errstate(all="ignore"):
        kappa = dn * sp * np.maximum(_norm(e1), _norm(e2))[None, :] / np.abs(det)
        bound_b = 64 * EPS * kappa
    both = ~np.isnan(z) & ~np.isnan(zi)
    assert both.sum() > 100
    with np.errstate(all="ignore"):
        bound_z = 64 * EPS * (sp + np.abs(z) * dn) * (_norm(e1) * _norm(e2))[None, :] / np.abs(det)
    ratio = (np.abs(z - zi)[both] / bound_z[both]).max()
    differ = np.isnan(z) != np.isnan(zi)
    share = differ.any(axis=1).mean()
    print(f"{name}: {both.sum()} common hits, max |z - z'| / bound = {ratio:.3f}, pixels with a differing pair {100 * share:.3f} %")
    assert ratio <= 1.0
    near_border = np.minimum(np.minimum(np.abs(bu), np.abs(bv)), np.abs(1.0 - bu - bv))
    assert (near_border[differ] <= bound_b[differ]).all()
    assert share <= 0.01
    # per pixel, away from the differing pairs: the same verdict and the same depth
    best, face = O.cast(tri, consts, cols, rows)
    clean = ~differ.any(axis=1)
    zi_best = np.where(np.isnan(zi), np.inf, zi).min(axis=1)
    assert np.array_equal(np.isinf(best[clean]), np.isinf(zi_best[clean]))
    hit = clean & (face >= 0)
    assert 0.1 <= (face >= 0).mean() <= 0.9
    assert (np.abs(best[hit] - zi_best[hit]) <= bound_z[np.nonzero(hit)[0], face[hit]]).all()


def _sphere_depth(o, d, centre, rho):
    """The smaller root of |o + z d - centre| = rho per ray; NaN where the ray misses the sphere."""
    oc = o - centre
    A, B, Cc = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum(-1) - rho * rho
    with np.errstate(invalid="ignore"):
        return (-B - np.sqrt(B * B - A * Cc)) / A


def test_oracle_sphere_bound():
    """Icosphere with centre c0, circumradius R and inradius r_in: the surface lies in the shell r_in <= |x - c0| <= R and
    encloses the inner ball, so a ray that reaches the inner sphere at z_in enters the outer one at z_out <= depth <= z_in,
    and a ray that misses the outer sphere misses the mesh.  (The camera -> grid affine scales every axis by 20: spheres stay
    spheres.)  Slack: 2^-23 relative for the float32 depth."""
    H, W = 48, 64
    consts = O.make_consts(H, W)
    V, F = _mesh("mesh_sphere")
    c0 = 0.5 * (V.min(0) + V.max(0))
    V = (V - c0) * (0.6 / np.abs(V - c0).max()) + np.array([0.0, 0.0, 2.0])
    Vg, cg = O.camera_to_grid(V, consts), O.camera_to_grid(np.array([[0.0, 0.0, 2.0]]), consts)[0]
    rad = _norm(Vg - cg)
    R = rad.max()
    assert rad.min() > R * (1 - 1e-6), "not an icosphere about the centre of its bounding box"
    tri = O.triangle_table(Vg, F)
    a, n = tri[:, 0:3], np.cross(tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3])
    r_in = (np.abs(((a - cg) * n).sum(-1)) / _norm(n)).min()
    assert 0 < r_in < R
    rows, cols = _pixels(H, W)
    out = O.maps_at(tri, consts, H, W, rows, cols)
    o, d = O.ray_directions(cols, rows, consts)
    z_out, z_in = _sphere_depth(o, d, cg, R), _sphere_depth(o, d, cg, r_in)
    depth, hit = out["depth"].astype(np.float64), out["face"] >= 0
    inner = ~np.isnan(z_in)
    assert inner.sum() > 100 and hit[inner].all() and not hit[np.isnan(z_out)].any()
    tol = 2.0 ** -23
    assert (depth[inner] >= z_out[inner] * (1 - tol)).all() and (depth[inner] <= z_in[inner] * (1 + tol)).all()
    assert (depth[hit] >= z_out[hit] * (1 - tol)).all()
    print(f"sphere: R={R:.4f} r_in={r_in:.4f} grid units, {inner.sum()} rays through the inner sphere, {hit.sum()} hits")


def _facing(consts, z=2.0, half=0.5):
    """A triangle across the optical axis at depth z, in grid units."""
    return O.camera_to_grid(np.array([[-half, -half, z], [half, -half, z], [0.0, half, z]]), consts)


def test_oracle_rules():
    H, W = 9, 12
    consts = O.make_consts(H, W)
    rows, cols = _pixels(H, W)
    A = _facing(consts)
    one = O.maps_at(O.triangle_table(A, [[0, 1, 2]]), consts, H, W, rows, cols)
    assert (one["face"] == 0).any() and (one["face"] == -1).any()
    centre = (rows == H // 2) & (cols == W // 2)
    assert abs(one["depth"][centre][0] - 2.0) < 1e-6
    assert (one["depth"][one["face"] < 0] == 0).all() and (one["normal"][one["face"] < 0] == 0).all()
    hit = one["face"] == 0
    # the normal is a unit vector turned towards the camera (here -z in grid space, whichever the winding)
    assert np.allclose(one["normal"][hit], [0, 0, -1], atol=1e-6)
    flipped = O.maps_at(O.triangle_table(A, [[0, 2, 1]]), consts, H, W, rows, cols)
    assert np.allclose(flipped["normal"][hit], [0, 0, -1], atol=1e-6) and np.array_equal(flipped["face"], one["face"])
    assert one["shade"][centre][0] == 255 and (one["shade"][~hit] == 0).all() and (one["shade"][hit] > 200).all()
    # coincident faces: the lower index wins
    two = O.maps_at(O.triangle_table(A, [[0, 1, 2], [0, 1, 2]]), consts, H, W, rows, cols)
    assert np.array_equal(two["face"], one["face"]) and np.array_equal(two["depth"].view(np.int32), one["depth"].view(np.int32))
    # zero-area faces (a repeated vertex: det is exactly 0) in front never win
    Vz = np.concatenate([A, O.camera_to_grid(np.array([[0.0, 0.0, 1.0], [0.1, 0.0, 1.0]]), consts)])
    mixed = O.maps_at(O.triangle_table(Vz, [[3, 3, 4], [3, 4, 4], [3, 3, 3], [0, 1, 2]]), consts, H, W, rows, cols)
    assert np.array_equal(mixed["face"] == 3, hit) and np.array_equal(mixed["depth"].view(np.int32), one["depth"].view(np.int32))
    # an exactly edge-on face: it contains the camera centre, so det = e1 . (d x e2) is 0 for every ray up to rounding --
    # with the centre as vertex a and the two others along exactly representable directions it is 0 exactly
    k = consts.astype(np.float64)
    edge_on = np.array([[k[4], k[6], k[8]], [k[4], k[6], k[8] + 64.0], [k[4] + 32.0, k[6], k[8] + 64.0]])
    o, d = O.ray_directions(cols, rows, consts)
    z, det, _, _ = O.pair_details(o, d, O.triangle_table(edge_on, [[0, 1, 2]]))
    on_plane = d[:, 1] == 0.0
    assert np.isnan(z).all() and (det[on_plane] == 0.0).all()
    # a face behind the camera never hits
    behind = O.maps_at(O.triangle_table(_facing(consts, z=-2.0), [[0, 1, 2]]), consts, H, W, rows, cols)
    assert (behind["face"] == -1).all()
    # near / far / miss
    assert (O.maps_at(O.triangle_table(A, [[0, 1, 2]]), consts, H, W, rows, cols, near=2.5)["face"] == -1).all()
    assert (O.maps_at(O.triangle_table(A, [[0, 1, 2]]), consts, H, W, rows, cols, far=1.5)["face"] == -1).all()
    both = np.concatenate([_facing(consts, 1.0, 0.2), A])
    layered = O.triangle_table(both, [[0, 1, 2], [3, 4, 5]])
    front = O.maps_at(layered, consts, H, W, rows, cols)
    cut = O.maps_at(layered, consts, H, W, rows, cols, near=1.5, miss=-1.0)
    assert (front["face"] == 0).any() and not (cut["face"] == 0).any() and np.array_equal(cut["face"] == 1, hit)
    assert (cut["depth"][cut["face"] < 0] == -1.0).all() and (cut["distance"][cut["face"] < 0] < 0).all()


def test_host_checks_and_transform_need_no_device():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import render_view as R
    from svr_amd.data_processing.mesh_to_df import triangle_table
    from svr_amd.data_processing.process_sample import EmptyMeshError
    V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.5, 2.0]])
    F = np.array([[0, 1, 2], [1, 2, 3]])
    bad = V.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        triangle_table(R.transformed((bad, F), None))
    with pytest.raises(ValueError, match="outside the 4 vertices"):
        triangle_table(R.transformed((V, np.array([[0, 1, 4]])), None))
    with pytest.raises(EmptyMeshError):
        triangle_table(R.transformed((V, np.zeros((0, 3), np.int32)), np.eye(4)))
    # transform = M is the documented expression, row by row
    rng = np.random.default_rng(3)
    M = np.eye(4)
    M[:3] = rng.normal(size=(3, 4)) * [1, 1, 1, 30]
    Vt, Ft = R.transformed((V, F), M)
    want = O.transform_vertices(V, M)
    assert np.array_equal(Vt.view(np.int64), want.view(np.int64)) and np.array_equal(Ft, F)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    assert np.array_equal(want[:, 1], ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3])
    # so rendering with transform = M is rendering the transformed mesh: the same triangle table goes to the device
    assert np.array_equal(triangle_table(R.transformed((V, F), M)), O.triangle_table(want, F))
    with pytest.raises(ValueError, match="4x4"):
        R.transformed((V, F), np.eye(3))
    # the constants: 12 numbers as given, or those of the default intrinsic
    assert np.array_equal(R.view_consts(consts=np.arange(12)), np.arange(12, dtype=np.float32))
    k = R.view_consts()
    assert k.dtype == np.float32 and np.allclose(k[:9], [277.1281435, 159.5, 119.5, 20, 69.0655, 20, 51.745, 20, -8], atol=1e-3)
    with pytest.raises(ValueError, match="need 12"):
        R.view_consts(consts=[1.0, 2.0])


def test_face_rectangles_are_conservative():
    """Random triangles -- in view, crossing the camera plane, far off screen, slivers -- against every pixel of a 24 x 32
    image: every (pixel, face) pair the rule accepts lies in the face's rectangle (an "every tile" face has the rectangle
    +-2^30).  The test also pins that the rectangles do cull: a face far off screen has one that misses the image."""
    H, W = 24, 32
    consts = O.make_consts(H, W)
    rng = np.random.default_rng(17)
    n = 400
    centre = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-0.5, 4.0, n)], axis=1)
    size = rng.choice([0.05, 0.3, 1.5], size=n)[:, None, None]
    cam = centre[:, None, :] + size * rng.normal(size=(n, 3, 3))
    cam[:40, 1, :] = cam[:40, 0, :] + 1e-3 * (cam[:40, 1, :] - cam[:40, 0, :])          # slivers
    tri = O.camera_to_grid(cam.reshape(-1, 3), consts).reshape(n, 9)
    rect = O.face_rects(tri, consts)
    every = rect[:, 0] == -O.RECT_MAX
    crossing = (cam[:, :, 2].min(1) <= 0) & (cam[:, :, 2].max(1) > 0)
    assert crossing.sum() > 20 and every[crossing].all() and (~every).sum() > 100
    rows, cols = _pixels(H, W)
    o, d = O.ray_directions(cols, rows, consts)
    accepted = ~np.isnan(O.pair_z(o, d, tri))
    inside = (cols[:, None] >= rect[None, :, 0]) & (cols[:, None] <= rect[None, :, 1]) \
        & (rows[:, None] >= rect[None, :, 2]) & (rows[:, None] <= rect[None, :, 3])
    print(f"rectangles: {accepted.sum()} accepted pairs, {accepted[:, every].sum()} of them on every-tile faces, "
          f"{inside.sum()} pairs inside a rectangle of {inside.size}")
    assert accepted.sum() > 2000 and accepted[:, crossing].sum() > 0
    assert not (accepted & ~inside).any()
    off_screen = ~every & ((rect[:, 1] < 0) | (rect[:, 0] >= W) | (rect[:, 3] < 0) | (rect[:, 2] >= H))
    assert off_screen.sum() > 20 and not accepted[:, off_screen].any()
    assert inside[:, ~every].mean() < 0.5


def test_distance_round_trip():
    """distance = depth * sqrt(t) and svr_distance_to_depth's sqrt(distance^2 / t) share t = rc / (f f) + 1 bit for bit, so the
    round trip carries five roundings: sqrt(t) (1), the product (1), the square and the quotient (each halved by the
    square root that follows: 1/2 + 1/2) and that square root (1) -- 4 * 2^-24 relative."""
    H, W = 240, 320
    rows, cols = _pixels(H, W)
    rng = np.random.default_rng(1)
    depth = rng.uniform(0.4, 6.0, size=H * W).astype(np.float32)
    f = np.float32(277.1281435)
    distance = (depth * O.distance_factor(H, W, f, rows, cols)).astype(np.float32)
    assert distance.dtype == np.float32 and (distance >= depth).all()
    back = O.distance_to_depth(distance, H, W, f, rows, cols)
    rel = np.abs(back.astype(np.float64) - depth.astype(np.float64)) / depth.astype(np.float64)
    print(f"distance round trip: max relative error {rel.max() / 2.0 ** -24:.2f} * 2^-24")
    assert rel.max() <= 4 * 2.0 ** -24


PAIR_MAIN = r"""
// stand-alone host check of csrc/raycast_pair.h: reads records of 17 doubles (o, d, a, b, c, near, far) from argv[1],
// writes two doubles per record (1 / 0 for the verdict, z or 0) to argv[2]
#include <cstdio>
#include <vector>
#include "raycast_pair.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<double> out;
  double r[17];
  while (std::fread(r, sizeof(double), 17, in) == 17) {
    double z = 0.0;
    const bool hit = svr::ray_triangle(r, r + 3, r + 6, r[15], r[16], &z);
    out.push_back(hit ? 1.0 : 0.0);
    out.push_back(hit ? z : 0.0);
  }
  std::fclose(in);
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), o) == out.size();
  return std::fclose(o) == 0 && ok ? 0 : 5;
}
"""


def test_pair_routine_compiled_for_the_host_equals_the_oracle(tmp_path):
    """csrc/raycast_pair.h -- the function every kernel calls -- built with g++ -O2 -ffp-contract=off into a program with
    its own main, on 100 000 (ray, triangle) pairs: verdict and z equal the oracle's bit for bit."""
    rng = np.random.default_rng(23)
    n = 100_000
    consts = O.make_consts(240, 320, f=277.1281435, cx=159.5, cy=119.5)
    o, d = O.ray_directions(rng.integers(0, 320, n), rng.integers(0, 240, n), consts)
    # a triangle around a point of the ray (most pairs near a hit, many near an edge), some rays with their own near / far
    zc = rng.uniform(0.3, 6.0, n)
    on_ray = o + zc[:, None] * d
    spread = rng.choice([0.02, 1.0, 20.0], size=n)[:, None, None]
    tri = (on_ray[:, None, :] + spread * rng.normal(size=(n, 3, 3))).reshape(n, 9)
    tri[:500, 3:6] = tri[:500, 0:3]                                                    # zero area
    tri[500:1000, 0:3] = o                                                             # the camera centre as a vertex
    near = np.where(rng.random(n) < 0.2, zc * rng.uniform(0.5, 1.5, n), 0.0)
    far = np.where(rng.random(n) < 0.2, zc * rng.uniform(0.8, 2.0, n), np.inf)
    want = O.pair_details(o, d, tri, near, far, pairwise=True)[0]
    rec = np.concatenate([np.broadcast_to(o, (n, 3)), d, tri, near[:, None], far[:, None]], axis=1)
    (tmp_path / "main.cpp").write_text(PAIR_MAIN)
    rec.astype("<f8").tofile(tmp_path / "pairs.bin")
    exe = tmp_path / "pair_check"
    r = subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", CSRC, str(tmp_path / "main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path / "pairs.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.fromfile(tmp_path / "out.bin", dtype="<f8").reshape(n, 2)
    hit = ~np.isnan(want)
    print(f"host pair routine: {hit.sum()} of {n} pairs accepted")
    assert 0.05 * n < hit.sum() < 0.95 * n
    assert np.array_equal(got[:, 0] == 1.0, hit)
    assert np.array_equal(got[hit, 1].view(np.int64), want[hit].view(np.int64))


def test_process_sample_render_missing_defaults_to_false():
    import svr_amd  # noqa: F401
    from svr_amd.data_processing import process_sample as P
    for fn in (P.process_sample, P.process_sample_pipeline):
        assert inspect.signature(fn).parameters["render_missing"].default is False
        assert inspect.signature(fn).parameters["scene_mesh"].default is None
