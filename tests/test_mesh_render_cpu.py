"""CPU: the mesh-preview oracle (tests/mesh_render_oracle.py, the numpy restatement of include/svr_hip.h's
svr_mesh_vertex_normals / svr_mesh_shade / svr_box_downsample_rgb8 rules) against what the rules promise, the pixel routine of
csrc/shade_pixel.h compiled for the host (plain and under the host sanitizers), and the two new file writers built with g++."""
import os
import subprocess

import numpy as np
import pytest

from tests import _mesh_render_cases as K
from tests import mesh_render_oracle as O
from tests import raycast_oracle as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "single-view-3d-reconstruction_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _no_gpu_or_skip():
    import torch
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds run on the CPU machine only")


def test_octahedron_normals_are_the_axes():
    v, f = K.case("octahedron")
    got = O.vertex_normals(v, f)
    assert got.counts == [6, 0, 0] and np.array_equal(got.normals, (v / np.float32(2.0)).astype(np.float32))
    assert np.array_equal(np.signbit(got.normals) & (got.normals != 0), v < 0)


@pytest.mark.parametrize("name", K.CASES)
def test_states_counts_and_unit_length(name):
    if name == "mc_sphere":
        import __graft_entry__ as ge
        ge.build()                                   # mc_oracle takes the case table from the library
    v, f = K.case(name)
    got = O.vertex_normals(v, f)
    assert got.normals.dtype == np.float32 and got.normals.shape == v.shape and got.state.shape == (len(v),)
    assert sum(got.counts) == len(v) and set(np.unique(got.state)) <= {0, 1, 3}
    has = got.state == O.HAS_NORMAL
    length = np.sqrt((got.normals[has].astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(length - 1.0) <= 2.0 ** -23).all(), np.abs(length - 1.0).max()
    assert not got.normals[~has].any()
    valid = O.valid_faces(v, f)
    in_a_face = np.zeros(len(v), dtype=bool)
    in_a_face[np.asarray(f, dtype=np.int64)[valid].reshape(-1)] = True
    assert not has[~in_a_face].any() and np.array_equal(got.state == O.BAD, ~O.usable(v))
    expect = {"coincident": [0, 3, 0], "no_vertices": [0, 0, 0], "no_faces": [0, 70, 0], "faces_without_vertices": [0, 0, 0],
              "cube": [8, 0, 0], "lone_vertex": [8, 1, 0], "fan": [41, 0, 0]}
    if name in expect:
        assert got.counts == expect[name]
    if name == "bad":
        assert got.counts[2] == 3 and got.state[17] != O.BAD
    if name == "mc_sphere":                          # closed and outward: every normal points away from the centre
        assert has.all() and len(v) > 100
        assert ((got.normals * (v - np.float32(5.5))).sum(axis=1) > 0).all()


@pytest.mark.parametrize("name", ["cube", "strip", "fan", "bad", "coincident"])
def test_face_order_and_rotation_change_no_bit(name):
    want = K.oracle(name)
    for seed in (5, 6):
        v, g = K.shuffled(name, seed)
        got = O.vertex_normals(v, g)
        assert np.array_equal(got.sums, want.sums) and np.array_equal(got.state, want.state) and got.counts == want.counts
        assert np.array_equal(got.normals.view(np.uint32), want.normals.view(np.uint32))


def test_sums_wrap_like_int64():
    """Vertex 0 in 600 large coplanar faces of one winding: the exact sum leaves int64, the rule's is its two's-complement wrap."""
    big = np.float32(65535.0)
    v = np.array([[-big, -big, 0], [big, -big, 0], [big, big, 0]], dtype=np.float32)
    f = np.tile(np.array([[0, 1, 2]], dtype=np.int32), (600, 1))
    got = O.vertex_normals(v, f)
    q = int(np.rint(np.float64(big) * 1024))
    exact = 600 * (2 * q) * (2 * q)
    assert exact > 2 ** 63 and int(got.sums[0, 2]) == ((exact + 2 ** 63) % 2 ** 64) - 2 ** 63
    assert got.counts == [3, 0, 0]


# ---- the pixel routine, compiled for the host ------------------------------------------------------------------------------------
SHADE_MAIN = r"""
// stand-alone host check of csrc/shade_pixel.h.  argv[1]: a header of 4 int64 (F, V, P, flags: 1 = normals, 2 = colors), then
// tri (F, 9) f64, faces (F, 3) i32, normals (V, 3) f32, colors (V, 3) u8, k (9) f64, ambient f64, albedo 3 u8, background 3 u8,
// then P records of 3 int32 (u, v, face).  argv[2]: P x 3 bytes.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "shade_pixel.h"

template <class T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<int64_t> head;
  std::vector<double> tri, k, ambient;
  std::vector<int32_t> faces, px;
  std::vector<float> normals;
  std::vector<uint8_t> colors, albedo, background;
  if (!rd(in, head, 4)) return 4;
  const int64_t F = head[0], V = head[1], P = head[2], flags = head[3];
  if (!(rd(in, tri, F * 9) && rd(in, faces, F * 3) && rd(in, normals, V * 3) && rd(in, colors, V * 3) && rd(in, k, 9) && rd(in, ambient, 1) &&
        rd(in, albedo, 3) && rd(in, background, 3) && rd(in, px, P * 3)))
    return 5;
  std::fclose(in);
  std::vector<uint8_t> out(P * 3);
  for (int64_t i = 0; i < P; ++i)
    svr::shade_pixel(px[i * 3], px[i * 3 + 1], px[i * 3 + 2], tri.data(), faces.data(), F, V, (flags & 1) ? normals.data() : nullptr,
                     (flags & 2) ? colors.data() : nullptr, k.data(), albedo.data(), background.data(), ambient[0], &out[i * 3]);
  FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  const bool ok = std::fwrite(out.data(), 1, out.size(), o) == out.size();
  return std::fclose(o) == 0 && ok ? 0 : 7;
}
"""


def _shade_job(n=10_000):
    """10^4 (pixel, face) pairs on the placed sphere at 24 x 32: the face the ray caster gives, a random face of the mesh (its
    barycentrics then lie outside the face: the rule is still defined), misses, and face / vertex indices out of range."""
    H, W = 24, 32
    consts = R.make_consts(H, W)
    v, f = K.placed("mc_sphere", consts)
    f = np.array(f)
    f[7] = [0, len(v), 1]                              # a vertex index out of range: flat normal, albedo
    f[11] = [-1, 2, 3]
    normals = O.vertex_normals(v, f).normals.copy()
    normals[f[20]] = 0                                 # an interpolated normal of length 0: the face's own
    normals[f[21, 0]] = np.nan
    rng = np.random.default_rng(77)
    u, r = rng.integers(0, W, n), rng.integers(0, H, n)
    tri = v.astype(np.float64)[np.clip(f, 0, len(v) - 1)].reshape(-1, 9)
    _, hit = R.cast(tri, consts, u, r)
    face = np.where(rng.random(n) < 0.6, hit, rng.integers(0, len(f), n)).astype(np.int32)
    face[:200] = rng.choice([7, 11, 20, 21], 200)
    face[200:260] = rng.choice([-1, -2 ** 31, len(f), 2 ** 31 - 1], 60)
    return dict(H=H, W=W, consts=consts, tri=tri, faces=f.astype(np.int32), V=len(v), normals=normals,
                colors=K.vertex_palette(len(v)), u=u, v=r, face=face)


def _write_job(path, j, flags, ambient, albedo, background):
    k = np.asarray(j["consts"], dtype=np.float32).astype(np.float64)[:9]
    with open(path, "wb") as fh:
        np.array([len(j["tri"]), j["V"], len(j["face"]), flags], dtype="<i8").tofile(fh)
        j["tri"].astype("<f8").tofile(fh)
        j["faces"].astype("<i4").tofile(fh)
        j["normals"].astype("<f4").tofile(fh)
        j["colors"].astype(np.uint8).tofile(fh)
        k.astype("<f8").tofile(fh)
        np.array([np.float64(np.float32(ambient))]).astype("<f8").tofile(fh)
        np.array(albedo, dtype=np.uint8).tofile(fh)
        np.array(background, dtype=np.uint8).tofile(fh)
        np.stack([j["u"], j["v"], j["face"]], axis=1).astype("<i4").tofile(fh)


@pytest.fixture(scope="module")
def shade_job():
    import __graft_entry__ as ge
    ge.build()
    return _shade_job()


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_pixel_routine_compiled_for_the_host_equals_the_oracle(shade_job, tmp_path, variant):
    """csrc/shade_pixel.h -- the function the kernel calls per pixel -- built with g++ -O2 -ffp-contract=off into a program with
    its own main: the bytes equal the oracle's on 10 000 (pixel, face) pairs, with and without normals and colours; the same
    program built with -fsanitize=address,undefined and run on its own reports nothing."""
    if variant == "sanitized":
        _no_gpu_or_skip()
    j = shade_job
    (tmp_path / "main.cpp").write_text(SHADE_MAIN)
    exe = tmp_path / ("shade_" + variant)
    cmd = ["g++", "-O2", "-g", "-ffp-contract=off", "-std=c++17"] + (SANITIZE if variant == "sanitized" else [])
    r = subprocess.run(cmd + ["-I", CSRC, str(tmp_path / "main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = set()
    for flags, ambient, albedo, background in ((0, 0.25, (200, 200, 200), (255, 255, 255)), (1, 0.25, (200, 180, 90), (0, 0, 0)),
                                               (2, 0.0, (1, 2, 3), (9, 8, 7)), (3, 1.0, (200, 200, 200), (255, 255, 255)),
                                               (3, 0.3, (200, 200, 200), (10, 20, 30))):
        _write_job(tmp_path / "job.bin", j, flags, ambient, albedo, background)
        r = subprocess.run([str(exe), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        got = np.fromfile(tmp_path / "out.bin", dtype=np.uint8).reshape(-1, 3)
        want = O.shade_pixels(j["tri"], j["faces"], j["V"], j["face"], j["u"], j["v"], j["consts"], j["normals"] if flags & 1 else None,
                              j["colors"] if flags & 2 else None, ambient, albedo, background)
        differ = np.flatnonzero((got != want).any(axis=1))
        assert len(differ) == 0, (flags, len(differ), differ[:5], got[differ[:5]], want[differ[:5]])
        seen.add(want.tobytes())
        assert (want == np.array(background, dtype=np.uint8)).all(axis=1).sum() >= 60
    assert len(seen) == 5


def test_shader_promises():
    """What the rule says in words, on the oracle: misses take the background; ambient 1 gives the base colour; the head light
    is brightest where the surface faces the camera; flat and smooth agree on a face seen with the face's own normal at its
    corners; a single colour at every vertex is the albedo of that colour."""
    import __graft_entry__ as ge
    ge.build()
    H, W = 24, 32
    consts = R.make_consts(H, W)
    v, f = K.placed("mc_sphere", consts)
    n = O.vertex_normals(v, f).normals
    flat = O.render(v, f, consts, (H, W))
    smooth = O.render(v, f, consts, (H, W), normals=n)
    depth = R.render(v, f, consts, (H, W))
    miss = depth["face"] < 0
    assert miss.any() and (~miss).sum() > 60
    assert (flat[miss] == 255).all() and (smooth[miss] == 255).all()
    assert (smooth[~miss] <= 200).all() and (smooth[~miss] >= 50).all()          # 200 (0.25 + 0.75 c), c in [0, 1]
    assert smooth[H // 2, W // 2, 0] >= 195 and smooth[~miss].min() < 150        # facing the camera / grazing at the rim
    assert np.array_equal(flat[..., 0], flat[..., 1]) and not np.array_equal(flat, smooth)
    full = O.render(v, f, consts, (H, W), normals=n, ambient=1.0, albedo=(10, 100, 250))
    assert (full[~miss] == np.array([10, 100, 250], dtype=np.uint8)).all()
    one = np.tile(np.array([[30, 60, 90]], dtype=np.uint8), (len(v), 1))
    painted = O.render(v, f, consts, (H, W), normals=n, colors=one)
    plain = O.render(v, f, consts, (H, W), normals=n, albedo=(30, 60, 90))
    assert (np.abs(painted.astype(int) - plain.astype(int)) <= 1).all()          # w0 + bu + bv is 1 to rounding
    # the face's own unit normal at its three corners: smooth shading of that face is flat shading
    tri_v = v[f[0]]
    e1, e2 = (tri_v[1] - tri_v[0]).astype(np.float64), (tri_v[2] - tri_v[0]).astype(np.float64)
    m = np.cross(e1, e2)
    own = np.tile((m / np.linalg.norm(m)).astype(np.float32), (3, 1))
    fm = np.zeros((H, W), dtype=np.int64).reshape(-1)
    a = O.render(tri_v, [[0, 1, 2]], consts, (H, W), normals=own, face_map=fm)
    b = O.render(tri_v, [[0, 1, 2]], consts, (H, W), face_map=fm)
    assert (np.abs(a.astype(int) - b.astype(int)) <= 1).all()


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_box_downsample_is_the_mean_rounded_half_up(s):
    rng = np.random.default_rng(50 + s)
    fine = rng.integers(0, 256, (5 * s, 7 * s, 3)).astype(np.uint8)
    fine[:s, :s] = 255
    fine[s:2 * s, :s] = 0
    if s == 2:
        fine[:2, 2:4, 0] = [[1, 0], [1, 0]]              # a mean of exactly 0.5 rounds up
    got = O.box_downsample(fine, s)
    mean = fine.reshape(5, s, 7, s, 3).astype(np.float64).mean(axis=(1, 3))
    assert got.shape == (5, 7, 3) and got.dtype == np.uint8 and np.array_equal(got, np.floor(mean + 0.5).astype(np.uint8))
    assert (got[0, 0] == 255).all() and (got[1, 0] == 0).all()
    if s == 2:
        assert got[0, 1, 0] == 1
    if s == 1:
        assert np.array_equal(got, fine)


def test_ssaa_constants_put_the_sub_pixels_where_the_header_says():
    consts = R.make_consts(13, 19, f=17.3, cx=8.7, cy=6.1)
    for s in (1, 2, 3, 4):
        k = O.ssaa_consts(consts, s)
        assert k.dtype == np.float32 and np.array_equal(k[3:], consts[3:])
        f, cx = np.float64(consts[0]), np.float64(consts[1])
        for u in (0, 7, 18):
            for i in range(s):
                fine = ((s * u + i) - np.float64(k[1])) / np.float64(k[0])
                coarse = ((u + (i - (s - 1) / 2) / s) - cx) / f
                assert abs(fine - coarse) <= 2.0 ** -20
    assert np.array_equal(O.ssaa_consts(consts, 1), consts)


def test_python_layer_checks_need_no_device():
    import __graft_entry__ as ge
    ge.build()
    import svr_amd  # noqa: F401
    from svr_amd.util import mesh_render as M
    n = K.oracle("cube").normals
    turn = M.orbit_transform(*K.case("cube"), 25.0, 10.0, 1.5, consts=R.make_consts(24, 32))
    assert np.array_equal(M.transform_normals(n, turn).view(np.uint32), O.transform_normals(n, turn).view(np.uint32))
    assert np.allclose(turn[:3, :3] @ turn[:3, :3].T, np.eye(3), atol=1e-15) and turn[3].tolist() == [0, 0, 0, 1]
    v, _ = K.case("cube")
    centre = (v.min(axis=0).astype(np.float64) + v.max(axis=0)) / 2
    assert np.allclose(turn[:3, :3] @ centre + turn[:3, 3], centre + [0, 0, 1.5], atol=1e-12)      # the centre only moves along the axis
    assert np.array_equal(M.orbit_transform(*K.case("bad"), 0, 0, 0, consts=R.make_consts(24, 32)), np.eye(4))
    assert M.transform_normals(n, np.eye(4)) is not None and np.array_equal(M.transform_normals(n, np.eye(4)), n)
    scale = np.diag([2.0, 1.0, 0.5, 1.0])
    got = M.transform_normals(n, scale)
    assert np.array_equal(got.view(np.uint32), O.transform_normals(n, scale).view(np.uint32)) and not np.array_equal(got, n)
    flat = np.diag([1.0, 1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="singular"):
        M.transform_normals(n, flat)
    assert np.array_equal(M.ssaa_consts(R.make_consts(13, 19), 3), O.ssaa_consts(R.make_consts(13, 19), 3))


# ---- the two writers, built with g++ ---------------------------------------------------------------------------------------------
WRITER_MAIN = r"""
// argv: verts.bin normals.bin nv faces.bin nf img.bin H W out_dir  ->  the codes of six calls, one per line
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>
#include "svr_hip.h"

template <class T>
static std::vector<T> slurp(const char *path, size_t n) {
  std::vector<T> v(n);
  FILE *f = std::fopen(path, "rb");
  if (!f || (n && std::fread(v.data(), sizeof(T), n, f) != n)) std::exit(9);
  std::fclose(f);
  return v;
}

int main(int argc, char **argv) {
  if (argc != 10) return 2;
  const long nv = std::atol(argv[3]), nf = std::atol(argv[5]);
  const int H = std::atoi(argv[7]), W = std::atoi(argv[8]);
  const auto verts = slurp<float>(argv[1], nv * 3), normals = slurp<float>(argv[2], nv * 3);
  const auto faces = slurp<int32_t>(argv[4], nf * 3);
  const auto img = slurp<uint8_t>(argv[6], (size_t)H * W * 3);
  const std::string dir = argv[9];
  std::printf("%d\n", svr_write_obj_normals((dir + "/mesh.obj").c_str(), verts.data(), normals.data(), nv, faces.data(), nf));
  std::printf("%d\n", svr_write_obj_normals((dir + "/empty.obj").c_str(), nullptr, nullptr, 0, nullptr, 0));
  std::printf("%d\n", svr_write_obj_normals((dir + "/missing/mesh.obj").c_str(), verts.data(), normals.data(), nv, faces.data(), nf));
  std::printf("%d\n", svr_write_obj_normals((dir + "/null.obj").c_str(), verts.data(), nullptr, nv, faces.data(), nf));
  std::printf("%d\n", svr_write_png_rgb8((dir + "/img.png").c_str(), img.data(), H, W));
  std::printf("%d\n", svr_write_png_rgb8((dir + "/missing/img.png").c_str(), img.data(), H, W));
  std::printf("%d\n", svr_write_png_rgb8((dir + "/zero.png").c_str(), img.data(), 0, W));
  std::printf("%d\n", svr_write_png_rgb8((dir + "/null.png").c_str(), nullptr, H, W));
  std::printf("%s\n", svr_last_error());
  return 0;
}
"""


def _parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        p = line.split()
        if p[0] == "v":
            v.append([float(x) for x in p[1:]])
        elif p[0] == "vn":
            vn.append([float(x) for x in p[1:]])
        elif p[0] == "f":
            f.append([tuple(int(x) for x in c.split("//")) for c in p[1:]])
    return np.array(v, dtype=np.float64).reshape(-1, 3), np.array(vn, dtype=np.float64).reshape(-1, 3), f


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_png_rgb_and_obj_normals_writers(tmp_path, variant):
    """svr_write_png_rgb8 and svr_write_obj_normals built with g++ into a program of their own (plain everywhere, under the host
    sanitizers on machines without a GPU): the PNG reads back equal through PIL, the OBJ parses back to the float32 bits, an
    unwritable path is SVR_E_IO (-5), and the shipped library writes the same bytes."""
    from PIL import Image
    if variant == "sanitized":
        _no_gpu_or_skip()
    rng = np.random.default_rng(12)
    verts = rng.standard_normal((301, 3)).astype(np.float32)
    verts.reshape(-1).view(np.uint32)[:4] = [0x80000000, 0x00000001, 0x7f7fffff, 0x3f800001]
    normals = rng.standard_normal((301, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True).astype(np.float32)
    normals[5] = 0
    faces = rng.integers(0, 301, (517, 3)).astype(np.int32)
    img = rng.integers(0, 256, (33, 20, 3)).astype(np.uint8)
    for name, a in (("verts", verts), ("normals", normals), ("faces", faces), ("img", img)):
        a.tofile(tmp_path / (name + ".bin"))
    (tmp_path / "main.cpp").write_text(WRITER_MAIN)
    exe = tmp_path / "writers"
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + (SANITIZE if variant == "sanitized" else []) + ["-I", os.path.join(REPO, "include"), "-I", CSRC]
    cmd += [os.path.join(CSRC, n) for n in ("io_mesh.cpp", "io_png.cpp", "capi.cpp")] + [str(tmp_path / "main.cpp"), "-lz", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([str(exe), str(tmp_path / "verts.bin"), str(tmp_path / "normals.bin"), "301", str(tmp_path / "faces.bin"), "517",
                        str(tmp_path / "img.bin"), "33", "20", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert [int(x) for x in lines[:8]] == [0, 0, -5, -1, 0, -5, -2, -1], lines
    with Image.open(out / "img.png") as im:
        assert im.mode == "RGB" and im.size == (20, 33) and np.array_equal(np.array(im), img)
    v, vn, f = _parse_obj(out / "mesh.obj")
    assert np.array_equal(v.astype(np.float32).view(np.uint32), verts.view(np.uint32))
    assert np.array_equal(vn.astype(np.float32).view(np.uint32), normals.view(np.uint32))
    assert f == [[(int(i) + 1, int(i) + 1) for i in row] for row in faces]
    text = (out / "mesh.obj").read_text().splitlines()
    assert [l.split()[0] for l in text] == ["v"] * 301 + ["vn"] * 301 + ["f"] * 517 and (out / "empty.obj").read_bytes() == b""
    # the shipped library: the same bytes, and its plain writers unchanged by the shared code
    import __graft_entry__ as ge
    ge.build()
    import svr_amd  # noqa: F401
    from svr_amd.util import visualize as VZ
    VZ.export_obj(verts, faces, tmp_path / "lib.obj", normals=normals)
    VZ.save_png(img, tmp_path / "lib.png")
    assert (tmp_path / "lib.obj").read_bytes() == (out / "mesh.obj").read_bytes()
    assert (tmp_path / "lib.png").read_bytes() == (out / "img.png").read_bytes()
    VZ.export_obj(verts, faces, tmp_path / "plain.obj")
    plain = (tmp_path / "plain.obj").read_text().splitlines()
    assert plain[:301] == text[:301] and plain[301:] == ["f " + " ".join(str(int(i) + 1) for i in row) for row in faces]
    with pytest.raises(RuntimeError, match="rc=-5"):
        VZ.save_png(img, tmp_path / "missing" / "x.png")
    with pytest.raises(ValueError, match="300 normals for 301"):
        VZ.export_obj(verts, faces, tmp_path / "x.obj", normals=normals[:300])
