"""CPU: the numpy oracle of the mesh evaluation (tests/eval_oracle.py) against the reference's eval_pointcloud
(tests/golden/eval_pointcloud.npz, made by tools/gen_golden_eval.py: the reference's util/evaluate.py with a
scipy cKDTree standing in for pykdtree -- the golden pins the aggregation and exact nearest neighbours, not pykdtree's
rounding), and the parts of the C ABI that work without a GPU: the host face table bit for bit, the argument checks of
every new entry point, and the Python surface refusing CPU tensors."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import eval_oracle as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = 2e-6     # ~2^-23 on each distance from the float32 rule plus the final sqrt; the rest is headroom for the
#                float32 normalisation of the normals in the reference


def golden():
    return np.load(os.path.join(GOLD, "eval_pointcloud.npz"), allow_pickle=False)


def ref_dict(z):
    return {k: float(z["ref_" + k.replace(" ", "_")]) for k in E.KEYS}


def assert_dict_close(got, want, rel=REL):
    assert set(got) == set(E.KEYS)
    for k in E.KEYS:
        if np.isnan(want[k]):
            assert np.isnan(got[k]), k
        else:
            assert abs(got[k] - want[k]) <= rel * abs(want[k]), (k, got[k], want[k])


def test_oracle_reproduces_the_reference_dictionary_and_indices():
    z = golden()
    assert z["pred"].dtype == np.float32 and z["pred"].shape == (8192, 3) and z["gt"].shape == (8192, 3)
    assert float(z["min_relative_gap"]) > 1e-5          # what makes index equality a fair demand on every point
    assert "stand-in" in str(z["note"])
    a_dist, _, a_idx = E.distance_p2p(z["pred"], z["gt"], None, None)
    c_dist, _, c_idx = E.distance_p2p(z["gt"], z["pred"], None, None)
    assert np.array_equal(a_idx, z["accuracy_idx"]) and np.array_equal(c_idx, z["completeness_idx"])
    for d, ref in ((a_dist, z["accuracy_dist"]), (c_dist, z["completeness_dist"])):
        assert np.all(np.abs(d.astype(np.float64) - ref) <= REL * ref)
    want = ref_dict(z)
    got = E.eval_pointcloud(z["pred"], z["gt"], z["normals_pred"], z["normals_gt"])
    assert_dict_close(got, want)
    assert np.isnan(want["iou"]) and 0.0 < want["normals"] < 1.0 and want["chamfer_l2"] > 0.0
    no_normals = E.eval_pointcloud(z["pred"], z["gt"])
    assert np.isnan(no_normals["normals"]) and no_normals["chamfer_l2"] == got["chamfer_l2"]


def test_oracle_nn_rules_ties_nan_and_inf():
    t = np.array([[1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 1, 0], [-1, 0, 0]], dtype=np.float32)
    q = np.array([[0, 0, 0], [0, 0.9, 0], [np.nan, 0, 0], [3e38, 0, 0]], dtype=np.float32)
    d, i = E.nn_search(q, t)
    assert i.tolist() == [0, 1, -1, 0]                  # tie -> lowest index; NaN target never returned; NaN query: none
    assert d[0] == 1.0 and np.isnan(d[2]) and d[3] == np.inf      # +inf is a number: it beats the NaN


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _face_table(v, f):
    import svr_amd
    v = np.ascontiguousarray(v, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.int32)
    normals = np.full((len(f), 3), np.nan)
    cum = np.full(len(f), np.nan)
    rc = svr_amd._lib.lib().svr_mesh_face_table(_vp(v), len(v), _vp(f), len(f), _vp(normals), _vp(cum))
    return rc, normals, cum


@pytest.mark.parametrize("tag", ["sphere", "torus", "openbox"])
def test_face_table_equals_oracle_bit_for_bit_on_golden_meshes(tag):
    z = np.load(os.path.join(GOLD, f"mesh_{tag}.npz"), allow_pickle=False)
    rc, normals, cum = _face_table(z["vertices"], z["faces"])
    on, oc = E.face_table(z["vertices"], z["faces"])
    assert rc == 0 and np.array_equal(normals, on) and np.array_equal(cum, oc)
    assert cum[-1] > 0 and np.all(np.diff(cum) >= 0)
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-15)


def test_face_table_zero_area_and_duplicate_faces():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(40, 3))
    v[7] = v[3]                                                                   # a repeated vertex
    f = rng.integers(0, 40, size=(200, 3)).astype(np.int32)
    f[10] = [5, 5, 9]                                                             # repeated index
    f[11] = [3, 7, 12]                                                            # coincident vertices
    f[12] = f[13] = f[50] = [1, 2, 30]                                            # duplicates
    v[20], v[21], v[22] = [0, 0, 0], [1, 2, 3], [2, 4, 6]
    f[14] = [20, 21, 22]                                                          # collinear, exactly
    f[0] = [4, 4, 4]
    f[-1] = [6, 6, 8]                                                             # the last face has no area
    rc, normals, cum = _face_table(v, f)
    on, oc = E.face_table(v, f)
    assert rc == 0 and np.array_equal(normals, on) and np.array_equal(cum, oc)
    for j in (0, 10, 11, 14, 199):
        assert not normals[j].any() and cum[j] == (cum[j - 1] if j else 0.0)
    assert np.array_equal(normals[12], normals[13]) and cum[13] - cum[12] > 0
    # the oracle sampler never picks them, not even with u0 at the ends of [0, 1]
    u = np.concatenate([rng.random((5000, 3)), [[0.0, 0.3, 0.3], [np.nextafter(1.0, 0.0), 0.9, 0.9], [1.0, 0.5, 0.5]]])
    _, face = E.sample(v, f, oc, u)
    area = np.diff(np.concatenate([[0.0], oc]))
    assert np.all(area[face] > 0) and face[-1] == np.nonzero(area > 0)[0][-1]


def test_new_entry_points_check_arguments_without_a_gpu():
    import svr_amd
    l = svr_amd._lib.lib()
    z = C.c_void_p(0)
    buf = np.zeros(64, dtype=np.float64)
    p = _vp(buf)
    BADARG, BADSHAPE = -1, -2
    # face table: nulls, counts, a face index out of range
    f = np.array([[0, 1, 2]], dtype=np.int32)
    assert l.svr_mesh_face_table(z, 3, _vp(f), 1, p, p) == BADARG and l.svr_mesh_face_table(p, 3, z, 1, p, p) == BADARG
    assert l.svr_mesh_face_table(p, 3, _vp(f), 1, z, p) == BADARG and l.svr_mesh_face_table(p, 3, _vp(f), 1, p, z) == BADARG
    assert l.svr_mesh_face_table(p, 3, _vp(f), 0, p, p) == BADARG and l.svr_mesh_face_table(p, 3, _vp(f), -1, p, p) == BADARG
    assert l.svr_mesh_face_table(p, 2, _vp(f), 1, p, p) == BADARG and l.svr_mesh_face_table(p, 0, _vp(f), 1, p, p) == BADARG
    assert b"face" in l.svr_last_error()
    # nearest neighbour: T == 0 and T >= 2^31 are shape errors, Q == 0 is a no-op, the rest are bad arguments
    assert l.svr_nn_search(p, 5, p, 0, p, p, p, 40, z) == BADSHAPE and l.svr_nn_search(p, 5, p, 1 << 31, p, p, p, 40, z) == BADSHAPE
    assert l.svr_nn_search(p, 5, p, -3, p, p, p, 40, z) == BADSHAPE
    assert l.svr_nn_search(p, -1, p, 4, p, p, p, 40, z) == BADARG
    assert l.svr_nn_search(z, 0, z, 4, z, z, z, 0, z) == 0
    for hole in range(5):
        args = [p, p, p, p, p]
        args[hole] = z
        assert l.svr_nn_search(args[0], 5, args[1], 4, args[2], args[3], args[4], 40, z) == BADARG, hole
    assert l.svr_nn_search(p, 5, p, 4, p, p, p, 39, z) == BADARG                  # workspace one byte short
    assert l.svr_nn_search_workspace(5) == 40 and l.svr_nn_search_workspace(0) == 0 and l.svr_nn_search_workspace(-1) == BADARG
    # sampler
    assert l.svr_mesh_sample(p, p, 0, p, 4, p, p, z) == BADARG and l.svr_mesh_sample(p, p, 1 << 31, p, 4, p, p, z) == BADARG
    assert l.svr_mesh_sample(p, p, 3, p, -1, p, p, z) == BADARG and l.svr_mesh_sample(z, z, 3, z, 0, z, z, z) == 0
    assert l.svr_mesh_sample(z, p, 3, p, 4, p, p, z) == BADARG and l.svr_mesh_sample(p, p, 3, p, 4, p, z, z) == BADARG
    # epilogue and reductions
    assert l.svr_nn_normals_dot(p, p, 0, p, -1, 4, p, z) == BADARG and l.svr_nn_normals_dot(p, p, 0, p, 4, 0, p, z) == BADARG
    assert l.svr_nn_normals_dot(z, p, 0, p, 4, 4, p, z) == BADARG and l.svr_nn_normals_dot(z, z, 0, z, 0, 4, z, z) == 0
    ws = svr_amd._lib.EVAL_SUMS_WORKSPACE_BYTES
    assert l.svr_eval_sums(z, z, 4, p, p, ws, z) == BADARG and l.svr_eval_sums(p, z, -1, p, p, ws, z) == BADARG
    assert l.svr_eval_sums(p, z, 4, z, p, ws, z) == BADARG and l.svr_eval_sums(p, z, 4, p, p, ws - 1, z) == BADARG
    assert l.svr_iou_counts(z, p, 4, p, z) == BADARG and l.svr_iou_counts(p, p, 4, z, z) == BADARG
    assert l.svr_iou_counts(p, p, -1, p, z) == BADARG


def test_header_constant_matches_binding():
    import re
    import svr_amd
    txt = open(os.path.join(os.path.dirname(GOLD), "..", "include", "svr_hip.h")).read()
    assert int(re.search(r"#define SVR_EVAL_SUMS_WORKSPACE_BYTES (\d+)", txt).group(1)) == svr_amd._lib.EVAL_SUMS_WORKSPACE_BYTES


def test_evaluate_imports_and_refuses_cpu_tensors():
    import svr_amd  # noqa: F401
    from svr_amd.util import distance_p2p, eval_mesh, eval_pointcloud, sample_surface  # noqa: F401
    from svr_amd.util import evaluate
    from svr_amd.data_processing.mesh_occupancies import sample_points  # noqa: F401
    assert evaluate.KEYS == E.KEYS
    a = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        distance_p2p(a, a, None, None)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        eval_pointcloud(a, a)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        evaluate.sample_with_uniforms(None, torch.zeros(4, 3, dtype=torch.float64))


def test_evaluate_runs_as_a_module_and_writes_the_result_file(tmp_path):
    """`python -m svr_amd.util.evaluate` (the reference's __main__ loop): argument parsing and the result-file format, on
    empty lists -- no mesh, so no GPU work."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / "pf").mkdir()
    (tmp_path / "pf" / "exp.txt").write_text("")
    (tmp_path / "pf" / "normed_gt.txt").write_text("")
    env = dict(os.environ, PYTHONPATH=repo + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "svr_amd.util.evaluate", "--path_files", "pf", "--experiment", "exp.txt"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = (tmp_path / "results" / "exp_exp.txt").read_text().splitlines()
    assert lines[0] == "0 meshes" and lines[1] == "mean completeness: nan" and lines[10] == "" and lines[11] == "completeness: []"
    assert [l.split(":")[0] for l in lines[11:]] == list(E.KEYS)
