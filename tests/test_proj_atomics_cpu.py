"""CPU: tools/proj_atomics.py, the numpy model of the atomic projected scatter's run logic, on the benched level-4 shape
(16^3, 50 000 uniform points, one sample): the (cell, j) order costs what DESIGN.md quotes for the kernel, and the x-block
order with the face hand-over removes about a third of it (without a hand-over the ratio would be 1.0)."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("proj_atomics", os.path.join(REPO, "tools", "proj_atomics.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_block_order_removes_a_third_of_the_level4_atomics():
    pa = _tool()
    pts = pa.make_points("uniform", 1, 50000, 0)
    k1 = pa.count(pts, (16, 16, 16), False, 0.0722, 1)
    k4 = pa.count(pts, (16, 16, 16), False, 0.0722, 4)
    print(k1, k4)
    assert k1["handed"] == 0
    assert abs(k1["atomic_bytes"] / 1e9 - 0.238) < 0.03 * 0.238        # 1.9 GB per step at batch 8
    ratio = k4["atomic_bytes"] / k1["atomic_bytes"]
    assert 0.60 < ratio < 0.70, ratio
