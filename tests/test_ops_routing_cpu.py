"""CPU: SVR_BACKWARD is read once and validated when svr_amd.ops is imported (a typo used to mean exact f32 everywhere)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import_ops(backward):
    env = dict(os.environ)
    env.pop("SVR_BACKWARD", None)
    if backward is not None:
        env["SVR_BACKWARD"] = backward
    return subprocess.run([sys.executable, "-c", "import svr_amd.ops as o; print(o.BACKWARD_GEMM, o.BACKWARD_CONV, o.BACKWARD_CONV_WEIGHT)"],
                          cwd=REPO, env=env, capture_output=True, text=True)


def test_svr_backward_is_validated_at_import():
    bad = _import_ops("bf16")
    assert bad.returncode != 0 and "SVR_BACKWARD" in bad.stderr and "ValueError" in bad.stderr
    for good in ("bf16x3", "f16x3s", "f32"):
        r = _import_ops(good)
        assert r.returncode == 0 and r.stdout.split() == [good] * 3
    assert _import_ops(None).stdout.split() == ["f16x3s"] * 3
