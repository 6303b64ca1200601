"""CPU: the fused point-MLP tail's host side (csrc/mlp_tail.hip, csrc/mlp_tail_layout.h).  The workspace size the library
reports equals what the layout function walks (stand-alone driver, g++, once plain and once with sanitizers); the entry
point's argument checks run in front of anything it enqueues, so they answer without a device; the binding's routing rule
(ops._mlp_tail_op) is host only."""
import ctypes as C
import os
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "single-view-3d-reconstruction_amd", "csrc")
DRIVER = os.path.join(REPO, "tests", "host", "mlp_tail_layout_driver.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
OK, BADARG, UNSUPPORTED = 0, -1, -4


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import svr_amd
    return svr_amd._lib.lib()


@pytest.mark.parametrize("variant", ["plain", "sanitized"])
def test_size_query_equals_what_the_layout_walks(tmp_path, variant):
    if variant == "sanitized" and torch.cuda.is_available():
        pytest.skip("sanitizer builds run on the CPU machine only")
    exe = tmp_path / ("mlp_tail_layout_driver_" + variant)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if variant == "sanitized" else [])
    r = subprocess.run(cmd + ["-I", CSRC, DRIVER, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    word, nbytes, carved = r.stdout.split()
    assert word == "ok" and int(carved) == 5
    # two amax lines, two plane pairs of 256 x 256 halves, the cursor's base slack
    assert int(nbytes) == 2 * 256 + 2 * (2 * 256 * 256 * 2) + 256
    assert _lib().svr_mlp_tail_fwd_workspace(256) == int(nbytes)


def test_unsupported_widths_are_refused_by_size_query_and_entry_point():
    l = _lib()
    z = C.c_void_p(0)
    host = (C.c_char * 64)()
    for hidden in (0, 128, 255, 512):
        assert l.svr_mlp_tail_fwd_workspace(hidden) == UNSUPPORTED
        assert l.svr_mlp_tail_fwd(z, 0, C.addressof(host), z, C.addressof(host), z, z, z, z, 0, z, 0, z, z, 0, hidden,
                                  C.addressof(host), z) == UNSUPPORTED
        assert b"hidden" in l.svr_last_error()


def test_prepare_only_call_is_accepted_without_a_device():
    """h0 == NULL: only W1, W2 and the workspace are looked at.  The argument checks come first: what they refuse is refused
    without a device; a call they accept goes on to the launches -- on a machine with a GPU it prepares a real workspace and
    returns 0, without one the runtime's own (positive) launch error is all that is left to come back."""
    l = _lib()
    z = C.c_void_p(0)
    host = (C.c_char * 64)()
    a = C.addressof(host)
    assert l.svr_mlp_tail_fwd(z, 0, z, z, z, z, z, z, z, 0, z, 0, z, z, 0, 256, a, z) == BADARG      # neither h0 nor W1
    assert l.svr_mlp_tail_fwd(z, 0, a, z, z, z, z, z, z, 0, z, 0, z, z, 0, 256, a, z) == BADARG      # W1 without W2
    assert l.svr_mlp_tail_fwd(z, 0, a, z, a, z, z, z, z, 0, z, 0, z, z, 0, 256, z, z) == BADARG      # no workspace
    if torch.cuda.is_available():
        w1, w2 = torch.randn(256, 256, device="cuda"), torch.randn(256, 256, device="cuda")
        ws = torch.empty(l.svr_mlp_tail_fwd_workspace(256), device="cuda", dtype=torch.uint8)
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = l.svr_mlp_tail_fwd(z, 0, p(w1), z, p(w2), z, z, z, z, 0, z, 0, z, z, 0, 256, p(ws), z)
        torch.cuda.synchronize()
        assert rc == OK
    else:
        ws = (C.c_char * l.svr_mlp_tail_fwd_workspace(256))()
        w = (C.c_float * (256 * 256))()
        rc = l.svr_mlp_tail_fwd(z, 0, C.addressof(w), z, C.addressof(w), z, z, z, z, 0, z, 0, z, z, 0, 256, C.addressof(ws), z)
        assert rc >= 0, l.svr_last_error()      # not one of the SVR_E_* argument refusals


def test_routing_rule_picks_the_fused_tail_only_where_it_applies(monkeypatch):
    import svr_amd  # noqa: F401
    from svr_amd import ops
    w = torch.zeros(256, 256)
    wo = torch.zeros(256)
    pick = lambda **k: ops._mlp_tail_op(k.get("mode"), k.get("hidden", 256), k.get("w1", w), k.get("w2", w), k.get("wo", wo),
                                        k.get("h0", (256, 0, True)))
    assert pick() == "mlp_tail_f16x3" and pick(h0=(320, 0, True)) == "mlp_tail_f16x3" and pick(h0=None, wo=None) == "mlp_tail_f16x3"
    assert pick(mode="bf16x6") == "three_ops" and pick(mode="f32") == "three_ops"
    assert pick(hidden=128, w1=torch.zeros(128, 128), w2=torch.zeros(128, 128)) == "three_ops"
    assert pick(h0=(258, 0, True)) == "three_ops" and pick(h0=(256, 4, True)) == "three_ops" and pick(h0=(256, 0, False)) == "three_ops"
    assert pick(w1=torch.zeros(256, 512)[:, :256]) == "three_ops" and pick(w2=torch.zeros(128, 256)) == "three_ops"
    monkeypatch.setattr(ops, "FORWARD_GEMM", "bf16x6")
    assert pick() == "three_ops"
