"""CPU: the C-ABI library builds, loads, and exports every symbol include/svr_hip.h declares
(no compute calls without a GPU); host-side layout logic."""
import ctypes
import os
import re

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(REPO, "include", "svr_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(svr_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge.build()
    import svr_amd
    lib = ctypes.CDLL(svr_amd._lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/svr_hip.h but not exported"
    bound = set(svr_amd._lib.SIGNATURES)
    assert bound == set(names), bound ^ set(names)
    l = svr_amd._lib.lib()
    assert l.svr_version() >= 100
    assert l.svr_linear_bwd_weight_workspace(1000, 256, 2592) > 0


def test_feature_layout_is_a_permutation_of_the_reference_rows():
    import svr_amd  # noqa: F401
    from svr_amd.ops import FeatureLayout
    for chans in ([1, 16, 32, 64, 128, 128], [1, 64, 128, 128]):
        lay = FeatureLayout(chans)
        perm = lay.reference_permutation()
        used = perm[perm >= 0]
        assert lay.row_stride % 32 == 0 and lay.width == 7 * sum(chans)
        assert sorted(used.tolist()) == list(range(7 * sum(chans)))
        assert all(c % 16 == 0 for l, c in enumerate(lay.col) if chans[l] >= 4)


def test_module_state_dict_matches_reference_names():
    import svr_amd  # noqa: F401
    from svr_amd.model import IFNet
    from oracle import ifnet_oracle as O
    for res in (128, 32):
        m = IFNet(net_res=res)
        keys = {k for k in m.state_dict() if "num_batches" not in k}
        assert keys == set(O.param_shapes(res)), keys ^ set(O.param_shapes(res))
        for k, shp in O.param_shapes(res).items():
            assert tuple(m.state_dict()[k].shape) == tuple(shp), k
    assert sum(p.numel() for p in IFNet().parameters()) == 2550881
    assert sum(p.numel() for p in IFNet(net_res=32).parameters()) == 2954049


def test_hip_path_refuses_cpu_tensors():
    import pytest
    import svr_amd  # noqa: F401
    from svr_amd.model import IFNet
    with pytest.raises(RuntimeError):
        IFNet()(torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 4, 3))


def _doc_stub_namespace():
    """Execute the ctypes struct definitions of INTEGRATION.md section 3 (the stub a maintainer would paste)."""
    txt = open(os.path.join(REPO, "INTEGRATION.md")).read()
    block = re.search(r"```python\nimport ctypes as C, torch\n(.*?)```", txt, flags=re.S).group(1)
    structs = block.split("lib.svr_gather_trilinear_fwd.restype")[0]
    structs = "\n".join(l for l in structs.splitlines() if not l.startswith("lib = "))
    ns = {"C": ctypes}
    exec(structs, ns)                                   # our own documentation, not reference code
    return ns


def test_header_structs_binding_and_doc_stub_cannot_drift(tmp_path):
    """include/svr_hip.h is compiled on its own (plain C, gcc) and its sizeof / offsetof of svr_level and
    svr_gather_desc are compared with (a) the ctypes mirrors in _lib.py, (b) the struct sizes the library itself
    reports (svr_sizeof_*), (c) the stub documented in INTEGRATION.md -- a field added to one of them fails here,
    on the CPU, instead of as a wild device read on the GPU."""
    import subprocess
    import svr_amd
    L, Gd = svr_amd._lib.Level, svr_amd._lib.GatherDesc
    src = tmp_path / "layout.c"
    lf = [n for n, _ in L._fields_]
    gf = [n for n, _ in Gd._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "svr_hip.h"', 'int main(void) {',
             '  printf("svr_level %zu\\n", sizeof(svr_level));', '  printf("svr_gather_desc %zu\\n", sizeof(svr_gather_desc));']
    lines += [f'  printf("svr_level.{f} %zu\\n", offsetof(svr_level, {f}));' for f in lf]
    lines += [f'  printf("svr_gather_desc.{f} %zu\\n", offsetof(svr_gather_desc, {f}));' for f in gf]
    lines += ['  printf("SVR_MAX_LEVELS %d\\n", SVR_MAX_LEVELS);', '  return 0;', '}']
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    out = {k: int(v) for k, v in out.items()}
    assert out["SVR_MAX_LEVELS"] == svr_amd._lib.SVR_MAX_LEVELS
    assert out["svr_level"] == ctypes.sizeof(L) and out["svr_gather_desc"] == ctypes.sizeof(Gd)
    for f in lf:
        assert out[f"svr_level.{f}"] == getattr(L, f).offset, f
    for f in gf:
        assert out[f"svr_gather_desc.{f}"] == getattr(Gd, f).offset, f
    lib = svr_amd._lib.lib()
    assert lib.svr_sizeof_level() == out["svr_level"] and lib.svr_sizeof_gather_desc() == out["svr_gather_desc"]
    # the documented stub
    ns = _doc_stub_namespace()
    for name, mirror in (("Level", L), ("GatherDesc", Gd)):
        doc = ns[name]
        assert ctypes.sizeof(doc) == ctypes.sizeof(mirror), name
        assert [(n, getattr(doc, n).offset) for n, _ in doc._fields_] == \
               [(n, getattr(mirror, n).offset) for n, _ in mirror._fields_], name


def test_hand_written_kernels_do_not_spill():
    """Register report of the gfx950 build (hipcc -Rpass-analysis=kernel-resource-usage, kept per object file by build.py):
    no hand-written kernel may use scratch memory, except the two listed ones at their known sizes.  A source change that
    makes the register allocator spill shows up as a multiple of the kernel time on the GPU only (the fused gather -> fc_0
    kernel: 260 B / lane of scratch = 11.7 instead of 2.6 ms) -- this catches it where the code is compiled."""
    import importlib
    import __graft_entry__ as ge
    ge.build()
    b = importlib.import_module("single-view-3d-reconstruction_amd.build")
    usage = b.resource_usage()
    if not usage:                    # objects built before the report existed: rebuild once
        b.build(force=True)
        usage = b.resource_usage()
    own = {k: v for k, v in usage.items() if "rocprim" not in k and "hipcub" not in k}
    assert len(own) > 100 and any("gather_fc0_kernel" in k for k in own)
    known = {"linear_nt_h3_kernelILi64ELi0ELi2": 32, "conv3d_bwd_weight_x3_kernel": 16}
    bad = {}
    for k, v in own.items():
        limit = max([lim for name, lim in known.items() if name in k], default=0)
        if v.get("scratch", 0) > limit:
            bad[k] = v
    assert not bad, bad
    fc0 = [v for k, v in own.items() if "gather_fc0_kernel" in k][0]
    assert fc0["scratch"] == 0 and fc0["vgprs"] <= 128 and fc0["occupancy"] >= 4, fc0


def test_module_copies_and_pickles_after_a_step_left_scratch_state():
    """a training step leaves a torch.cuda.Event in ext._prepared.ready and GBs in ext._arena; the reference
    nn.Module can be deep-copied / pickled, so this one must be too -- the copy gets fresh, empty scratch state."""
    import copy
    import io
    import pickle

    import torch
    from svr_amd.arena import StepArena
    from svr_amd.model import IFNet
    m = IFNet(net_res=128)
    ext = m.ifnet_feature_extractor
    ext._prepared.ready = torch.cuda.Event()          # what _prepare_weights_async leaves behind
    ext._points_ready = torch.cuda.Event()
    ext._arena._bufs["x"] = torch.zeros(4)
    for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        e2 = clone.ifnet_feature_extractor
        assert isinstance(e2._arena, StepArena) and e2._arena is not ext._arena and e2._arena.nbytes() == 0
        assert e2._prepared is not ext._prepared and e2._prepared.ready is None
        # _stages / _param_list of the copy point at the copy's own modules
        assert e2._stages[0][0][0] is e2.conv_in and e2._param_list[0] is e2.conv_in.weight
        assert e2._param_list[0] is not ext._param_list[0]
        for (k, a), (k2, b) in zip(m.state_dict().items(), clone.state_dict().items()):
            assert k == k2 and torch.equal(a, b)
    buf = io.BytesIO()
    torch.save(m, buf)
    ext.release_step_buffers()
    assert ext._arena.nbytes() == 0


def _conv_variants(shapes, persistent_env=None):
    """svr_conv3d_k3_variant for [(op, B, dims, Ci, Co)] in a child process (persistent_bricks() reads SVR_CONV_PERSISTENT once
    per process): the variant tags of tests/_conv_cases.py, workgroup rows and svr_conv3d_fwd_f16x3_stats_blocks."""
    import json
    import subprocess
    import sys
    code = ("import json, sys; sys.path.insert(0, sys.argv[1]); import svr_amd; from svr_amd import ops, _lib; "
            "from tests import _conv_cases as K; out = []\n"
            "for op, B, dims, Ci, Co in json.loads(sys.argv[2]):\n"
            "    v = ops.conv3d_k3_variant(op, B, tuple(dims), Ci, Co)\n"
            "    out.append([K.tag(v), v['workgroup_rows'], _lib.lib().svr_conv3d_fwd_f16x3_stats_blocks(B, *dims, Ci, Co)])\n"
            "print('VARIANTS ' + json.dumps(out))")
    env = {k: v for k, v in os.environ.items() if k != "SVR_CONV_PERSISTENT"}
    if persistent_env is not None:
        env["SVR_CONV_PERSISTENT"] = persistent_env
    r = subprocess.run([sys.executable, "-c", code, REPO, json.dumps(shapes)], env=env, cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("VARIANTS ")][-1]
    return json.loads(line[len("VARIANTS "):])


def test_conv3d_variant_table_and_every_instantiation_is_reached():
    """Which kernel of csrc/conv3d_bf16.hip a shape runs, asked of the library (svr_conv3d_k3_variant: the function the
    launchers themselves call), for the encoder's layers at batch 8 and for every case of tests/test_gpu_conv_paths.py; and the
    cases of that file, together, reach EVERY instantiation the three launchers can produce.  A case edit that drops a variant
    fails here, without a GPU."""
    import __graft_entry__ as ge
    ge.build()
    from tests import _conv_cases as K
    exp = K.expected()
    got = _conv_variants([(op, B, dims, Ci, Co) for _, op, B, dims, Ci, Co, _ in exp])
    for (name, op, B, dims, Ci, Co, tag), (gtag, rows, blocks) in zip(exp, got):
        assert gtag == tag, (name, op, gtag, tag)
        # the 4 x 4 x 8 bricks of the volume, or its 8 x 4 x 8 double bricks on the two-slices-per-wave tiles
        bz = 8 if tag in ("P", "VT2") else 4
        assert rows == B * -(-dims[0] // bz) * -(-dims[1] // 4) * -(-dims[2] // 8), (name, op, rows)
        if op == "fwd_f16x3":
            assert blocks == rows, (name, blocks, rows)
    # the table of DESIGN.md section 4, spelled out once more: (forward, backward-data) of the real layers at batch 8
    table = {(64, 16, 32): ("P", "P"), (64, 32, 32): ("P", "P"), (32, 32, 64): ("CK32TN2", "P"), (32, 64, 64): ("CK32TN2", "CK32TN2"),
             (16, 64, 128): ("CK32TN2", "CK32TN1"), (16, 128, 128): ("CK32TN2", "CK32TN2"), (8, 128, 128): ("CK32TN1", "CK32TN1")}
    real = [K.by_name(n) for n in K.REAL]
    assert {(c[2][0], c[3], c[4]): (c[6], c[7]) for c in real} == table and all(c[1] == 8 and len(set(c[2])) == 1 for c in real)
    # the forward bf16x6 entry point: 16-channel chunks, tile width from Co alone (no 512 rule), never persistent
    x6 = _conv_variants([("fwd_bf16x6", 8, (n, n, n), Ci, Co) for n, Ci, Co in table])
    assert [t for t, _, _ in x6] == ["CK16TN1", "CK16TN1", "CK16TN2", "CK16TN2", "CK16TN4", "CK16TN4", "CK16TN4"]
    # SVR_CONV_PERSISTENT=0: every "P" becomes the one-brick form of the same tile, nothing else moves
    off = _conv_variants([(op, B, dims, Ci, Co) for _, op, B, dims, Ci, Co, _ in exp], persistent_env="0")
    assert [g[0] for g in off] == ["VT2" if e[-1] == "P" else e[-1] for e in exp]
    assert [g[1:] for g in off] == [g[1:] for g in got]
    reached = {(op, tag) for _, op, _, _, _, _, tag in exp}
    off_cases = {(op, "VT2") for n in K.NO_PERSISTENT for _, op, *_ in [e for e in exp if e[0] == n]}
    assert off_cases == {(op, "VT2") for op in K.FWD_OPS + K.BWD_OPS}, off_cases      # the child-process cases cover all three too
    assert reached >= K.ALL_VARIANTS, sorted(K.ALL_VARIANTS - reached)
    assert len(K.ALL_VARIANTS) == 3 * 8


def test_conv3d_variant_refuses_what_the_entry_points_refuse():
    import svr_amd  # noqa: F401
    from svr_amd import _lib
    l = _lib.lib()
    z = ctypes.c_void_p(0)
    q = lambda op, *a: l.svr_conv3d_k3_variant(op, *a, z, z, z, z, z)     # noqa: E731  (every output may be NULL)
    assert q(0, 2, 8, 8, 8, 16, 5) == 0 and q(3, 2, 8, 8, 8, 16, 5) == 0 and q(1, 2, 8, 8, 8, 6, 16) == 0
    assert q(0, 2, 8, 8, 8, 8, 32) == -4 and q(1, 2, 8, 8, 8, 16, 8) == -4 and q(2, 2, 8, 8, 8, 3, 16) == -4
    assert q(4, 2, 8, 8, 8, 16, 16) == -1 and q(-1, 2, 8, 8, 8, 16, 16) == -1 and q(0, 2, 0, 8, 8, 16, 16) == -2


def test_wgrad_variant_table_and_every_kernel_is_reached():
    """Which kernel a 3x3x3 weight-gradient entry point runs, asked of the library (svr_conv3d_k3_bwd_weight_variant: the
    function the launchers of csrc/conv3d.hip and csrc/conv3d_bwdw_bf16.hip themselves call), for every row of
    tests/_wgrad_cases.py; the rows, together, reach EVERY kernel the launchers can select, the 8-wave split kernel and the f32
    brick kernel each with one brick per workgroup and with several.  A change to x3_parts, bw_brick_parts, WS_MIN_BRICKS or the
    W <= 128 rule that moves a row onto another kernel fails here, without a GPU."""
    import __graft_entry__ as ge
    ge.build()
    from svr_amd import _lib, ops
    from tests import _wgrad_cases as WC
    assert len({c[0] for c in WC.CASES}) == len(WC.CASES)
    l = _lib.lib()
    z = ctypes.c_void_p(0)
    reached, per_seen = set(), set()
    for name, op, B, dims, Ci, Co, tag, per in WC.expected():
        if tag is None:      # refused by the entry point: the query returns its error code
            assert l.svr_conv3d_k3_bwd_weight_variant(ops.WGRAD_VARIANT_OPS[op], B, *dims, Ci, Co, z, z, z) == WC.UNSUPPORTED, (name, op)
            continue
        v = ops.conv3d_k3_bwd_weight_variant(op, B, dims, Ci, Co)
        assert v["kernel"] == tag, (name, op, v)
        reached.add((op, tag))
        nb, pairs = WC.bricks(B, dims), -(-Ci // 32) * -(-Co // 32)
        if tag in ("X3", "BRICK"):
            assert per in ("1", ">1") and (v["max_bricks_per_part"] == 1) == (per == "1"), (name, op, v)
            per_seen.add((tag, per))
        if tag == "BRICK":   # one brick per workgroup exactly when the volume has fewer bricks than the rule's 512 / pairs parts
            assert (v["max_bricks_per_part"] == 1) == (nb <= -(-512 // pairs)), (name, v, nb)
            assert v["parts"] == min(-(-512 // pairs), nb), (name, v)
        if tag in ("WS_PAIR", "WS", "X3"):
            assert v["parts"] == min(-(-256 // pairs), nb) and v["max_bricks_per_part"] == -(-nb // v["parts"]), (name, v)
            assert (tag == "X3") == (nb < 8 * v["parts"]) and (tag == "WS_PAIR") == (tag != "X3" and Ci <= 16), (name, v)
        if tag.startswith("C1"):
            assert v["max_bricks_per_part"] == 1 and v["parts"] >= 1, (name, v)
    assert reached == WC.ALL_VARIANTS, sorted(reached ^ WC.ALL_VARIANTS)
    assert per_seen == {(t, p) for t in ("X3", "BRICK") for p in ("1", ">1")}, per_seen
    assert len(WC.ALL_VARIANTS) == 4 + 2 * 3
    # what the entry points refuse, the query refuses with the same code; every output may be NULL
    q = lambda op, *a: l.svr_conv3d_k3_bwd_weight_variant(op, *a, z, z, z)     # noqa: E731
    assert q(0, 1, 8, 8, 8, 16, 32) == 0 and q(1, 1, 8, 8, 8, 16, 32) == 0 and q(2, 1, 8, 8, 8, 4, 4) == 0
    assert q(3, 1, 8, 8, 8, 16, 32) == -1 and q(-1, 1, 8, 8, 8, 16, 32) == -1
    assert q(0, 1, 0, 8, 8, 16, 32) == -2 and q(2, 1, 8, 8, 0, 16, 32) == -2
    assert q(0, 1, 8, 8, 8, 1, 48) == -4 and q(0, 1, 8, 8, 8, 6, 32) == -4 and q(1, 1, 8, 8, 8, 1, 16) == -4 and q(2, 1, 8, 8, 8, 16, 6) == -4
    assert q(1, 1, 256, 256, 257, 16, 16) == -4 and q(0, 1, 256, 256, 257, 16, 16) == 0      # over 2^24 voxels: the f32 kernel only


def test_linear_variant_table_and_every_launcher_branch_is_reached():
    """Which kernel, epilogue form and bias form a linear op runs, asked of the library (svr_linear_variant: the function the
    launchers of csrc/gemm*.hip themselves call) through ops.linear_variant, for every case of tests/test_gpu_gemm_paths.py;
    the cases, together, reach EVERY (entry point, kernel, epilogue form, bias form) the launchers can produce -- found by
    sweeping the query over shapes, leading dimensions and address bits, so a launcher branch that gains a variant fails here
    until a case names it -- and the split regimes of the weight gradient.  A case edit that drops a branch fails here,
    without a GPU."""
    import itertools
    import __graft_entry__ as ge
    ge.build()
    from svr_amd import ops
    from tests import _gemm_cases as GC
    assert len({c[0] for c in GC.CASES}) == len(GC.CASES)
    reached, splits = set(), {}
    for case in GC.CASES:
        name, kind = case[0], case[1]
        assert set(case[7]) == set(GC.modes(case)), name
        for mode in GC.modes(case):
            v = GC.query(ops, case, mode, want_bias=case[6].get("bias", (True,))[0])
            assert GC.tag(kind, v) == case[7][mode], (name, mode, v)
            for want_bias, masked in itertools.product(case[6].get("bias", (True, False)) if kind == "bwd_weight" else (True,),
                                                       (True, False) if kind == "bwd_data" else (True,)):
                v = GC.query(ops, case, mode, want_bias=want_bias, masked=masked)
                if v["status"] == 0:
                    reached.add((v["op"], v["kernel"], v["coalesced"], v["bias"]))
                    if v["kernel"] in ("tn_tr", "tn_prepass"):
                        splits[name] = (v["splits"], case[2] - (v["splits"] - 1) * v["rows_per_split"])      # (splits, rows of the last)
                else:
                    assert v["status"] in (-2, -3), (name, mode, v)
    assert reached == GC.ALL_VARIANTS, sorted(reached ^ GC.ALL_VARIANTS)
    assert splits["w_1x4x4"] == (1, 1) and splits["w_33x8x36"] == (2, 1), splits
    # more than 28 splits: the eight-deep walk of slab_reduce_x3_kernel AND its remainder loop (splits % 32 not in 0, 29..31)
    assert any(s > 28 and 0 < s % 32 <= 28 for s, _ in splits.values()), splits
    # everything the launchers can answer with, over a sweep of shapes / leading dimensions / address bits
    seen = set()
    for kind, modes in GC.MODES.items():
        for mode, M, N, K, pad, lo, flag in itertools.product(modes, (1, 33, 1100), (4, 16, 32, 48, 64, 72, 130, 256, 1792),
                                                              (4, 6, 16, 36, 64, 130), (0, 2, 4), (0, 4), (False, True)):
            cols = {"fwd": (K, K, N), "bwd_data": (N, K, K), "bwd_weight": (N, K, K)}[kind]
            for which in range(4):      # the operand that is padded / misaligned (3: the mask)
                lay = [(c + pad if i == which else c, lo if i == which else 0, True) for i, c in enumerate(cols)]
                mask = (K + pad if which == 3 else K, lo if which == 3 else 0, True) if kind == "bwd_data" and flag else None
                v = ops.linear_variant(kind, mode, M, N, K, a=lay[0], b=lay[1], out=lay[2], mask=mask, epilogue=2 if kind == "fwd" else None,
                                       want_bias=flag and kind == "bwd_weight")
                if v["status"] == 0:
                    seen.add((v["op"], v["kernel"], v["coalesced"], v["bias"]))
    assert seen == GC.ALL_VARIANTS, sorted(seen ^ GC.ALL_VARIANTS)


def test_linear_variant_refuses_what_the_entry_points_refuse():
    import svr_amd  # noqa: F401
    from svr_amd import _lib, ops
    l = _lib.lib()
    z = ctypes.c_void_p(0)
    st = ctypes.c_int32()

    def q(op, M, N, K, lds, los, epi=0):      # lds / los: (a, b, out, mask)
        rc = l.svr_linear_variant(op, M, N, K, *lds, *los, epi, 0, z, z, z, z, z, ctypes.byref(st))      # (every output may be NULL)
        return rc, st.value
    O = ops.LINEAR_OPS
    assert q(9, 8, 32, 32, (32,) * 4, (0,) * 4)[0] == -1 and q(-1, 8, 32, 32, (32,) * 4, (0,) * 4)[0] == -1
    assert q(O["fwd_f16x3"], 8, 32, 24, (24, 24, 32, 0), (0,) * 4) == (0, -2)               # K % 16
    assert q(O["fwd_f16x3"], 8, 32, 32, (32, 32, 32, 0), (4, 0, 0, 0)) == (0, -3)           # X misaligned
    assert q(O["fwd_f16x3"], 8, 32, 32, (32, 32, 33, 0), (0, 0, 4, 0)) == (0, 0)            # Y: any layout (per-lane epilogue)
    assert q(O["bwd_data_f32"], 8, 32, 30, (32, 30, 30, 0), (0,) * 4) == (0, -2)            # K % 4
    # the float4 epilogue of linear_nn_x3_kernel: dX and the mask must be 16-byte aligned, in both splits
    for op in ("bwd_data_bf16x3", "bwd_data_f16x3s"):
        assert q(O[op], 8, 32, 36, (32, 36, 40, 40), (0,) * 4, 3) == (0, 0), op
        assert q(O[op], 8, 32, 36, (32, 36, 40, 40), (0, 0, 4, 0), 3) == (0, -3), op
        assert q(O[op], 8, 32, 36, (32, 36, 40, 40), (0, 0, 0, 8), 3) == (0, -3), op
        assert q(O[op], 8, 32, 36, (32, 36, 40, 40), (0, 0, 0, 8), 0) == (0, 0), op        # no mask epilogue: its bits do not matter
    # ... and ops.linear_bwd_data sends such operands to the exact-f32 kernel, as the f16x3s chain always did
    for mode in ("bf16x3", "f16x3s"):
        v = ops.linear_variant("bwd_data", mode, 8, 32, 36, out=(40, 4, True))
        assert (v["op"], v["kernel"], v["status"]) == ("bwd_data_f32", "nn", 0), (mode, v)
        v = ops.linear_variant("bwd_data", mode, 8, 32, 36, mask=(40, 12, True))
        assert (v["op"], v["kernel"], v["status"]) == ("bwd_data_f32", "nn", 0), (mode, v)
    assert q(O["bwd_weight_f16x3s"], 8, 8, 6, (8, 6, 6, 0), (0,) * 4) == (0, -2)
    assert q(O["bwd_weight_bf16x3"], 8, 6, 8, (6, 8, 8, 0), (0,) * 4) == (0, -2)            # N % 4
    assert q(O["bwd_weight_bf16x3"], 8, 8, 6, (8, 6, 6, 0), (0,) * 4) == (0, 0)             # K % 4 != 0: the pre-pass path


def test_conv2d_variant_table_and_every_branch_is_reached():
    """What a UNet 2-D convolution op runs -- kernel family, loader form, parity classes, epilogue form, splits, the small
    kernels' grids -- asked of the library (svr_conv2d_variant: the plan functions of csrc/conv2d_plan.h, which the launchers of
    conv2d_igemm.hip, conv2d.hip and gemm_bf16x3.hip and their workspace-size functions themselves call), for every row of
    tests/_conv2d_cases.py; the rows, together, reach EVERY (op, family, loader, classes, epilogue) the launchers can produce --
    found by sweeping the query over shapes and address bits, so a launcher branch that gains a variant fails here until a case
    names it -- and the regimes inside the branches (grid-stride reduce, > 4 slabs, grid.y > 1, capped grids).  The real layers
    of Unet and UNetMini at num_filters = 32 (batch 1, 2 and 8) are pinned against tests/golden/conv2d_unet_layers.json.  No GPU."""
    import itertools
    import json
    import __graft_entry__ as ge
    ge.build()
    from svr_amd import _lib, ops
    from svr_amd.model import UNetMini, Unet
    from tests import _conv2d_cases as K
    assert len({c[0] for c in K.CASES}) == len(K.CASES)
    reached, extras = set(), set()
    for name, shape, mis, tags, ext in K.CASES:
        assert set(tags) == ({"fwd"} if shape[6] == 1 else set(K.OPS)), name
        got_ext = set()
        for op, tag in tags.items():
            v = K.query(ops, op, shape, mis)
            assert K.tag(v) == tag, (name, op, K.tag(v), tag)
            reached.add((op, tag))
            got_ext |= K.extras(v)
        assert got_ext == set(ext), (name, got_ext, ext)
        extras |= got_ext
    assert reached == K.ALL_VARIANTS, sorted(reached ^ K.ALL_VARIANTS)
    assert extras >= K.ALL_EXTRAS, sorted(K.ALL_EXTRAS - extras)
    assert len(K.ALL_VARIANTS) == 14 + 28 + 3 + 16 + 8 + 16
    # everything the launchers can answer with, over a sweep of shapes and address bits
    seen = set()
    for (H, W), C0, C1, Cout, (k, s), mis in itertools.product(((6, 5), (40, 36)), (3, 4, 68, 132), (0, 4, 5), (1, 2, 3, 4, 6, 8, 24, 66, 72),
                                                              ((3, 1), (4, 2)), ((), ("src0",), ("dy",))):
        for op in K.OPS:
            seen.add((op, K.tag(K.query(ops, op, (1, H, W, C0, C1, Cout, k, s), mis))))
    for shape in [c[1] for c in K.CASES]:
        for op in K.OPS if shape[6] != 1 else ("fwd",):
            seen.add((op, K.tag(K.query(ops, op, shape))))
    assert seen == K.ALL_VARIANTS, sorted(seen ^ K.ALL_VARIANTS)
    # the real layers
    table = json.load(open(os.path.join(REPO, "tests", "golden", "conv2d_unet_layers.json")))
    for nm, cls, (H, W) in (("full", Unet, (256, 256)), ("mini", UNetMini, (240, 320))):
        for B in (1, 2, 8):
            rows = table[f"{nm}_{H}x{W}_b{B}"]
            layers = K.unet_layers(cls, B, H, W)
            assert [r[0] for r in rows] == [n for n, _ in layers]
            for (name, shape), row in zip(layers, rows):
                vs = [K.query(ops, op, shape) for op in K.OPS]
                got = [name, list(shape)] + [K.tag(v) for v in vs] + \
                      [vs[0]["splits"], vs[1]["splits"], vs[2]["splits"] if vs[2]["family"] != "small" else vs[2]["parts"]]
                assert got == row, (nm, B, got, row)
    full8 = {r[0]: r for r in table["full_256x256_b8"]}
    assert full8["conv1"][2] == "igemm64/s/c1/lane" and full8["conv1"][5] == 1          # 1 024 tiles: the kernel's own epilogue
    assert full8["conv4"][3] == "igemm128/v4/c4/reduce_v4" and full8["dconv8"][2].startswith("small/")
    # the workspace-size functions answer from the same plans
    l = _lib.lib()
    for _, shape, _, tags, _ in K.CASES:
        B, H, W, C0, C1, Cout, k, s = shape
        d = _lib.Conv2dDesc(ctypes.c_void_p(16), ctypes.c_void_p(16) if C1 else None, B, H, W, C0, C1, k, s, 0, 0)
        if tags["fwd"].startswith("small"):
            v = K.query(ops, "bwd_weight", shape)
            assert l.svr_conv2d_small_bwd_weight_workspace(ctypes.byref(d), Cout) == v["workspace_bytes"] + 256
            continue
        need = max(K.query(ops, op, shape)["workspace_bytes"] for op in tags if op != "bwd_weight")
        assert l.svr_conv2d_workspace_bytes(ctypes.byref(d), Cout) == (need + 255) // 256 * 256 + 256, shape


def test_conv2d_variant_refuses_what_the_entry_points_refuse():
    """The query's refusals are the entry points' own (one plan function each): unknown op, bad counts, kernel sizes, the 2^24
    row-decode limit of ig_check / sm_check / svr_conv2d_bwd_weight, and an input smaller than the window -- where C division
    (truncating toward zero) used to count one output row for H = 1 at k4 s2 and the ops failed on a null pointer instead."""
    import pytest
    import svr_amd  # noqa: F401
    from svr_amd import _lib, ops
    l = _lib.lib()
    q = lambda op, *a: l.svr_conv2d_variant(op, *a, 0, 0, 0, 0, None)     # noqa: E731  (the plan may be NULL)
    ok = (2, 9, 7, 16, 0, 40, 3, 1)
    assert [q(op, *ok) for op in (0, 1, 2)] == [0, 0, 0] and q(3, *ok) == -1 and q(-1, *ok) == -1
    for op in (0, 1, 2):
        assert q(op, 0, 9, 7, 16, 0, 40, 3, 1) == -1 and q(op, 2, 9, 7, 0, 0, 40, 3, 1) == -1 and q(op, 2, 9, 7, 16, -1, 40, 3, 1) == -1
        assert q(op, 2, 9, 7, 16, 0, 0, 3, 1) == -1
        assert q(op, 2, 9, 7, 16, 0, 40, 3, 2) == -4 and q(op, 2, 9, 7, 16, 0, 40, 5, 1) == -4
        assert q(op, 2, 9, 7, 16, 0, 2, 5, 1) == -4                                   # the small kernels: k3 s1 / k4 s2 only
        # 2^24 pixels: the float row decode (cv_divmod) and the 32-bit pixel indices end there
        assert q(op, 1, 4096, 4096, 16, 0, 40, 3, 1) == -4 and q(op, 1, 4096, 4095, 16, 0, 40, 3, 1) == 0
        assert q(op, 1, 4096, 4096, 16, 0, 2, 3, 1) == -4 and q(op, 1, 4096, 4095, 16, 0, 2, 3, 1) == 0
        assert q(op, 4, 2048, 2048, 4, 0, 8, 4, 2) == -4 and q(op, 4, 2048, 2047, 4, 0, 8, 4, 2) == 0
        # no output pixel: H + 2 < k
        for shape in ((1, 1, 8, 16, 0, 40, 4, 2), (1, 8, 1, 16, 0, 40, 4, 2), (1, 1, 1, 16, 0, 2, 4, 2)):
            assert q(op, *shape) == -2, (op, shape)
            assert b"smaller than the 4 x 4 window" in l.svr_last_error() and b"1" in l.svr_last_error()
        assert q(op, 1, 2, 2, 16, 0, 40, 4, 2) == 0 and q(op, 1, 1, 1, 16, 0, 40, 3, 1) == 0
    assert q(0, 1, 1, 40, 16, 0, 16, 1, 1) == 0 and q(1, 1, 1, 40, 16, 0, 16, 1, 1) == -4 and q(2, 1, 1, 40, 16, 0, 16, 1, 1) == -4   # k = 1: forward only
    with pytest.raises(RuntimeError, match="smaller than the 4 x 4 window"):
        ops.conv2d_variant("fwd", 1, 1, 8, 16, 0, 40, 4, 2)
    # the entry points themselves, before any launch (host checks; the pointers are never followed)
    P = ctypes.c_void_p
    for H, W in ((1, 8), (8, 1)):
        d = _lib.Conv2dDesc(P(256), None, 1, H, W, 16, 0, 4, 2, 0, 0)
        r = ctypes.byref(d)
        assert l.svr_conv2d_fwd(r, P(256), P(256), None, P(256), 40, None, None, P(256), None) == -2
        assert l.svr_conv2d_bwd_data(r, P(256), P(256), P(256), None, 40, P(256), P(256), None) == -2
        assert l.svr_conv2d_bwd_weight(r, P(256), None, 40, P(256), None, P(256), None) == -2
        assert l.svr_conv2d_small_fwd(r, P(256), None, P(256), 2, None) == -2
        assert l.svr_conv2d_small_bwd_data(r, P(256), P(256), 2, P(256), None) == -2
        assert l.svr_conv2d_small_bwd_weight(r, P(256), 2, P(256), None, P(256), None) == -2
        assert l.svr_conv2d_im2col(r, P(256), None) == -2 and l.svr_conv2d_col2im(r, P(256), P(256), P(256), None, None) == -2
        assert b"smaller than the 4 x 4 window" in l.svr_last_error()
        # ... and the ops refuse on the host with the sizes, before they allocate
        x = torch.zeros(1, H, W, 16)
        for call in (lambda: ops.conv2d_im2col(x, None, 4, 2, 0, False), lambda: ops.conv2d_bwd_weight(x, None, 4, 2, 0, x, 40)):
            with pytest.raises(ValueError, match=f"input {H} x {W} .* smaller than the 4 x 4 window"):
                call()


def test_conv2d_plan_struct_matches_the_header(tmp_path):
    """svr_conv2d_plan of include/svr_hip.h, compiled as plain C, against its ctypes mirror: size and every field's offset."""
    import subprocess
    import svr_amd
    Pl = svr_amd._lib.Conv2dPlan
    names = [n for n, _ in Pl._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "svr_hip.h"', 'int main(void) {', '  printf("%zu\\n", sizeof(svr_conv2d_plan));']
    lines += [f'  printf("%zu\\n", offsetof(svr_conv2d_plan, {n}));' for n in names] + ['  return 0;', '}']
    (tmp_path / "plan.c").write_text("\n".join(lines))
    exe = tmp_path / "plan"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(tmp_path / "plan.c"), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(Pl)] + [getattr(Pl, n).offset for n in names]


def test_cv_divmod_one_correction_step_suffices(tmp_path):
    """csrc/cv_divmod.h -- the row decode of the UNet's weight-gradient kernels -- built with g++ into tests/host/cv_divmod_driver.cpp:
    q, r equal n / d, n % d exhaustively in n < 2^24 for the network's divisors and d = 1, 2, 3, 2^k +- 1, 2^24 - 1, and at the
    multiples of d +- 1 for a sweep of d."""
    import subprocess
    exe = tmp_path / "cv_divmod_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(REPO, "single-view-3d-reconstruction_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "cv_divmod_driver.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-500:])
    divisors, checks = (int(x) for x in r.stdout.split()[1:3])
    assert divisors >= 60 and checks > 60 * (1 << 24)
