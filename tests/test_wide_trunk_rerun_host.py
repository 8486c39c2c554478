"""Which networks run the pts_linears of the conditional bf16x3 RE-RUN of a forward pass in one launch (kw_rerun_b3 in
csrc/nsr_wide_trunk.inc; NSRW_FLAG_TRUNK_RERUN, WideModel(trunk="onchip", trunk_rerun="onchip")), restated in plain Python on
wide_onchip_rules and held against nsrw_trunk_rerun_plan of the built library -- the function nsrw_upload_network itself consults --
and the option's resolution.  No GPU needed; tests/test_gpu_wide_trunk_rerun.py holds the kernel to the per-layer chain's bits."""
import os
import re

import pytest

from wide_onchip_rules import LDS_LIMIT, ROOT, pad32, trunk_rule, wide      # (wide: the fixture)
from wide_onchip_rules import net as _net

DEPTHS, WIDTHS, LEVELS = (1, 2, 3, 8), (24, 40, 64, 66, 100, 128, 136, 256), (0, 10, 15, 16)


def rerun_lds(rows):
    """three bf16 piece images where the f16x2 forms have two, one column block a wave.  128 rows (4 x 2 waves, 64 columns):
    double-buffered weight stages of two k16 blocks x 2 column blocks x 3 KiB, the activation 128 rows of 64 values + 16 bytes, the
    encoding 128 rows of 96 values + 16 bytes.  64 rows (2 x 4 waves, 128 columns): stages of two k16 blocks x 4 column blocks x
    3 KiB, the activation 64 rows of 128 values + 16 bytes, the encoding 64 rows of 96 values + 16 bytes"""
    ncb = {128: 2, 64: 4}[rows]
    return 2 * (2 * ncb * 3072) + 3 * rows * (2 * 32 * ncb + 16) + 3 * rows * (2 * 96 + 16)


def rule(D, W, mlp, trunk, trunk_rerun, width):
    """None = the re-run stays a conditional GEMM launch per layer, else the rows of a tile (NJ is 1 in either form):
    trunk_rerun="onchip" on a handle whose trunk rule takes the network in its 128-row form; 128 rows up to a padded width of 64, 64
    rows at 96 and 128"""
    if trunk_rerun != "onchip":
        return None
    t = trunk_rule(D, W, mlp, trunk, width)
    if t is None or t[1] != 128:
        return None
    return 128 if pad32(W) <= 64 else 64


def reason(D, W, mlp, trunk, trunk_rerun, width):
    """why a (valid) network's re-run stays layer by layer, in the library's words and its order of asking"""
    if trunk_rerun != "onchip":
        return "NSRW_FLAG_TRUNK_RERUN not set"
    t = trunk_rule(D, W, mlp, trunk, width)
    if t is None:
        return "the trunk is not on chip"
    assert t[1] == 64
    return "padded width above 128: the wide trunk has no re-run form"


def test_lds_of_the_forms():
    assert rerun_lds(128) == 159744 and rerun_lds(64) == 141312 and max(rerun_lds(128), rerun_lds(64)) <= LDS_LIMIT == 163840


def test_trunk_rerun_plan_is_the_rule(wide):
    from neural_sim_nerf_amd import _lib
    assert [rule(3, W, "f16x2", "onchip", "onchip", 128) for W in WIDTHS] == [128, 128, 128, 64, 64, 64, None, None]
    assert [rule(3, W, "f16x2", "onchip", "onchip", 256) for W in WIDTHS] == [128, 128, 128, 64, 64, 64, None, None]
    assert rule(1, 64, "f16x2", "onchip", "onchip", 128) is None and rule(3, 64, "bf16x3", "onchip", "onchip", 128) is None
    assert rule(3, 64, "f16x2", "layers", "onchip", 128) is None and rule(3, 64, "f16x2", "onchip", "layers", 128) is None
    on = 0
    for W in WIDTHS:
        for D in DEPTHS:
            for multires in LEVELS:
                net = _net(wide, D, W, multires, [s for s in (0, 2) if s < D - 1], True)
                for mlp in wide.MLPS:
                    for trunk in wide.TRUNKS:
                        for trunk_rerun in wide.TRUNK_RERUNS:
                            for width in wide.TRUNK_WIDTHS:
                                case = (W, D, multires, mlp, trunk, trunk_rerun, width)
                                if multires > 15:                       # not a network: every plan entry refuses it
                                    with pytest.raises(_lib.NsrError, match="multires"):
                                        wide.trunk_rerun_plan(net, mlp, trunk, trunk_rerun, width)
                                    continue
                                plan = wide.trunk_rerun_plan(net, mlp, trunk, trunk_rerun, width)
                                rows = rule(D, W, mlp, trunk, trunk_rerun, width)
                                if rows is None:
                                    assert plan == dict(mode="layers", reason=reason(D, W, mlp, trunk, trunk_rerun, width)), (case, plan)
                                else:
                                    on += 1
                                    assert plan == dict(mode="onchip", nj=1, tile_rows=rows, lds_bytes=rerun_lds(rows)), (case, plan)
                                    front = wide.trunk_plan(net, mlp, trunk, width)
                                    assert front["mode"] == "onchip" and front["tile_rows"] == 128, (case, front)
    assert on == 6 * 3 * 3 * 2                # the six widths up to 128, three depths, the three encodings, either trunk_width
    # the wide trunk: on chip, and no re-run form
    n = _net(wide, 3, 136, 10, [0])
    assert wide.trunk_plan(n, "f16x2", "onchip", 256)["tile_rows"] == 64
    assert wide.trunk_rerun_plan(n, "f16x2", "onchip", "onchip", 256) == \
        dict(mode="layers", reason="padded width above 128: the wide trunk has no re-run form")
    assert wide.trunk_rerun_plan(n, "f16x2", "onchip", "onchip", 128) == dict(mode="layers", reason="the trunk is not on chip")
    with pytest.raises(ValueError, match="trunk_rerun must be"):
        wide.trunk_rerun_plan(n, "f16x2", "onchip", "lds")


def test_trunk_rerun_plan_reads_state_dicts_and_every_flag_combination(wide, oracle):
    sd = oracle.synth_weights_shape(1, 3, 40, 15, 2, [1], True)
    assert wide.trunk_rerun_plan(sd, "f16x2") == dict(mode="onchip", nj=1, tile_rows=128, lds_bytes=159744)
    assert wide.trunk_rerun_plan(oracle.synth_weights_shape(1, 3, 100, 0, 2, [0], False), "f16x2") == \
        dict(mode="onchip", nj=1, tile_rows=64, lds_bytes=141312)
    # the decision reads the trunk's flags and its own, none of the other forms'
    lib, C = wide.load(), wide.C
    f16, on, rr = wide.FLAG_MLP_F16X2, wide.FLAG_TRUNK_ONCHIP, wide.FLAG_TRUNK_RERUN
    others = (0, wide.FLAG_HEADS_ONCHIP, wide.FLAG_TRUNK_BWD, wide.FLAG_TRUNK_BWD | wide.FLAG_TRUNK_KEEP, wide.FLAG_STAGES_WAVE,
              wide.FLAG_HEADS_ONCHIP | wide.FLAG_TRUNK_BWD | wide.FLAG_TRUNK_KEEP | wide.FLAG_STAGES_WAVE | wide.FLAG_WHITE_BKGD)
    for W in WIDTHS:
        net = _net(wide, 3, W, 10, [0])
        for base, want in ((0, b"the trunk is not on chip"), (f16, b"the trunk is not on chip"), (on, b"the trunk is not on chip"),
                           (wide.FLAG_MLP_BF16X3 | on, b"the trunk is not on chip"), (f16 | on, None),
                           (f16 | on | wide.FLAG_TRUNK_WIDE, None)):
            for extra in others:
                plan = wide.NsrwTrunkPlan()
                assert lib.nsrw_trunk_rerun_plan(C.byref(net), base | extra, C.byref(plan)) == 0
                assert plan.onchip == 0 and plan.reason == b"NSRW_FLAG_TRUNK_RERUN not set", (W, base, extra)
                assert lib.nsrw_trunk_rerun_plan(C.byref(net), base | extra | rr, C.byref(plan)) == 0
                if want is None and pad32(W) <= 128:
                    rows = 128 if pad32(W) <= 64 else 64
                    assert (plan.onchip, plan.nj, plan.tile_rows, plan.lds_bytes) == (1, 1, rows, rerun_lds(rows)), (W, base, extra)
                elif want is None:
                    wide_form = base & wide.FLAG_TRUNK_WIDE and pad32(W) <= 256
                    assert plan.onchip == 0 and plan.reason == (b"padded width above 128: the wide trunk has no re-run form" if wide_form
                                                                else b"the trunk is not on chip"), (W, base, extra, plan.reason)
                else:
                    assert plan.onchip == 0 and (plan.nj, plan.tile_rows, plan.lds_bytes) == (0, 0, 0) and plan.reason == want, (W, base, extra)


def test_the_other_plans_do_not_read_the_flag(wide):
    """without NSRW_FLAG_TRUNK_RERUN all four existing plans are what they were, and with it they are too"""
    lib, C = wide.load(), wide.C
    f16, on, hd, wd, bw, kp = (wide.FLAG_MLP_F16X2, wide.FLAG_TRUNK_ONCHIP, wide.FLAG_HEADS_ONCHIP, wide.FLAG_TRUNK_WIDE,
                               wide.FLAG_TRUNK_BWD, wide.FLAG_TRUNK_KEEP)
    for W in WIDTHS + (8, 32, 160, 257, 300):
        for D in DEPTHS:
            net = _net(wide, D, W, 10, [0] if D > 2 else [])
            for base in (0, f16, f16 | on, f16 | on | bw, f16 | on | bw | kp, f16 | on | hd | wd | bw | kp, wide.FLAG_MLP_BF16X3):
                for entry, struct in (("nsrw_trunk_plan", wide.NsrwTrunkPlan), ("nsrw_heads_plan", wide.NsrwHeadsPlan),
                                      ("nsrw_trunk_bwd_plan", wide.NsrwTrunkPlan), ("nsrw_trunk_keep_plan", wide.NsrwTrunkPlan)):
                    a, b = struct(), struct()
                    assert getattr(lib, entry)(C.byref(net), base, C.byref(a)) == 0
                    assert getattr(lib, entry)(C.byref(net), base | wide.FLAG_TRUNK_RERUN, C.byref(b)) == 0
                    assert bytes(a) == bytes(b), (entry, W, D, base)


def test_the_plans_lds_bytes_are_those_of_the_kernels_they_select(wide):
    """Either form: the lds_bytes of the plan equals the LDS the kernel it selects has in the built library -- the code object's
    group_segment_fixed_size (tools/kernel_resources.py); the two named here are all the kw_rerun_b3 the library instantiates; a
    512-thread workgroup has at most 256 VGPRs a lane, and neither kernel spills or has scratch."""
    import sys
    lib = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(lib)[0]
    seen = {}
    for W in (24, 40, 64, 66, 100, 128):
        plan = wide.trunk_rerun_plan(_net(wide, 3, W, 4, [0]), "f16x2")
        assert plan["mode"] == "onchip" and plan["nj"] == 1, (W, plan)
        kernel = "kw_rerun_b3<1, %d>" % (plan["tile_rows"] // 32)
        assert plan["lds_bytes"] == res[kernel]["group_segment_fixed_size"], (W, kernel, plan, res[kernel])
        seen[kernel] = plan["lds_bytes"]
    assert seen == {"kw_rerun_b3<1, 4>": rerun_lds(128), "kw_rerun_b3<1, 2>": rerun_lds(64)}, seen
    assert sorted(seen) == sorted(k for k in res if k.startswith("kw_rerun")), sorted(res)
    for k in seen:
        assert res[k]["vgpr_count"] <= 256 and res[k]["vgpr_spill_count"] == 0 and res[k]["private_segment_fixed_size"] == 0, (k, res[k])


def test_flag_and_signatures_are_declared(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert re.search(r"enum\s*\{\s*NSRW_FLAG_TRUNK_RERUN\s*=\s*\(?\s*1 << 10\s*\)?\s*\}", hdr) and wide.FLAG_TRUNK_RERUN == 1024 == 1 << 10
    assert "NSRW_FLAG_TRUNK_RERUN = 1024" not in hdr
    assert "int nsrw_trunk_rerun_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);" in hdr
    assert "int nsrw_rerun_status(nsrw_handle h, unsigned long long* launches_onchip);" in hdr
    assert {"nsrw_trunk_rerun_plan", "nsrw_rerun_status"} <= set(wide.SIGNATURES) and wide.TRUNK_RERUNS == ("layers", "onchip")
    # the bit is free: no other flag of the module has it
    flags = {k: v for k, v in vars(wide).items() if k.startswith("FLAG_") and k != "FLAG_TRUNK_RERUN"}
    assert len(flags) == 12 and not any(v & 1024 for v in flags.values()), flags
    lib, C = wide.load(), wide.C
    plan = wide.NsrwTrunkPlan()
    net = _net(wide, 3, 100, 10, [0])
    assert lib.nsrw_trunk_rerun_plan(C.byref(net), 1024 | 8, C.byref(plan)) == 0
    assert plan.onchip == 0 and (plan.nj, plan.tile_rows, plan.lds_bytes) == (0, 0, 0) and plan.reason == b"the trunk is not on chip"
    assert lib.nsrw_trunk_rerun_plan(C.byref(net), 1024 | 16 | 8, C.byref(plan)) == 0
    assert (plan.onchip, plan.nj, plan.tile_rows, plan.lds_bytes) == (1, 1, 64, 141312)
    assert lib.nsrw_trunk_rerun_plan(C.byref(_net(wide, 3, 1)), 1024 | 16 | 8, C.byref(plan)) == -1
    assert "netwidth" in lib.nsrw_last_error().decode()
    assert lib.nsrw_trunk_rerun_plan(None, 1024 | 16 | 8, C.byref(plan)) == -1 and "null" in lib.nsrw_last_error().decode()
    n = C.c_ulonglong(7)
    assert lib.nsrw_rerun_status(None, C.byref(n)) != 0 and "null" in lib.nsrw_last_error().decode()
