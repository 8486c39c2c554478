"""Which networks run the f16x2 pass of a KEPT forward -- one that keeps its activations for a backward -- in the layered renderer's
on-chip kept kernel (kw_keep_h2 / kw_keep_bwd_h2 in csrc/nsr_wide_trunk.inc; NSRW_FLAG_TRUNK_KEEP, WideModel(trunk="onchip",
trunk_bwd="onchip", trunk_keep="onchip")), restated in plain Python on wide_onchip_rules and held against nsrw_trunk_keep_plan of the
built library -- the function nsrw_upload_network itself consults.  No GPU needed."""
import os

import pytest

from wide_onchip_rules import LDS_LIMIT, ROOT, bwd_lds, bwd_rule, heads_rule, trunk_lds, trunk_nj, wide      # (wide: the fixture)
from wide_onchip_rules import net as _net

WIDTHS = (8, 24, 32, 33, 40, 64, 65, 96, 100, 128, 129, 136, 160, 200, 256, 257, 300)
DEPTHS, LEVELS = (1, 2, 3, 4), (0, 4, 10, 15)


def rule(D, W, multires, mlp, trunk, trunk_bwd, trunk_keep, width):
    """None = the kept forward stays a GEMM launch per layer, else the NJ of the kept kernel: trunk_keep="onchip" on a handle whose
    backward rule takes the network (so f16x2, the 128-row forward form, two layers); the forward's NJ, not the backward's"""
    if trunk_keep != "onchip" or bwd_rule(D, W, multires, mlp, trunk, trunk_bwd, width) is None:
        return None
    return trunk_nj(D, W, mlp, trunk)


def reason(trunk_keep):
    """why a (valid) network keeps fp32 activations layer by layer, in the library's words and its order of asking"""
    return "NSRW_FLAG_TRUNK_KEEP not set" if trunk_keep != "onchip" else "the backward trunk is not on chip"


def test_trunk_keep_plan_is_the_rule(wide):
    assert [rule(3, W, 4, "f16x2", "onchip", "onchip", "onchip", 128) for W in (24, 64, 65, 128, 129)] == [1, 1, 2, 2, None]
    assert [rule(3, 40, L, "f16x2", "onchip", "onchip", "onchip", 128) for L in LEVELS] == [1, 1, 1, 1]      # the forward's NJ
    assert rule(3, 64, 4, "f16x2", "onchip", "layers", "onchip", 128) is None and rule(3, 64, 4, "f16x2", "onchip", "onchip", "layers", 128) is None
    assert rule(1, 64, 4, "f16x2", "onchip", "onchip", "onchip", 128) is None and rule(3, 200, 4, "f16x2", "onchip", "onchip", "onchip", 256) is None
    on = 0
    for W in WIDTHS:
        for D in DEPTHS:
            for multires in LEVELS:
                net = _net(wide, D, W, multires, [s for s in (0, 2) if s < D - 1], True)
                for mlp in wide.MLPS:
                    for trunk in wide.TRUNKS:
                        for trunk_bwd in wide.TRUNK_BWDS:
                            for trunk_keep in wide.TRUNK_KEEPS:
                                for width in wide.TRUNK_WIDTHS:
                                    for heads in wide.HEADS:
                                        plan = wide.trunk_keep_plan(net, mlp, trunk, trunk_bwd, trunk_keep, heads, width)
                                        want = rule(D, W, multires, mlp, trunk, trunk_bwd, trunk_keep, width)
                                        case = (W, D, multires, mlp, trunk, trunk_bwd, trunk_keep, heads, width)
                                        if want is None:
                                            assert plan == dict(mode="layers", reason=reason(trunk_keep)), (case, plan)
                                        else:
                                            on += 1
                                            assert plan == dict(mode="onchip", nj=want, tile_rows=128, lds_bytes=trunk_lds(want)), (case, plan)
                                            assert plan["lds_bytes"] <= LDS_LIMIT == 163840, case
                                            bwd = wide.trunk_bwd_plan(net, mlp, trunk, trunk_bwd, width)
                                            assert bwd["mode"] == "onchip" and bwd["tile_rows"] == 128, (case, bwd)
    assert on == 10 * 3 * 4 * 2 * 2           # the ten widths up to 128, three depths, every encoding, either trunk_width, either heads


def test_trunk_keep_plan_reads_state_dicts_and_refuses_invalid_networks(wide, oracle):
    sd = oracle.synth_weights_shape(1, 3, 40, 15, 2, [1], True)
    assert wide.trunk_keep_plan(sd, "f16x2") == dict(mode="onchip", nj=1, tile_rows=128, lds_bytes=trunk_lds(1))
    assert wide.trunk_bwd_plan(sd, "f16x2")["nj"] == 2          # (the backward launch of the same network: NJ = 2 by the encoding)
    assert wide.trunk_keep_plan(oracle.synth_weights_shape(1, 3, 100, 0, 2, [0], False), "f16x2", heads="onchip")["nj"] == 2
    assert wide.trunk_keep_plan(oracle.synth_weights_shape(1, 3, 136, 4, 2, [1], True), "f16x2", trunk_width=256) == \
        dict(mode="layers", reason="the backward trunk is not on chip")
    assert wide.trunk_keep_plan(sd, "f16x2", trunk_bwd="layers") == dict(mode="layers", reason="the backward trunk is not on chip")
    assert wide.trunk_keep_plan(sd, "f16x2", trunk_keep="layers") == dict(mode="layers", reason="NSRW_FLAG_TRUNK_KEEP not set")
    from neural_sim_nerf_amd import _lib
    with pytest.raises(_lib.NsrError, match="netwidth"):
        wide.trunk_keep_plan(_net(wide, 3, 1), "f16x2")


def test_the_other_plans_do_not_read_the_flag(wide):
    """without NSRW_FLAG_TRUNK_KEEP all four existing plans are what they were, and with it they are too"""
    lib, C = wide.load(), wide.C
    f16, on, hd, wd, bw = wide.FLAG_MLP_F16X2, wide.FLAG_TRUNK_ONCHIP, wide.FLAG_HEADS_ONCHIP, wide.FLAG_TRUNK_WIDE, wide.FLAG_TRUNK_BWD
    for W in WIDTHS:
        for D in DEPTHS:
            net = _net(wide, D, W, 10, [0] if D > 2 else [])
            for base in (0, f16, f16 | on, f16 | on | bw, f16 | on | hd | wd | bw):
                for entry, struct in (("nsrw_trunk_plan", wide.NsrwTrunkPlan), ("nsrw_heads_plan", wide.NsrwHeadsPlan),
                                      ("nsrw_trunk_bwd_plan", wide.NsrwTrunkPlan)):
                    a, b = struct(), struct()
                    assert getattr(lib, entry)(C.byref(net), base, C.byref(a)) == 0
                    assert getattr(lib, entry)(C.byref(net), base | wide.FLAG_TRUNK_KEEP, C.byref(b)) == 0
                    assert bytes(a) == bytes(b), (entry, W, D, base)
                plan = wide.NsrwTrunkPlan()
                assert lib.nsrw_trunk_keep_plan(C.byref(net), base, C.byref(plan)) == 0
                assert plan.onchip == 0 and plan.reason == b"NSRW_FLAG_TRUNK_KEEP not set", (W, D, base)


def test_the_plans_lds_bytes_are_those_of_the_kernels_they_select(wide):
    """Every new form: the lds_bytes of the plan equals the LDS the kernel it selects has in the built library -- the code object's
    group_segment_fixed_size (tools/kernel_resources.py).  kw_keep_h2<nj, heads> by nsrw_trunk_keep_plan and nsrw_heads_plan,
    kw_keep_bwd_h2<nj> by nsrw_trunk_bwd_plan, whose launch it replaces; the six named here are all the library instantiates."""
    import sys
    lib = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(lib)[0]
    seen = {}
    for W, L in ((40, 4), (128, 4), (40, 15)):             # NJ = 1, 2; the backward's NJ = 2 by the encoding
        n = _net(wide, 3, W, L, [0])
        for heads in wide.HEADS:
            keep = wide.trunk_keep_plan(n, "f16x2", heads=heads)
            hp = wide.heads_plan(n, "f16x2", "onchip", heads)
            bwd = wide.trunk_bwd_plan(n, "f16x2")
            assert keep["mode"] == bwd["mode"] == "onchip" and hp["mode"] == heads, (W, L, heads, keep, hp, bwd)
            assert (heads_rule(3, W, 4, True, "f16x2", "onchip", heads) is not None) == (heads == "onchip")
            for kernel, plan in (("kw_keep_h2<%d, %d>" % (keep["nj"], heads == "onchip"), keep), ("kw_keep_bwd_h2<%d>" % bwd["nj"], bwd)):
                assert plan["lds_bytes"] == res[kernel]["group_segment_fixed_size"], (W, L, kernel, plan, res[kernel])
                seen[kernel] = plan["lds_bytes"]
    assert seen == {"kw_keep_h2<1, 0>": trunk_lds(1), "kw_keep_h2<2, 0>": trunk_lds(2), "kw_keep_h2<1, 1>": trunk_lds(1),
                    "kw_keep_h2<2, 1>": trunk_lds(2), "kw_keep_bwd_h2<1>": bwd_lds(1), "kw_keep_bwd_h2<2>": bwd_lds(2)}, seen
    assert sorted(seen) == sorted(k for k in res if k.startswith("kw_keep")), sorted(res)
    assert "kw_mask_pack" in res and "kw_mask_unpack" in res
    for k in list(seen) + ["kw_mask_pack", "kw_mask_unpack"]:
        assert res[k]["vgpr_spill_count"] == 0 and res[k]["private_segment_fixed_size"] == 0, (k, res[k])


def test_flag_and_signatures_are_declared(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert "NSRW_FLAG_TRUNK_KEEP = 256" in hdr and wide.FLAG_TRUNK_KEEP == 256
    assert "int nsrw_trunk_keep_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);" in hdr
    assert "int nsrw_keep_status(nsrw_handle h, unsigned long long* passes_onchip);" in hdr
    assert "nsrw_trunk_keep_plan" in wide.SIGNATURES and "nsrw_keep_status" in wide.SIGNATURES and wide.TRUNK_KEEPS == ("layers", "onchip")
    lib, C = wide.load(), wide.C
    plan = wide.NsrwTrunkPlan()
    net = _net(wide, 3, 100, 10, [0])
    assert lib.nsrw_trunk_keep_plan(C.byref(net), 256 | 16 | 8, C.byref(plan)) == 0
    assert plan.onchip == 0 and (plan.nj, plan.tile_rows, plan.lds_bytes) == (0, 0, 0) and plan.reason == b"the backward trunk is not on chip"
    assert lib.nsrw_trunk_keep_plan(C.byref(net), 256 | 128 | 16 | 8, C.byref(plan)) == 0
    assert (plan.onchip, plan.nj, plan.tile_rows, plan.lds_bytes) == (1, 2, 128, 155648)
    assert lib.nsrw_trunk_keep_plan(C.byref(net), 256 | 128 | 32 | 16 | 8, C.byref(plan)) == 0
    assert (plan.onchip, plan.nj, plan.tile_rows, plan.lds_bytes) == (1, 2, 128, 155648)
    assert lib.nsrw_trunk_keep_plan(C.byref(_net(wide, 3, 1)), 256 | 128 | 16 | 8, C.byref(plan)) == -1
    assert "netwidth" in lib.nsrw_last_error().decode()
    n = C.c_ulonglong(7)
    assert lib.nsrw_keep_status(None, C.byref(n)) != 0 and "null" in lib.nsrw_last_error().decode()
