"""Which networks run their heads behind the layered renderer's on-chip trunk (the heads form of kw_trunk_h2 in
csrc/nsr_wide_trunk.inc), restated in plain Python and held against nsrw_heads_plan of the built library -- the function
nsrw_upload_network itself consults.  No GPU needed."""
import os

import pytest

from wide_onchip_rules import LDS_LIMIT, ROOT, pad32, wide      # (wide: the fixture)
from wide_onchip_rules import heads_rule as rule
from wide_onchip_rules import net
from wide_onchip_rules import trunk_lds as lds_bytes

WIDTHS, DEPTHS, VIEW_LEVELS = (2, 24, 40, 64, 66, 100, 128, 129, 256), (1, 2, 8), (0, 2, 4, 6, 15)


def _net(wide, D, W, multires_views, viewdirs, multires=10, skips=()):
    return net(wide, D, W, multires, skips, viewdirs, multires_views)


def test_heads_plan_is_the_rule(wide):
    assert wide.HEADS == ("layers", "onchip")
    assert [rule(3, W, 4, True, "f16x2", "onchip", "onchip") for W in WIDTHS] == [1, 1, 1, 1, 2, 2, 2, None, None]
    assert rule(1, 64, 4, True, "f16x2", "onchip", "onchip") is None and rule(8, 64, 4, True, "f16x2", "layers", "onchip") is None
    assert rule(8, 64, 4, True, "bf16x3", "onchip", "onchip") is None and rule(8, 64, 4, True, "f16x2", "onchip", "layers") is None
    on = 0
    for W in WIDTHS:
        for D in DEPTHS:
            for Lv in VIEW_LEVELS:
                for viewdirs in (True, False):
                    net = _net(wide, D, W, Lv, viewdirs, skips=[0] if D > 2 else [])
                    for mlp in wide.MLPS:
                        for trunk in wide.TRUNKS:
                            for heads in wide.HEADS:
                                plan = wide.heads_plan(net, mlp, trunk, heads)
                                want = rule(D, W, Lv, viewdirs, mlp, trunk, heads)
                                case = (W, D, Lv, viewdirs, mlp, trunk, heads)
                                if want is None:
                                    assert plan["mode"] == "layers" and plan["reason"], (case, plan)
                                else:
                                    on += 1
                                    assert plan == dict(mode="onchip", lds_bytes=lds_bytes(want)), (case, plan)
                                    assert plan["lds_bytes"] <= LDS_LIMIT == 163840, case
                                    assert wide.trunk_plan(net, mlp, trunk)["mode"] == "onchip", case
    assert on == 7 * 2 * 5 * 2           # the seven widths up to 128, two depths, every direction encoding, with and without
    # the reasons name what is missing
    net = _net(wide, 3, 64, 4, True)
    assert "NSRW_FLAG_HEADS_ONCHIP" in wide.heads_plan(net, "f16x2", "onchip", "layers")["reason"]
    assert "trunk" in wide.heads_plan(net, "f16x2", "layers", "onchip")["reason"]
    assert "trunk" in wide.heads_plan(_net(wide, 3, 136, 4, True), "f16x2", "onchip", "onchip")["reason"]
    assert pad32(3 + 6 * 15) == 96       # multires_views = 15, the widest direction encoding there is, still fits


def test_heads_plan_reads_state_dicts_and_refuses_invalid_networks(wide, oracle):
    sd = oracle.synth_weights_shape(1, 3, 66, 4, 6, [0], True)
    assert wide.heads_plan(sd, "f16x2") == dict(mode="onchip", lds_bytes=lds_bytes(2))
    assert wide.heads_plan(oracle.synth_weights_shape(1, 3, 40, 4, 2, [0], False), "f16x2") == dict(mode="onchip", lds_bytes=lds_bytes(1))
    assert wide.heads_plan(oracle.synth_weights_shape(1, 3, 136, 4, 2, [1], True), "f16x2")["mode"] == "layers"
    from neural_sim_nerf_amd import _lib
    with pytest.raises(_lib.NsrError, match="netwidth"):
        wide.heads_plan(_net(wide, 3, 1, 4, True), "f16x2")


def test_the_trunk_plan_does_not_read_the_heads_flag(wide):
    lib = wide.load()
    for W in WIDTHS:
        for D in DEPTHS:
            for viewdirs in (True, False):
                net = _net(wide, D, W, 4, viewdirs)
                for base in (0, wide.FLAG_MLP_F16X2, wide.FLAG_MLP_F16X2 | wide.FLAG_TRUNK_ONCHIP, wide.FLAG_MLP_BF16X3 | wide.FLAG_TRUNK_ONCHIP):
                    a, b = wide.NsrwTrunkPlan(), wide.NsrwTrunkPlan()
                    assert lib.nsrw_trunk_plan(wide.C.byref(net), base, wide.C.byref(a)) == 0
                    assert lib.nsrw_trunk_plan(wide.C.byref(net), base | wide.FLAG_HEADS_ONCHIP, wide.C.byref(b)) == 0
                    assert bytes(a) == bytes(b), (W, D, viewdirs, base)


def test_flag_and_signature_are_declared(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert "NSRW_FLAG_HEADS_ONCHIP = 32" in hdr and wide.FLAG_HEADS_ONCHIP == 32
    assert "int nsrw_heads_plan(const NsrwNet* net, int flags, NsrwHeadsPlan* plan_out);" in hdr
    assert "int32_t onchip, lds_bytes;" in hdr and "nsrw_heads_plan" in wide.SIGNATURES
