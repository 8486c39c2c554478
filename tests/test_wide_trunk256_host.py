"""Which networks the WIDE form of the layered renderer's on-chip trunk takes (kw_trunk_h2<2, false, 2> in csrc/nsr_wide_trunk.inc;
NSRW_FLAG_TRUNK_WIDE, WideModel(trunk="onchip", trunk_width=256)), restated in plain Python and held against nsrw_trunk_plan /
nsrw_heads_plan of the built library -- the functions nsrw_upload_network itself consults.  No GPU needed."""
import os

import pytest

from wide_onchip_rules import LDS_LIMIT, ROOT, pad32, wide      # (wide: the fixture)
from wide_onchip_rules import net as _net
from wide_onchip_rules import trunk_lds as lds_bytes
from wide_onchip_rules import trunk_nj as rule_128
from wide_onchip_rules import trunk_reason_128 as reason_128
from wide_onchip_rules import trunk_rule as rule

WIDTHS = (2, 64, 128, 129, 136, 160, 161, 192, 200, 224, 256, 257, 288, 1024)
DEPTHS, LEVELS = (1, 2, 3, 8, 64), (0, 4, 10, 15)
lds_bytes_128 = lds_bytes


def _cases(wide):
    for W in WIDTHS:
        for D in DEPTHS:
            for multires in LEVELS:
                net = _net(wide, D, W, multires, [s for s in (0, 4) if s < D - 1])
                for mlp in wide.MLPS:
                    for trunk in wide.TRUNKS:
                        yield net, (W, D, mlp, trunk, multires)


def test_trunk_plan_with_trunk_width_256_is_the_rule(wide):
    assert lds_bytes(2, 64) == 67584 + 26624 + 65536 == 159744
    assert [rule(3, W, "f16x2", "onchip", 256) for W in (128, 129, 160, 161, 224, 256, 257)] == \
        [(2, 128), (2, 64), (2, 64), (2, 64), (2, 64), (2, 64), None]
    assert rule(1, 256, "f16x2", "onchip", 256) is None and rule(8, 256, "bf16x3", "onchip", 256) is None
    assert rule(8, 256, "f16x2", "layers", 256) is None and rule(8, 256, "f16x2", "onchip", 128) is None
    n_wide = 0
    for net, case in _cases(wide):
        W, D, mlp, trunk, multires = case
        plan = wide.trunk_plan(net, mlp, trunk, trunk_width=256)
        want = rule(D, W, mlp, trunk, 256)
        if want is None:
            assert plan["mode"] == "layers" and plan["reason"], (case, plan)
        else:
            assert plan == dict(mode="onchip", nj=want[0], tile_rows=want[1], lds_bytes=lds_bytes(*want)), (case, plan)
            assert plan["lds_bytes"] <= LDS_LIMIT == 163840, case
            n_wide += want[1] == 64
    assert n_wide == 8 * 4 * 4          # the eight widths 129 .. 256, four depths, every encoding
    assert "256" in wide.trunk_plan(_net(wide, 3, 257), "f16x2", "onchip", trunk_width=256)["reason"]
    with pytest.raises(ValueError, match="trunk_width"):
        wide.trunk_plan(_net(wide, 3, 256), "f16x2", "onchip", trunk_width=192)


def test_trunk_plan_with_trunk_width_128_is_as_before(wide):
    for net, case in _cases(wide):
        W, D, mlp, trunk, multires = case
        want = rule_128(D, W, mlp, trunk)
        for plan in (wide.trunk_plan(net, mlp, trunk), wide.trunk_plan(net, mlp, trunk, 128), wide.trunk_plan(net, mlp, trunk, trunk_width=128)):
            if want is None:
                assert plan == dict(mode="layers", reason=reason_128(D, W, mlp, trunk)), (case, plan)
            else:
                assert plan == dict(mode="onchip", nj=want, tile_rows=128, lds_bytes=lds_bytes_128(want)), (case, plan)
    for W in (129, 136, 256):
        assert wide.trunk_plan(_net(wide, 3, W, 10, [0]), "f16x2") == dict(mode="layers", reason="padded width above 128")
    assert wide.TRUNKS == ("layers", "onchip") and wide.HEADS == ("layers", "onchip")


def test_heads_plan_leaves_the_heads_of_a_wide_trunk_as_launches(wide):
    for W in (2, 64, 100, 128):
        for viewdirs in (True, False):
            net = _net(wide, 3, W, 10, [0], viewdirs)
            plan = wide.heads_plan(net, "f16x2", "onchip", "onchip", trunk_width=256)
            assert plan == dict(mode="onchip", lds_bytes=lds_bytes_128(1 if pad32(W) <= 64 else 2)), (W, plan)
            assert plan == wide.heads_plan(net, "f16x2", "onchip", "onchip") == wide.heads_plan(net, "f16x2", "onchip", "onchip", 128)
    for W in (136, 256):
        net = _net(wide, 3, W, 10, [0])
        plan = wide.heads_plan(net, "f16x2", "onchip", "onchip", trunk_width=256)
        assert plan["mode"] == "layers" and "128" in plan["reason"], (W, plan)
        assert wide.trunk_plan(net, "f16x2", "onchip", trunk_width=256)["tile_rows"] == 64
        assert wide.heads_plan(net, "f16x2", "onchip", "onchip") == dict(mode="layers", reason="the trunk is not on chip")


def test_flag_is_declared_and_needs_the_onchip_flag(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert "NSRW_FLAG_TRUNK_WIDE = 64" in hdr and wide.FLAG_TRUNK_WIDE == 64
    lib, C = wide.load(), wide.C
    net = _net(wide, 3, 256, 10, [1])
    plan = wide.NsrwTrunkPlan()
    assert lib.nsrw_trunk_plan(C.byref(net), 64 | 8, C.byref(plan)) == 0
    assert plan.onchip == 0 and (plan.nj, plan.tile_rows, plan.lds_bytes) == (0, 0, 0) and plan.reason == b"NSRW_FLAG_TRUNK_ONCHIP not set"
    assert lib.nsrw_trunk_plan(C.byref(net), 64 | 16 | 8, C.byref(plan)) == 0
    assert (plan.onchip, plan.nj, plan.tile_rows, plan.lds_bytes) == (1, 2, 64, 159744)
    assert lib.nsrw_trunk_plan(C.byref(net), 16 | 8, C.byref(plan)) == 0 and plan.onchip == 0
    assert lib.nsrw_trunk_plan(C.byref(_net(wide, 3, 1)), 64 | 16 | 8, C.byref(plan)) == -1
    assert "netwidth" in lib.nsrw_last_error().decode()
    hp = wide.NsrwHeadsPlan()
    assert lib.nsrw_heads_plan(C.byref(net), 64 | 32 | 16 | 8, C.byref(hp)) == 0 and hp.onchip == 0 and hp.reason
    assert lib.nsrw_heads_plan(C.byref(_net(wide, 3, 1)), 64 | 32 | 16 | 8, C.byref(hp)) == -1


def test_widemodel_refuses_a_trunk_width_it_cannot_honour(wide):
    """(the arguments are judged before a device is asked for)"""
    with pytest.raises(NotImplementedError, match="trunk_width=256"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="layers", trunk_width=256)
    with pytest.raises(NotImplementedError, match="f16x2"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="bf16x3", trunk="layers", trunk_width=256)
    for bad in (192, 0, "wide"):
        with pytest.raises(ValueError, match="trunk_width must be"):
            wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip", trunk_width=bad)
