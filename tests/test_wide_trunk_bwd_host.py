"""Which networks run the input-gradient chain of their gradient calls in the layered renderer's on-chip BACKWARD trunk
(kw_trunk_bwd_h2 in csrc/nsr_wide_trunk.inc; NSRW_FLAG_TRUNK_BWD, WideModel(trunk="onchip", trunk_bwd="onchip")), restated in plain
Python and held against nsrw_trunk_bwd_plan of the built library -- the function nsrw_upload_network itself consults.  No GPU needed."""
import os

import pytest

from wide_onchip_rules import LDS_LIMIT, ROOT, wide      # (wide: the fixture)
from wide_onchip_rules import bwd_lds as lds_bytes
from wide_onchip_rules import bwd_reason as reason
from wide_onchip_rules import bwd_rule as rule
from wide_onchip_rules import net as _net

WIDTHS = (8, 24, 32, 33, 40, 64, 65, 96, 100, 128, 129, 136, 160, 200, 256, 257, 300)
DEPTHS, LEVELS = (1, 2, 3, 4), (0, 4, 10, 15)


def test_trunk_bwd_plan_is_the_rule(wide):
    assert (lds_bytes(1), lds_bytes(2)) == (53248, 102400)
    assert [rule(3, W, 4, "f16x2", "onchip", "onchip", 128) for W in (24, 64, 65, 128, 129)] == [1, 1, 2, 2, None]
    assert [rule(3, 40, L, "f16x2", "onchip", "onchip", 128) for L in LEVELS] == [1, 1, 1, 2]        # NJ = 2 by the encoding alone
    assert rule(1, 64, 4, "f16x2", "onchip", "onchip", 128) is None and rule(3, 200, 4, "f16x2", "onchip", "onchip", 256) is None
    assert rule(3, 64, 4, "f16x2", "layers", "onchip", 128) is None and rule(3, 64, 4, "bf16x3", "onchip", "onchip", 128) is None
    on = 0
    for W in WIDTHS:
        for D in DEPTHS:
            for multires in LEVELS:
                for viewdirs in (True, False):
                    net = _net(wide, D, W, multires, [s for s in (0, 2) if s < D - 1], viewdirs)
                    for mlp in wide.MLPS:
                        for trunk in wide.TRUNKS:
                            for trunk_bwd in wide.TRUNK_BWDS:
                                for width in wide.TRUNK_WIDTHS:
                                    plan = wide.trunk_bwd_plan(net, mlp, trunk, trunk_bwd, width)
                                    want = rule(D, W, multires, mlp, trunk, trunk_bwd, width)
                                    case = (W, D, multires, viewdirs, mlp, trunk, trunk_bwd, width)
                                    if want is None:
                                        assert plan == dict(mode="layers", reason=reason(D, W, mlp, trunk, trunk_bwd, width)), (case, plan)
                                    else:
                                        on += 1
                                        assert plan == dict(mode="onchip", nj=want, tile_rows=128, lds_bytes=lds_bytes(want)), (case, plan)
                                        assert plan["lds_bytes"] <= LDS_LIMIT == 163840, case
                                        fwd = wide.trunk_plan(net, mlp, trunk, width)
                                        assert fwd["mode"] == "onchip" and fwd["tile_rows"] == 128, (case, fwd)
    assert on == 10 * 3 * 4 * 2 * 2           # the ten widths up to 128, three depths, every encoding, with and without view
    #                                           directions, either trunk_width


def test_trunk_bwd_plan_reads_state_dicts_and_refuses_invalid_networks(wide, oracle):
    assert wide.trunk_bwd_plan(oracle.synth_weights_shape(1, 3, 40, 4, 2, [1], True), "f16x2") == \
        dict(mode="onchip", nj=1, tile_rows=128, lds_bytes=lds_bytes(1))
    assert wide.trunk_bwd_plan(oracle.synth_weights_shape(1, 3, 40, 15, 2, [1], True), "f16x2")["nj"] == 2
    assert wide.trunk_bwd_plan(oracle.synth_weights_shape(1, 3, 100, 0, 2, [0], False), "f16x2")["nj"] == 2
    assert wide.trunk_bwd_plan(oracle.synth_weights_shape(1, 3, 136, 4, 2, [1], True), "f16x2", trunk_width=256) == \
        dict(mode="layers", reason="padded width above 128: the wide trunk has no backward form")
    from neural_sim_nerf_amd import _lib
    with pytest.raises(_lib.NsrError, match="netwidth"):
        wide.trunk_bwd_plan(_net(wide, 3, 1), "f16x2")
    with pytest.raises(ValueError, match="trunk_width"):
        wide.trunk_bwd_plan(_net(wide, 3, 64), "f16x2", trunk_width=192)


def test_the_other_plans_do_not_read_the_flag(wide):
    """without NSRW_FLAG_TRUNK_BWD every plan is what it was, and with it the forward's plans are too"""
    lib, C = wide.load(), wide.C
    for W in WIDTHS:
        for D in DEPTHS:
            net = _net(wide, D, W, 10, [0] if D > 2 else [])
            for base in (0, wide.FLAG_MLP_F16X2, wide.FLAG_MLP_F16X2 | wide.FLAG_TRUNK_ONCHIP,
                         wide.FLAG_MLP_F16X2 | wide.FLAG_TRUNK_ONCHIP | wide.FLAG_HEADS_ONCHIP | wide.FLAG_TRUNK_WIDE):
                a, b = wide.NsrwTrunkPlan(), wide.NsrwTrunkPlan()
                assert lib.nsrw_trunk_plan(C.byref(net), base, C.byref(a)) == 0
                assert lib.nsrw_trunk_plan(C.byref(net), base | wide.FLAG_TRUNK_BWD, C.byref(b)) == 0
                assert bytes(a) == bytes(b), (W, D, base)
                a, b = wide.NsrwHeadsPlan(), wide.NsrwHeadsPlan()
                assert lib.nsrw_heads_plan(C.byref(net), base, C.byref(a)) == 0
                assert lib.nsrw_heads_plan(C.byref(net), base | wide.FLAG_TRUNK_BWD, C.byref(b)) == 0
                assert bytes(a) == bytes(b), (W, D, base)


def test_flag_and_signature_are_declared(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert "NSRW_FLAG_TRUNK_BWD = 128" in hdr and wide.FLAG_TRUNK_BWD == 128
    assert "int nsrw_trunk_bwd_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);" in hdr
    assert "nsrw_trunk_bwd_plan" in wide.SIGNATURES and wide.TRUNK_BWDS == ("layers", "onchip")
    lib, C = wide.load(), wide.C
    plan = wide.NsrwTrunkPlan()
    net = _net(wide, 3, 100, 10, [0])
    assert lib.nsrw_trunk_bwd_plan(C.byref(net), 128 | 8, C.byref(plan)) == 0
    assert plan.onchip == 0 and (plan.nj, plan.tile_rows, plan.lds_bytes) == (0, 0, 0) and plan.reason == b"the trunk is not on chip"
    assert lib.nsrw_trunk_bwd_plan(C.byref(net), 128 | 16 | 8, C.byref(plan)) == 0
    assert (plan.onchip, plan.nj, plan.tile_rows, plan.lds_bytes) == (1, 2, 128, 102400)
    assert lib.nsrw_trunk_bwd_plan(C.byref(_net(wide, 3, 1)), 128 | 16 | 8, C.byref(plan)) == -1
    assert "netwidth" in lib.nsrw_last_error().decode()


def test_widemodel_refuses_a_trunk_bwd_it_cannot_honour(wide, monkeypatch):
    """(the arguments are judged before a device is asked for)"""
    with pytest.raises(NotImplementedError, match="trunk_bwd=\"onchip\""):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="layers", trunk_bwd="onchip")
    with pytest.raises(NotImplementedError, match="f16x2"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="bf16x3", trunk="layers", trunk_bwd="onchip")
    monkeypatch.delenv("NSR_WIDE_TRUNK", raising=False)
    with pytest.raises(NotImplementedError, match="trunk=\"onchip\""):       # the default trunk is "layers"
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk_bwd="onchip")
    for bad in ("lds", "on", 1):
        with pytest.raises(ValueError, match="trunk_bwd must be"):
            wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip", trunk_bwd=bad)
    monkeypatch.setenv("NSR_WIDE_TRUNK_BWD", "lds")
    with pytest.raises(ValueError, match="trunk_bwd must be"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip")
