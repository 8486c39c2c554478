"""Where a handle of the layered renderer computes the encodings of a network pass (NSRW_FLAG_EMBED_ONCHIP, WideModel(trunk="onchip",
embed="onchip"); trunk_rows_encode in csrc/nsr_wide_trunk.inc), restated in plain Python on wide_onchip_rules and held against
nsrw_embed_plan of the built library -- the decision nsrw_upload_network itself keeps -- and the option's resolution.  No GPU needed;
tests/test_gpu_wide_embed.py holds the kernels to kw_embed's bits."""
import os
import re

import pytest

from wide_onchip_rules import ROOT, bwd_rule, heads_rule, trunk_rule, wide      # (wide: the fixture)
from wide_onchip_rules import net as _net

WIDTHS, DEPTHS = (24, 64, 100, 128, 136, 256), (1, 2, 3)
ONCHIP = dict(mode="onchip")


def rule(D, W, multires, viewdirs, multires_views, mlp, trunk, heads, width, trunk_bwd, trunk_keep, embed, kept):
    """(positions, directions), each None = in the pass's one f16x2 launch, else why kw_embed writes them, in the library's words and
    its order of asking.  The pass's launch: unkept -- the trunk rule's (any form: 128 rows, the wide one); kept -- the kept forward's
    (trunk_keep="onchip" on a network the backward rule takes).  The positions go with the launch; the directions with a launch that
    runs the heads (the heads rule), where there are view directions at all."""
    if embed != "onchip":
        return ("NSRW_FLAG_EMBED_ONCHIP not set",) * 2
    if kept:
        launch = trunk_keep == "onchip" and bwd_rule(D, W, multires, mlp, trunk, trunk_bwd, width) is not None
        no_launch = "the kept forward is not on chip"
    else:
        launch = trunk_rule(D, W, mlp, trunk, width) is not None
        no_launch = "the trunk is not on chip"
    if not launch:
        return (no_launch,) * 2
    if not viewdirs:
        return None, "no view directions"
    if heads_rule(D, W, multires_views, viewdirs, mlp, trunk, heads) is None:
        return None, "the heads are not on chip"
    return None, None


def test_embed_plan_is_the_rule(wide):
    full = ("f16x2", "onchip", "onchip", 128, "onchip", "onchip", "onchip")
    assert rule(3, 64, 10, True, 4, *full, kept=False) == (None, None) and rule(3, 64, 10, True, 4, *full, kept=True) == (None, None)
    assert rule(3, 64, 10, False, 0, *full, kept=False) == (None, "no view directions")
    assert rule(3, 64, 10, True, 4, "f16x2", "onchip", "layers", 128, "onchip", "onchip", "onchip", False) == (None, "the heads are not on chip")
    assert rule(3, 136, 10, True, 4, *full, kept=False) == ("the trunk is not on chip",) * 2
    assert rule(3, 136, 10, True, 4, "f16x2", "onchip", "onchip", 256, "onchip", "onchip", "onchip", False) == (None, "the heads are not on chip")
    assert rule(3, 136, 10, True, 4, "f16x2", "onchip", "onchip", 256, "onchip", "onchip", "onchip", True) == ("the kept forward is not on chip",) * 2
    assert rule(1, 64, 10, True, 4, *full, kept=False) == ("the trunk is not on chip",) * 2
    assert rule(3, 64, 10, True, 4, "f16x2", "onchip", "onchip", 128, "onchip", "layers", "onchip", True) == ("the kept forward is not on chip",) * 2
    assert rule(3, 64, 10, True, 4, "bf16x3", "onchip", "onchip", 128, "onchip", "onchip", "onchip", False) == ("the trunk is not on chip",) * 2
    as_plan = lambda why: ONCHIP if why is None else dict(mode="layers", reason=why)
    on = 0
    for W in WIDTHS:
        for D in DEPTHS:
            for viewdirs in (True, False):
                net = _net(wide, D, W, 10, [0] if D > 1 else [], viewdirs)
                for mlp in wide.MLPS:
                    for trunk in wide.TRUNKS:
                        for heads in wide.HEADS:
                            for width in wide.TRUNK_WIDTHS:
                                for trunk_bwd in wide.TRUNK_BWDS:
                                    for trunk_keep in wide.TRUNK_KEEPS:
                                        for embed in wide.EMBEDS:
                                            for kept in (False, True):
                                                case = (W, D, viewdirs, mlp, trunk, heads, width, trunk_bwd, trunk_keep, embed, kept)
                                                plan = wide.embed_plan(net, mlp, trunk, heads, width, trunk_bwd, trunk_keep, embed, kept=kept)
                                                pos, dirs = rule(D, W, 10, viewdirs, 4, mlp, trunk, heads, width, trunk_bwd, trunk_keep, embed, kept)
                                                assert plan == dict(positions=as_plan(pos), directions=as_plan(dirs)), (case, plan)
                                                on += (pos is None) + (dirs is None)
    assert on > 0
    # the widest encodings fit the image the launch fills: 96 columns of positions and of directions
    wide96 = _net(wide, 3, 64, 15, [0], True, 15)
    assert wide.embed_plan(wide96, heads="onchip") == dict(positions=ONCHIP, directions=ONCHIP)
    assert wide.embed_plan(_net(wide, 3, 64, 0, [0], True, 0), heads="onchip") == dict(positions=ONCHIP, directions=ONCHIP)


def test_embed_plan_reads_state_dicts_and_refuses_bad_arguments(wide, oracle):
    sd = oracle.synth_weights_shape(1, 3, 40, 15, 2, [1], True)
    assert wide.embed_plan(sd) == dict(positions=ONCHIP, directions=dict(mode="layers", reason="the heads are not on chip"))
    assert wide.embed_plan(sd, heads="onchip") == dict(positions=ONCHIP, directions=ONCHIP)
    assert wide.embed_plan(sd, heads="onchip", kept=True)["positions"] == dict(mode="layers", reason="the kept forward is not on chip")
    assert wide.embed_plan(sd, heads="onchip", trunk_bwd="onchip", trunk_keep="onchip", kept=True) == dict(positions=ONCHIP, directions=ONCHIP)
    assert wide.embed_plan(sd, embed="layers")["positions"] == dict(mode="layers", reason="NSRW_FLAG_EMBED_ONCHIP not set")
    assert wide.embed_plan(sd, mlp="fp32")["positions"] == dict(mode="layers", reason="the trunk is not on chip")
    with pytest.raises(ValueError, match="embed must be one of"):
        wide.embed_plan(sd, embed="lds")
    from neural_sim_nerf_amd import _lib
    with pytest.raises(_lib.NsrError, match="netwidth"):
        wide.embed_plan(_net(wide, 3, 1))


def test_the_interface_is_declared_and_exported(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert re.search(r"NSRW_FLAG_EMBED_ONCHIP = \(1 << 11\)", hdr)
    assert "int32_t positions_onchip, directions_onchip;" in hdr
    assert {"nsrw_embed_plan", "nsrw_embed_status"} <= set(wide.SIGNATURES)
    lib = wide.load()
    import ctypes
    plan = wide.NsrwEmbedPlan()
    assert lib.nsrw_embed_plan(None, 0, 0, ctypes.byref(plan)) == -1 and b"null argument" in lib.nsrw_last_error()
    a = ctypes.c_ulonglong()
    assert lib.nsrw_embed_status(None, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a)) != 0
    assert b"nsrw_embed_status: null argument" in lib.nsrw_last_error()
    # the drop-in API builds its handles without the argument: the environment decides, as for the other options
    assert wide.resolve_knobs("f16x2", {"trunk": "onchip"}, {"NSR_WIDE_EMBED": "onchip"})["embed"] == "onchip"
    assert "NSR_WIDE_EMBED" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
