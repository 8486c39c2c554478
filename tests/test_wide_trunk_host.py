"""Which networks the layered renderer's on-chip trunk (kw_trunk_h2 in csrc/nsr_wide_trunk.inc) takes, restated in plain Python and
held against nsrw_trunk_plan of the built library -- the function nsrw_upload_network itself consults.  No GPU needed."""
import os

import pytest

from wide_onchip_rules import LDS_LIMIT, ROOT, pad32, wide      # (wide: the fixture)
from wide_onchip_rules import net as _net
from wide_onchip_rules import trunk_lds as lds_bytes
from wide_onchip_rules import trunk_nj as rule


def test_trunk_plan_is_the_rule(wide):
    assert [rule(3, W, "f16x2", "onchip") for W in (24, 40, 64, 100, 128, 129, 136, 256)] == [1, 1, 1, 2, 2, None, None, None]
    assert rule(1, 64, "f16x2", "onchip") is None and rule(8, 64, "bf16x3", "onchip") is None and rule(8, 64, "f16x2", "layers") is None
    for W in (2, 24, 32, 33, 40, 64, 65, 96, 100, 128, 129, 136, 160, 256, 1024):
        for D in (1, 2, 3, 8, 64):
            for mlp in wide.MLPS:
                for trunk in wide.TRUNKS:
                    for multires in (0, 4, 10, 15):
                        skips = [s for s in (0, 4) if s < D - 1]
                        plan = wide.trunk_plan(_net(wide, D, W, multires, skips), mlp, trunk)
                        want = rule(D, W, mlp, trunk)
                        case = (W, D, mlp, trunk, multires)
                        if want is None:
                            assert plan["mode"] == "layers" and plan["reason"], case
                        else:
                            assert plan == dict(mode="onchip", nj=want, tile_rows=128, lds_bytes=lds_bytes(want)), (case, plan)
                            assert plan["lds_bytes"] <= LDS_LIMIT == 163840, case
    # the cases the issue names, one by one
    on = lambda W, D=3, mlp="f16x2", L=10: wide.trunk_plan(_net(wide, D, W, L, [0]), mlp)
    assert [on(W)["nj"] for W in (24, 40, 64)] == [1, 1, 1] and [on(W)["nj"] for W in (100, 128)] == [2, 2]
    assert all(on(W)["mode"] == "layers" for W in (129, 136, 256))
    assert wide.trunk_plan(_net(wide, 1, 64), "f16x2")["mode"] == "layers"
    assert on(64, mlp="bf16x3")["mode"] == "layers" and on(64, mlp="fp32")["mode"] == "layers"
    assert on(128, L=15)["lds_bytes"] <= LDS_LIMIT and pad32(3 + 6 * 15) == 96        # multires = 15: the widest encoding there is
    assert wide.trunk_plan(_net(wide, 3, 64), "f16x2", trunk="layers")["mode"] == "layers"


def test_trunk_plan_reads_state_dicts_and_refuses_invalid_networks(wide, oracle):
    sd = oracle.synth_weights_shape(1, 3, 40, 4, 2, [1], True)
    assert wide.trunk_plan(sd, "f16x2") == dict(mode="onchip", nj=1, tile_rows=128, lds_bytes=lds_bytes(1))
    assert wide.trunk_plan(oracle.synth_weights_shape(1, 3, 136, 4, 2, [1], True), "f16x2")["mode"] == "layers"
    assert wide.trunk_plan(oracle.synth_weights_shape(1, 3, 40, 4, 2, [0], False), "f16x2")["nj"] == 1
    from neural_sim_nerf_amd import _lib
    with pytest.raises(_lib.NsrError, match="netwidth"):
        wide.trunk_plan(_net(wide, 3, 1), "f16x2")


def test_the_plans_lds_bytes_are_those_of_the_kernel_they_select(wide):
    """Every on-chip form: the lds_bytes a plan reports equals the LDS the kernel it selects has in the built library -- the code
    object's group_segment_fixed_size (tools/kernel_resources.py).  The kernel is named by the plan's own figures: kw_trunk_h2<nj,
    heads, tile_rows / 32> and kw_trunk_bwd_h2<nj>; the seven named here are all the library instantiates."""
    import sys
    lib = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(lib)[0]
    seen = {}
    for W, width, L in ((40, 128, 4), (128, 128, 4), (256, 256, 4), (40, 128, 15)):      # NJ = 1, 2; the wide form; NJ = 2 by the encoding
        n = _net(wide, 3, W, L, [0])
        trunk = wide.trunk_plan(n, "f16x2", "onchip", trunk_width=width)
        plans = [("kw_trunk_h2<%d, 0, %d>" % (trunk["nj"], trunk["tile_rows"] // 32), trunk)]
        heads = wide.heads_plan(n, "f16x2", "onchip", "onchip", trunk_width=width)
        bwd = wide.trunk_bwd_plan(n, "f16x2", "onchip", "onchip", trunk_width=width)
        assert (heads["mode"], bwd["mode"]) == (("onchip", "onchip") if width == 128 else ("layers", "layers")), (W, heads, bwd)
        if width == 128:
            plans += [("kw_trunk_h2<%d, 1, 4>" % trunk["nj"], heads), ("kw_trunk_bwd_h2<%d>" % bwd["nj"], bwd)]
        for kernel, plan in plans:
            assert plan["lds_bytes"] == res[kernel]["group_segment_fixed_size"], (W, L, kernel, plan, res[kernel])
            seen[kernel] = plan["lds_bytes"]
    assert seen == {"kw_trunk_h2<1, 0, 4>": 106496, "kw_trunk_h2<2, 0, 4>": 155648, "kw_trunk_h2<1, 1, 4>": 106496,
                    "kw_trunk_h2<2, 1, 4>": 155648, "kw_trunk_h2<2, 0, 2>": 159744, "kw_trunk_bwd_h2<1>": 53248,
                    "kw_trunk_bwd_h2<2>": 102400}, seen
    assert sorted(seen) == sorted(k for k in res if k.startswith("kw_trunk")), sorted(res)


def test_flag_and_signature_are_declared(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert "NSRW_FLAG_TRUNK_ONCHIP = 16" in hdr and wide.FLAG_TRUNK_ONCHIP == 16
    assert "int nsrw_trunk_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);" in hdr
    assert "200000 + the line" in hdr
