"""GPU tests of the layered renderer's ON-CHIP heads (the heads form of kw_trunk_h2 in csrc/nsr_wide_trunk.inc;
WideModel(trunk="onchip", heads="onchip"); run with -m gpu on an MI355X).  Behind the on-chip trunk the same workgroup runs
alpha_linear, feature_linear, views_linears.0 and rgb_linear (or output_linear) on its 128 rows with the arithmetic of the per-layer
GEMM per output element, and only the raw outputs reach memory.  So a heads="onchip" handle must give the bits of a trunk="layers"
handle, and of a trunk="onchip", heads="layers" handle, everywhere: every tap of the forward, the network outputs on ragged point
counts, the gradients (whose kept passes run layer by layer), the range safety net's counters and re-runs for values that leave
fp16's range in each head, hostile rays, any company of rays, under capture, and in the bounds-checked build.  No tolerance anywhere
but the one check against the oracle."""
import ctypes
import os

import numpy as np
import pytest

from test_gpu_wide_tiles import _rays, cpu
from wide_onchip_cases import HEADS_NETS as NETS
from wide_onchip_cases import (bounds_checked_build, bounds_clean_and_equal, company_case, fine_3x136, forward_bit_for_bit, hostile_case,
                               models, range_rerun_case, replay_equals_eager, taps_equal)
from wide_onchip_cases import head_range_nets as _head_range_nets
from wide_onchip_cases import heads_nets as _nets
from wide_onchip_cases import hostile as _hostile
from wide_onchip_cases import trunk_nets as _trunk_nets

pytestmark = pytest.mark.gpu

MODES = (("layers", "layers"), ("onchip", "layers"), ("onchip", "onchip"))       # (trunk, heads): the last is the one under test


def _models(sd_c, sd_f, ns, ni, modes=MODES):
    return models(sd_c, sd_f, ns, ni, [dict(trunk=t, heads=h) for t, h in modes])


@pytest.mark.parametrize("name", sorted(NETS))
def test_onchip_heads_equal_the_per_layer_path_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past four 128-row blocks) and 85 (255 rows), run_network
    on 1 .. 257 points of both networks: every tap, every network output, the rgb gradient and the gradient of all six outputs at
    the forward's z_fine are the same bits on the three handles; equal pass counts, no re-run."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    D, W, skips, Lv, _, _ = NETS[name]
    views = Lv is not None
    assert wide.heads_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.heads_plan(sd_f, "f16x2")["mode"] == "onchip"
    forward_bit_for_bit(oracle, _models(sd_c, sd_f, 3, 2), sd_c, sd_f, views, "%s heads on chip" % name)


@pytest.mark.parametrize("case", ["feature", "views", "trunk"])
def test_a_value_that_leaves_the_fp16_range_in_the_heads_reruns_the_pass(case, oracle):
    """The range safety net through the heads: 256 rays in 64-ray chunks; every coarse pass is re-run on bf16x3 (layer by layer), so
    the coarse taps are a bf16x3 handle's bits, and everything equals the trunk="layers" f16x2 handle's."""
    sd_c, sd_f = _head_range_nets(oracle, case)
    range_rerun_case(oracle, sd_c, sd_f, lambda: _models(sd_c, sd_f, 3, 2, (MODES[0], MODES[2])))


def test_hostile_rays_through_the_heads(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 40 network: every tap and the range counters
    equal the per-layer handle's (NaN in the same places)."""
    sd_c, sd_f = _trunk_nets(oracle, "3x40")
    ro, rd = _hostile(oracle)
    hostile_case(oracle, *_models(sd_c, sd_f, 3, 2, (MODES[0], MODES[2])), ro, rd)


def test_a_rays_result_with_onchip_heads_depends_on_nothing_but_the_ray(oracle):
    """3 x 128 at (5, 4) samples, 300 rays on the heads="onchip" handle: all rays, the same rays reversed, the first 37 alone and all
    of them in 64-ray chunks give every ray the same bits (a ray's rows share a 128-point block with other neighbours each time)."""
    sd_c, sd_f = _trunk_nets(oracle, "3x128")
    company_case(oracle, _models(sd_c, sd_f, 5, 4, (MODES[2],))[0])


def test_the_heads_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays on the heads="onchip" handle; the replay on rewritten input buffers equals the
    eager call."""
    sd_c, sd_f = _trunk_nets(oracle, "3x100")
    ro, rd = _rays(oracle, 171, 27)
    m, = _models(sd_c, sd_f, 3, 2, (MODES[2],))
    eager = replay_equals_eager(m, ro, rd, lambda o, d: m.render_rays(o, d, oracle.YCBV_NEAR, oracle.YCBV_FAR))
    assert np.isfinite(eager["rgb_map"]).all()


def test_heads_onchip_is_refused_without_the_onchip_trunk_and_an_ineligible_network_runs_per_layer(oracle):
    """heads="onchip" needs trunk="onchip" on an f16x2 handle -- WideModel says so, and nsrw_create for a caller of the C interface.
    Coarse 3 x 40 (on chip, heads too) with fine 3 x 136 (padded width 160: layer by layer, heads too) on one handle."""
    from neural_sim_nerf_amd import wide
    sd_c = _trunk_nets(oracle, "3x40")[0]
    with pytest.raises(NotImplementedError, match="trunk=\"onchip\""):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="layers", heads="onchip")
    for mlp in ("bf16x3", "fp32"):
        with pytest.raises(NotImplementedError):
            wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp=mlp, heads="onchip")
    with pytest.raises(ValueError, match="heads must be"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, trunk="onchip", heads="lds")
    lib = wide.load()
    for flags in (wide.FLAG_HEADS_ONCHIP | wide.FLAG_MLP_F16X2, wide.FLAG_HEADS_ONCHIP):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
        msg = lib.nsrw_last_error().decode()
        assert "NSRW_FLAG_HEADS_ONCHIP" in msg and "NSRW_FLAG_TRUNK_ONCHIP" in msg, msg
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_HEADS_ONCHIP | wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_F16X2)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    assert lib.nsrw_destroy(h) == 0
    # the environment's wish applies where it can
    os.environ["NSR_WIDE_HEADS"] = "onchip"
    try:
        m = wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip")
        assert m.heads == "onchip"
        m.close()
        for kw in (dict(mlp="f16x2"), dict(mlp="bf16x3"), dict(mlp="fp32")):
            m = wide.WideModel(sd_c, None, n_samples=3, n_importance=0, **kw)
            assert m.heads == "layers" and m.trunk == "layers"
            m.close()
    finally:
        del os.environ["NSR_WIDE_HEADS"]
    sd_f = fine_3x136(oracle)
    assert wide.heads_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.heads_plan(sd_f, "f16x2")["mode"] == "layers"
    ml, mh = _models(sd_c, sd_f, 3, 2, (MODES[0], MODES[2]))
    ro, rd = _rays(oracle, 171, 25)
    rl, rh = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mh))
    taps_equal(rl, rh)
    assert np.isfinite(cpu(rh["rgb_map"])).all() and ml.range_status() == mh.range_status()
    ml.close()
    mh.close()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 24, 66, 128 on 171 rays, the
    three range cases and the hostile rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x66-v6", "3x128-v4")]
    ro6, rd6 = _rays(oracle, 256, 26)
    runs += [("range-" + case,) + _head_range_nets(oracle, case) + (ro6, rd6) for case in ("feature", "views", "trunk")]
    runs.append(("hostile",) + _trunk_nets(oracle, "3x40") + _hostile(oracle))
    return runs


def test_onchip_heads_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_trunk_h2 (tag 200000 + line).  A fresh process
    runs the cases above on the heads="onchip" handle with a one-chunk and a 64-ray-chunk workspace; no check may trip, and every
    output equals the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_heads", "_bounds_runs"), dict(trunk="onchip", heads="onchip"), ("16", "0.0001"),
                               ("render", "vjp_ones", "run_network0"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 14, 7)
