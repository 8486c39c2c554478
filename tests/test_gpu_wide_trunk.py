"""GPU tests of the layered renderer's ON-CHIP trunk (kw_trunk_h2 in csrc/nsr_wide_trunk.inc; WideModel(trunk="onchip"); run with
-m gpu on an MI355X).  The trunk kernel keeps the arithmetic of the per-layer GEMM per output element -- accumulator from 0, k16
blocks ascending, the piece products in a fixed order, one epilogue expression, the next layer's operand pieces by the same split --
and only changes where the activation lives between two layers.  So a trunk="onchip" handle must give the bits of a trunk="layers"
handle everywhere: every tap of the forward, the network outputs on ragged point counts, the gradients (whose kept passes run layer
by layer while the coarse forward runs on chip), the range safety net's counters and re-runs, hostile rays, any company of rays,
under capture, and in the bounds-checked build.  No tolerance anywhere but the one check against the oracle."""
import ctypes

import numpy as np
import pytest

from test_gpu_wide_tiles import _rays, cpu
from wide_onchip_cases import TRUNK_NETS as NETS
from wide_onchip_cases import (bounds_checked_build, bounds_clean_and_equal, company_case, fine_3x136, forward_bit_for_bit, hostile_case,
                               models, range_rerun_case, replay_equals_eager, taps_equal)
from wide_onchip_cases import hostile as _hostile
from wide_onchip_cases import trunk_nets as _nets
from wide_onchip_cases import trunk_range_nets as _range_nets

pytestmark = pytest.mark.gpu


def _pair(sd_c, sd_f, ns, ni, mlp="f16x2"):
    """(trunk="layers" handle, trunk="onchip" handle) of one arithmetic"""
    return models(sd_c, sd_f, ns, ni, (dict(trunk="layers"), dict(trunk="onchip")), mlp)


def _onchip(sd_c, sd_f, ns, ni):
    return models(sd_c, sd_f, ns, ni, (dict(trunk="onchip"),))[0]


@pytest.mark.parametrize("name", sorted(NETS))
def test_onchip_trunk_equals_the_per_layer_path_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past four 128-row blocks) and 85 (255 rows), run_network
    on 1 .. 257 points of both networks: every tap, every network output, the rgb gradient and the gradient of all six outputs at
    the forward's z_fine are the same bits on a trunk="layers" and a trunk="onchip" handle; equal pass counts, no re-run."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    D, W, skips, views = NETS[name]
    assert wide.trunk_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.trunk_plan(sd_c, "f16x2")["nj"] == (1 if W <= 64 else 2)
    ml, mo = _pair(sd_c, sd_f, 3, 2)
    assert (ml.trunk, mo.trunk) == ("layers", "onchip")
    forward_bit_for_bit(oracle, (ml, mo), sd_c, sd_f, views, "%s on chip" % name)


def test_an_ineligible_network_on_an_onchip_handle_runs_per_layer_and_other_arithmetics_are_refused(oracle):
    """Coarse 3 x 40 (on chip) with fine 3 x 136 (padded width 160: layer by layer) on one handle; trunk="onchip" exists for f16x2
    only -- WideModel says so, and nsrw_create for a caller of the C interface."""
    from neural_sim_nerf_amd import wide
    sd_c = _nets(oracle, "3x40")[0]
    sd_f = fine_3x136(oracle)
    assert wide.trunk_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.trunk_plan(sd_f, "f16x2")["mode"] == "layers"
    ml, mo = _pair(sd_c, sd_f, 3, 2)
    ro, rd = _rays(oracle, 171, 25)
    rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
    taps_equal(rl, rc)
    assert np.isfinite(cpu(rc["rgb_map"])).all() and ml.range_status() == mo.range_status()
    ml.close()
    mo.close()
    for mlp in ("bf16x3", "fp32"):
        with pytest.raises(NotImplementedError, match="f16x2"):
            wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp=mlp, trunk="onchip")
    with pytest.raises(ValueError, match="trunk must be"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, trunk="lds")
    lib = wide.load()
    for flags in (wide.FLAG_TRUNK_ONCHIP, wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_BF16X3):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
        assert "NSRW_FLAG_TRUNK_ONCHIP needs NSRW_FLAG_MLP_F16X2" in lib.nsrw_last_error().decode()
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_F16X2)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    assert lib.nsrw_destroy(h) == 0


@pytest.mark.parametrize("layer", [1, 2])
def test_a_value_that_leaves_the_fp16_range_in_the_trunk_reruns_the_pass(layer, oracle):
    """The range safety net through the trunk kernel: 256 rays in 64-ray chunks; every coarse pass is re-run on bf16x3 (layer by
    layer), so the coarse taps are a bf16x3 handle's bits, and everything equals the trunk="layers" f16x2 handle's."""
    sd_c, sd_f = _range_nets(oracle, layer)
    range_rerun_case(oracle, sd_c, sd_f, lambda: _pair(sd_c, sd_f, 3, 2))


def test_hostile_rays_through_the_trunk(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 40 network: every tap and the range counters
    equal the per-layer handle's (NaN in the same places)."""
    sd_c, sd_f = _nets(oracle, "3x40")
    ro, rd = _hostile(oracle)
    hostile_case(oracle, *_pair(sd_c, sd_f, 3, 2), ro, rd)


def test_a_rays_result_on_chip_depends_on_nothing_but_the_ray(oracle):
    """3 x 128 at (5, 4) samples, 300 rays on the on-chip handle: all rays, the same rays reversed, the first 37 alone and all of
    them in 64-ray chunks give every ray the same bits (a ray's rows share a 128-point block with other neighbours each time)."""
    sd_c, sd_f = _nets(oracle, "3x128")
    company_case(oracle, _onchip(sd_c, sd_f, 5, 4))


def test_the_trunk_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays on the on-chip handle; the replay on rewritten input buffers equals the eager call."""
    sd_c, sd_f = _nets(oracle, "3x100")
    ro, rd = _rays(oracle, 171, 27)
    m = _onchip(sd_c, sd_f, 3, 2)
    eager = replay_equals_eager(m, ro, rd, lambda o, d: m.render_rays(o, d, oracle.YCBV_NEAR, oracle.YCBV_FAR))
    assert np.isfinite(eager["rgb_map"]).all()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 24, 100, 128 on 171 rays, both
    range cases and the hostile rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x100", "3x128")]
    ro6, rd6 = _rays(oracle, 256, 26)
    runs += [("range%d" % layer,) + _range_nets(oracle, layer) + (ro6, rd6) for layer in (1, 2)]
    runs.append(("hostile",) + _nets(oracle, "3x40") + _hostile(oracle))
    return runs


def test_onchip_trunk_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_trunk_h2 (tag 200000 + line).  A fresh process
    runs the cases above on the on-chip handle with a one-chunk and a 64-ray-chunk workspace; no check may trip, and every output
    equals the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_trunk", "_bounds_runs"), dict(trunk="onchip"), ("16", "0.0001"),
                               ("render", "vjp_ones", "run_network0"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 12, 7)
