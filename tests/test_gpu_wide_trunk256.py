"""GPU tests of the WIDE form of the layered renderer's on-chip trunk (kw_trunk_h2<2, false, 2> in csrc/nsr_wide_trunk.inc;
WideModel(trunk="onchip", trunk_width=256); run with -m gpu on an MI355X): networks of padded width 160 .. 256 on blocks of 64 points.
Per output element the wide form keeps the arithmetic of the per-layer GEMM -- accumulator from 0, k16 blocks ascending, the piece
products in a fixed order, one epilogue expression, the next layer's operand pieces by the same split -- so such a handle must give
the bits of a trunk="layers" handle everywhere: every tap of the forward, the network outputs on ragged point counts, the gradients
(whose kept passes run layer by layer on both), the range safety net's counters and re-runs, hostile rays, any company of rays,
under capture, and in the bounds-checked build.  No tolerance anywhere but the one check against the oracle."""
import os

import numpy as np
import pytest

from conftest import assert_close
from test_gpu_wide_tiles import _cots, _rays, cpu
from wide_onchip_cases import NARROW
from wide_onchip_cases import WIDE_NETS as NETS
from wide_onchip_cases import (bounds_checked_build, bounds_clean_and_equal, grads_equal, hostile_case, models, replay_equals_eager,
                               small_chunks, taps_equal, trunk_range_nets)
from wide_onchip_cases import hostile as _hostile
from wide_onchip_cases import scaled as _scaled
from wide_onchip_cases import wide_nets as _nets

pytestmark = pytest.mark.gpu

POINTS = (1, 63, 64, 65, 127, 128, 129, 257)        # around one and two blocks of either form, and past four


def _pair(sd_c, sd_f, ns=3, ni=2):
    """(trunk="layers" handle, trunk="onchip" handle that takes padded widths up to 256)"""
    return models(sd_c, sd_f, ns, ni, (dict(trunk="layers"), dict(trunk="onchip", trunk_width=256)))


def _range_nets(oracle, layer):
    """trunk_range_nets on the 3 x 200 network"""
    return trunk_range_nets(oracle, layer, _nets(oracle, "3x200"))


@pytest.mark.parametrize("name", sorted(NETS))
def test_wide_onchip_trunk_equals_the_per_layer_path_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past a whole number of 64-row and of 128-row blocks) and
    85, run_network on 1 .. 257 points of both networks: every tap, every network output, the rgb gradient and the gradient of all six
    outputs at the forward's z_fine are the same bits on a trunk="layers" and a trunk="onchip", trunk_width=256 handle; equal pass
    counts, no re-run.  One run_network result of the on-chip handle against the oracle, with the bound of test_gpu_wide_tiles."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    D, W, skips, views = NETS[name]
    assert wide.trunk_plan(sd_c, "f16x2")["mode"] == "layers"
    assert wide.trunk_plan(sd_c, "f16x2", "onchip", trunk_width=256) == dict(mode="onchip", nj=2, tile_rows=64, lds_bytes=159744)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ml, mo = _pair(sd_c, sd_f)
    assert (ml.trunk, ml.trunk_width, mo.trunk, mo.trunk_width) == ("layers", 128, "onchip", 256)
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        rl, rc = (m.render_rays(ro, rd, near, far, debug=True) for m in (ml, mo))
        taps_equal(rl, rc, n)
        assert np.isfinite(cpu(rc["rgb_map"])).all() and np.isfinite(cpu(rc["raw"])).all(), n
        zf = cpu(rl["z_fine"])
        cots = _cots(n, 31 + n)
        gl, gc = (m.render_rays_vjp(ro, rd, near, far, cots["rgb_map"], z_fine=zf) for m in (ml, mo))
        al, ac = (m.render_rays_vjp(ro, rd, near, far, cotangents=cots, z_fine=zf) for m in (ml, mo))
        grads_equal((gl, gc), ("rgb gradient", n))
        grads_equal((al, ac), ("gradient of all six outputs", n))
        assert np.abs(cpu(gc[0])).max() > 0
    rng = np.random.RandomState(7)
    e_net = 0.0
    for P in POINTS:
        pts = (rng.rand(P, 3).astype(np.float32) - 0.5) * 0.4
        dirs = oracle.normalize_dirs(rng.standard_normal((P, 3)).astype(np.float32))
        for net_id, sd in ((0, sd_c), (1, sd_f)):
            ol, oc = (cpu(m.run_network(pts, dirs, net_id)) for m in (ml, mo))
            assert np.array_equal(ol, oc, equal_nan=True), (P, net_id)
            assert np.isfinite(oc).all()
            if P == 257 and net_id == 0 and views:      # (the oracle's run_network takes view directions)
                want = oracle.run_network(sd, pts[:, None], dirs)[:, 0]
                e_net = np.abs(oc - want).max()
                print("%s on chip, run_network on 257 points against the oracle: %.2e" % (name, e_net))
                assert_close(oc, want, atol=5e-5 * max(1.0, float(np.abs(want).max())), rtol=5e-5, what="run_network on %d points" % P)
    sl, sc = ml.range_status(), mo.range_status()
    assert sl == sc and sc["passes"] > 0 and sc["passes_rerun"] == 0, (sl, sc)
    ml.close()
    mo.close()


def test_a_narrow_and_a_wide_network_on_one_handle(oracle):
    """Coarse 3 x 40 with fine 3 x 256 on a handle with all three switches: the narrow network runs in the heads form, the wide one
    as the wide trunk launch plus head launches; with trunk_width=128 the wide one runs per layer.  Both give the bits of
    trunk="layers".  $NSR_WIDE_TRUNK_WIDTH reaches WideModel where it can apply."""
    from neural_sim_nerf_amd import wide
    sd_c = _scaled(oracle, 511, *NARROW)
    sd_f = _nets(oracle, "3x256")[1]
    hp = lambda sd, tw: wide.heads_plan(sd, "f16x2", "onchip", "onchip", trunk_width=tw)
    assert hp(sd_c, 256)["mode"] == "onchip" and hp(sd_c, 128) == hp(sd_c, 256)
    assert hp(sd_f, 256)["mode"] == "layers" and "128" in hp(sd_f, 256)["reason"] and hp(sd_f, 128)["mode"] == "layers"
    assert wide.trunk_plan(sd_f, "f16x2", "onchip", trunk_width=256)["tile_rows"] == 64
    assert wide.trunk_plan(sd_c, "f16x2", "onchip", trunk_width=256)["tile_rows"] == 128
    kw = dict(n_samples=3, n_importance=2, mlp="f16x2")
    ml = wide.WideModel(sd_c, sd_f, trunk="layers", **kw)
    m256 = wide.WideModel(sd_c, sd_f, trunk="onchip", heads="onchip", trunk_width=256, **kw)
    m128 = wide.WideModel(sd_c, sd_f, trunk="onchip", heads="onchip", trunk_width=128, **kw)
    ro, rd = _rays(oracle, 171, 25)
    rl, r256, r128 = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, m256, m128))
    taps_equal(rl, r256)
    taps_equal(rl, r128)
    assert np.isfinite(cpu(r256["rgb_map"])).all()
    assert ml.range_status() == m256.range_status() == m128.range_status() and ml.range_status()["passes_rerun"] == 0
    for m in (ml, m256, m128):
        m.close()
    os.environ["NSR_WIDE_TRUNK_WIDTH"] = "256"
    try:
        for trunk, mlp, want in (("onchip", "f16x2", 256), ("layers", "f16x2", 128), (None, "bf16x3", 128)):
            m = wide.WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp=mlp, trunk=trunk)
            assert m.trunk_width == want, (trunk, mlp, m.trunk_width)
            m.close()
    finally:
        del os.environ["NSR_WIDE_TRUNK_WIDTH"]
    lib, C = wide.load(), wide.C
    h = C.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_TRUNK_WIDE | wide.FLAG_MLP_F16X2)
    assert lib.nsrw_create(C.byref(cfg), C.byref(h)) != 0 and not h.value
    err = lib.nsrw_last_error().decode()
    assert "NSRW_FLAG_TRUNK_WIDE" in err and "NSRW_FLAG_TRUNK_ONCHIP" in err


@pytest.mark.parametrize("layer", [1, 2])
def test_a_value_that_leaves_the_fp16_range_in_the_wide_trunk_reruns_the_pass(layer, oracle):
    """The range safety net through the wide form: 256 rays in small chunks; every coarse pass is re-run on bf16x3 (layer by layer),
    on both handles alike -- equal counters, re-runs counted, the same bits."""
    sd_c, sd_f = _range_nets(oracle, layer)
    ro, rd = _rays(oracle, 256, 26)
    with small_chunks():
        ml, mo = _pair(sd_c, sd_f)
        rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
        chunks = mo.last_kernel_ms()[1]
        sl, sc = ml.range_status(), mo.range_status()
        assert chunks > 1 and sl == sc and sc["passes"] > 0 and sc["passes_rerun"] > 0, (chunks, sl, sc)
        taps_equal(rc, rl)
        assert np.isfinite(cpu(rc["rgb_map"])).all()
        ml.close()
        mo.close()


def test_hostile_rays_through_the_wide_trunk(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 256 network: every tap and the range counters
    equal the per-layer handle's; the NaN ray stays NaN, the others' colours are finite."""
    sd_c, sd_f = _nets(oracle, "3x256")
    ro, rd = _hostile(oracle)
    rgb = hostile_case(oracle, *_pair(sd_c, sd_f), ro, rd)
    assert np.isnan(rgb[3]).all()


def test_a_rays_result_in_the_wide_trunk_depends_on_nothing_but_the_ray(oracle):
    """3 x 256 at (3, 2) samples on the on-chip handle: ray 0 alone, among 63, 64 and 200 other rays (its three coarse rows share
    a 64-point block with no, with some and with a blockful of neighbours) -- the same bits each time."""
    sd_c, sd_f = _nets(oracle, "3x256")
    ro, rd = _rays(oracle, 201, 22)
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw", "raw0")
    ml, mo = _pair(sd_c, sd_f)
    ml.close()
    alone = None
    for n in (1, 64, 65, 201):
        r = mo.render_rays(ro[:n], rd[:n], oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True)
        mine = [cpu(r[k])[0] for k in keys]
        assert np.isfinite(mine[0]).all()
        alone = alone or mine
        for k, a, b in zip(keys, alone, mine):
            assert np.array_equal(a, b, equal_nan=True), (k, n)
    assert mo.range_status()["passes_rerun"] == 0
    mo.close()


def test_the_wide_trunk_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays on the wide on-chip handle; the replay on rewritten input buffers equals the eager call."""
    sd_c, sd_f = _nets(oracle, "3x192")
    ro, rd = _rays(oracle, 171, 27)
    m, = models(sd_c, sd_f, 3, 2, (dict(trunk="onchip", trunk_width=256),))
    eager = replay_equals_eager(m, ro, rd, lambda o, d: m.render_rays(o, d, oracle.YCBV_NEAR, oracle.YCBV_FAR))
    assert np.isfinite(eager["rgb_map"]).all()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 136 and 256 on 171 rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    return [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x136", "3x256")]


def test_wide_onchip_trunk_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_trunk_h2 (tag 200000 + line).  A fresh process
    runs the two cases above on the wide on-chip handle, render_rays and run_network on 129 points; no check may trip, and every
    output equals the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_trunk256", "_bounds_runs"), dict(trunk="onchip", trunk_width=256), (None,),
                               ("render", "run_network1"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 2, 5)
    assert all(v == (False, 0, 0) for v in got[0]["release"].values()), got[0]["release"]
