"""GPU tests of the layered renderer's ON-CHIP BACKWARD trunk (kw_trunk_bwd_h2 in csrc/nsr_wide_trunk.inc; WideModel(trunk="onchip",
trunk_bwd="onchip"); run with -m gpu on an MI355X).  The kernel replaces the layer loop of the gradient calls' input-gradient chain --
per pts layer the product with the transposed hidden weights under the relu mask of the kept activation, and at layer 0 and the skip
layers the product with the transposed encoding weights, summed -- by one launch with the gradient between two layers in LDS.  Per
output element it keeps the chain's arithmetic (accumulator from 0, k16 blocks ascending, the piece products in a fixed order, one
epilogue expression, the same split of the next operand, the same association of the encoding sum), and the kept forward pass it reads
is unchanged.  So a trunk_bwd="onchip" handle must give the bits of a trunk="onchip", trunk_bwd="layers" handle and of a
trunk="layers" handle: every gradient, the range safety net's counters and re-runs, hostile rays, any company of rays, under
capture, and in the bounds-checked build.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from test_gpu_wide_tiles import TAPS, _cots, _rays, _same, cpu
from wide_onchip_cases import EXTRA, L_PTS, RANGE_LOG2
from wide_onchip_cases import TRUNK_NETS as NETS
from wide_onchip_cases import bounds_checked_build, bounds_clean_and_equal, fine_3x136, models, replay_equals_eager, small_chunks, taps_equal
from wide_onchip_cases import bwd_nets as _nets
from wide_onchip_cases import bwd_range_nets as _range_nets
from wide_onchip_cases import hostile as _hostile
from wide_onchip_cases import signed_nets as _signed_nets

pytestmark = pytest.mark.gpu


def _trio(sd_c, sd_f, ns, ni):
    """(trunk="layers", trunk="onchip" with trunk_bwd="layers", trunk="onchip" with trunk_bwd="onchip") f16x2 handles"""
    return models(sd_c, sd_f, ns, ni, [dict(trunk=t, trunk_bwd=b) for t, b in (("layers", "layers"), ("onchip", "layers"), ("onchip", "onchip"))])


def _bits_equal(a, b):
    """the same bits, NaN in the same places"""
    return np.array_equal(cpu(a), cpu(b), equal_nan=True)


@pytest.mark.parametrize("name", sorted(NETS) + sorted(EXTRA))
def test_onchip_backward_trunk_equals_the_per_layer_chain_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past four 128-row blocks; 855 fine rows) and 85 (255 rows:
    one short of two; 425): the rgb gradient, the gradient of all six outputs at the forward's z_fine (both networks' backward) and
    grad_viewdirs are the same bits on the three handles, as is every forward tap; equal pass counts, no re-run."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    if name in NETS:
        (D, W, skips, views), L = NETS[name], L_PTS
    else:
        (D, W, skips, L), views = EXTRA[name], True
    want_nj = max(1 if W <= 64 else 2, 1 if 3 + 6 * L <= 64 else 2)
    for sd in (sd_c, sd_f):
        plan = wide.trunk_bwd_plan(sd, "f16x2")
        assert plan["mode"] == "onchip" and plan["nj"] == want_nj and plan["tile_rows"] == 128, plan
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ms = _trio(sd_c, sd_f, 3, 2)
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
        taps_equal(rs[0], rs[2], n)
        taps_equal(rs[1], rs[2], n)
        zf = cpu(rs[0]["z_fine"])
        cots = _cots(n, 31 + n)
        ex = dict(viewdirs=oracle.normalize_dirs(rd)) if views else None
        calls = [("rgb gradient", dict(grad_rgb=cots["rgb_map"])), ("gradient of all six outputs", dict(cotangents=cots))]
        if views:
            calls.append(("gradient of all six outputs with given view directions", dict(cotangents=cots, extras=ex)))
        for what, kw in calls:
            gs = [m.render_rays_vjp(ro, rd, near, far, z_fine=zf, **kw) for m in ms]
            assert len(gs[2]) == (3 if "extras" in kw else 2), what
            for i in range(len(gs[2])):
                assert _same(gs[0][i], gs[2][i]) and _same(gs[1][i], gs[2][i]), (what, i, n)
                g = cpu(gs[2][i])
                assert np.isfinite(g).all() and np.abs(g).max() > 0, (what, i, n)      # (so that NaN == NaN proves nothing by accident)
    st = [m.range_status() for m in ms]
    assert st[0] == st[1] == st[2] and st[2]["passes"] > 0 and st[2]["passes_rerun"] == 0, st
    for m in ms:
        m.close()
    if name != "3x40":
        return
    # once more on the signed-density variant: acc = 1 on every ray above, so the acc cotangents compared there differentiate a
    # constant; here acc and acc0 vary from ray to ray
    ms = _trio(*_signed_nets(oracle, name), 3, 2)
    ro, rd = ro_all[:171], rd_all[:171]
    rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
    taps_equal(rs[0], rs[2], "signed")
    taps_equal(rs[1], rs[2], "signed")
    for k in ("acc_map", "acc0"):
        acc = cpu(rs[2][k])
        assert ((acc > 0.05) & (acc < 0.95)).sum() >= 171 // 4, ("signed", k)
    zf = cpu(rs[0]["z_fine"])
    cots = _cots(171, 33)
    for what, cot in (("acc and acc0", {k: cots[k] for k in ("acc_map", "acc0")}), ("all six", cots)):
        gs = [m.render_rays_vjp(ro, rd, near, far, cotangents=cot, z_fine=zf) for m in ms]
        for i in range(2):
            assert _bits_equal(gs[0][i], gs[2][i]) and _bits_equal(gs[1][i], gs[2][i]), ("signed", what, i)
            g = cpu(gs[2][i])
            assert np.isfinite(g).any() and np.nanmax(np.abs(g)) > 0, ("signed", what, i)
            if what == "acc and acc0":
                assert np.isfinite(g).all() and (np.abs(g).max(1) > 0).sum() >= 171 // 4, ("signed", what, i)
    st = [m.range_status() for m in ms]
    assert st[0] == st[1] == st[2] and st[2]["passes_rerun"] == 0, st
    for m in ms:
        m.close()


def test_a_mixed_handle_and_the_refusals(oracle, monkeypatch):
    """Coarse 3 x 40 (backward on chip) with fine 3 x 136 (padded width 160: layer by layer) and coarse cotangents: both net_backward
    calls of one gradient call, one of each kind.  NSRW_FLAG_TRUNK_BWD needs NSRW_FLAG_TRUNK_ONCHIP -- nsrw_create says so for a
    caller of the C interface -- and $NSR_WIDE_TRUNK_BWD is ignored where it cannot apply, while an explicit wish raises."""
    from neural_sim_nerf_amd import wide
    sd_c = _nets(oracle, "3x40")[0]
    sd_f = fine_3x136(oracle)
    assert wide.trunk_bwd_plan(sd_c, "f16x2")["mode"] == "onchip"
    assert wide.trunk_bwd_plan(sd_f, "f16x2") == dict(mode="layers", reason="the trunk is not on chip")
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ms = _trio(sd_c, sd_f, 3, 2)
    ro, rd = _rays(oracle, 171, 25)
    rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
    assert all(_same(rs[0][k], rs[2][k]) for k in TAPS)
    zf = cpu(rs[0]["z_fine"])
    cots = _cots(171, 77)
    for kw in (dict(cotangents=cots), dict(cotangents={k: cots[k] for k in ("rgb0", "disp0", "acc0")})):
        gs = [m.render_rays_vjp(ro, rd, near, far, z_fine=zf, **kw) for m in ms]
        for i in range(2):
            assert _same(gs[0][i], gs[2][i]) and _same(gs[1][i], gs[2][i]), (sorted(kw["cotangents"]), i)
            assert np.isfinite(cpu(gs[2][i])).all() and np.abs(cpu(gs[2][i])).max() > 0
    st = [m.range_status() for m in ms]
    assert st[0] == st[1] == st[2] and st[2]["passes_rerun"] == 0, st
    for m in ms:
        m.close()
    lib = wide.load()
    for flags in (wide.FLAG_TRUNK_BWD | wide.FLAG_MLP_F16X2, wide.FLAG_TRUNK_BWD, wide.FLAG_TRUNK_BWD | wide.FLAG_MLP_BF16X3):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
        assert "NSRW_FLAG_TRUNK_BWD needs NSRW_FLAG_TRUNK_ONCHIP" in lib.nsrw_last_error().decode()
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_TRUNK_BWD | wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_BF16X3)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and "NSRW_FLAG_MLP_F16X2" in lib.nsrw_last_error().decode()
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_TRUNK_BWD | wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_F16X2)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    assert lib.nsrw_destroy(h) == 0
    # the environment's wish applies where it can ...
    monkeypatch.setenv("NSR_WIDE_TRUNK_BWD", "onchip")
    for kw, want in ((dict(mlp="f16x2", trunk="onchip"), "onchip"), (dict(mlp="f16x2", trunk="layers"), "layers"),
                     (dict(mlp="bf16x3"), "layers"), (dict(mlp="fp32"), "layers"),
                     (dict(mlp="f16x2", trunk="onchip", trunk_bwd="layers"), "layers")):
        m = wide.WideModel(sd_c, None, n_samples=3, n_importance=0, **kw)
        assert m.trunk_bwd == want, (kw, m.trunk_bwd)
        m.close()
    monkeypatch.setenv("NSR_WIDE_TRUNK", "onchip")
    m = wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2")
    assert (m.trunk, m.trunk_bwd) == ("onchip", "onchip")
    m.close()
    # ... and an explicit one that cannot be honoured raises
    monkeypatch.delenv("NSR_WIDE_TRUNK")
    monkeypatch.delenv("NSR_WIDE_TRUNK_BWD")
    for kw in (dict(mlp="f16x2", trunk="layers"), dict(mlp="f16x2"), dict(mlp="bf16x3"), dict(mlp="fp32")):
        with pytest.raises(NotImplementedError, match="trunk_bwd"):
            wide.WideModel(sd_c, None, n_samples=3, n_importance=0, trunk_bwd="onchip", **kw)
    with pytest.raises(ValueError, match="trunk_bwd must be"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip", trunk_bwd="lds")


def test_a_gradient_that_leaves_the_fp16_range_in_the_backward_trunk_reruns_the_pass(oracle):
    """The range safety net through the backward kernel: 256 rays in 64-ray chunks, each of which decides for itself.  On the
    trunk="layers" handle the forward stays in range and the gradient call re-runs at least one pass (_range_nets); the on-chip
    handles then have identical counters and identical gradient bits -- the flag rose in exactly the same passes."""
    sd_c, sd_f = _range_nets(oracle)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 256, 26)
    cot = _cots(256, 41)["rgb_map"]
    with small_chunks():
        ms = _trio(sd_c, sd_f, 3, 2)
        rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
        assert ms[0].last_kernel_ms()[1] == 4
        after_forward = [m.range_status() for m in ms]
        assert after_forward[0]["passes"] == 8 and after_forward[0]["passes_rerun"] == 0, after_forward[0]
        zf = cpu(rs[0]["z_fine"])
        gs = [m.render_rays_vjp(ro, rd, near, far, cot, z_fine=zf) for m in ms]
        st = [m.range_status() for m in ms]
        print("range event in the backward: weight 2^%d, %d of %d passes of the gradient call re-run"
              % (RANGE_LOG2, st[0]["passes_rerun"], st[0]["passes"] - 8))
        assert st[0]["passes_rerun"] >= 1, st[0]
        assert after_forward[0] == after_forward[1] == after_forward[2] and st[0] == st[1] == st[2], (after_forward, st)
        taps_equal(rs[0], rs[2])
        for i in range(2):
            assert _same(gs[0][i], gs[2][i]) and _same(gs[1][i], gs[2][i]), i
            assert np.isfinite(cpu(gs[2][i])).all() and np.abs(cpu(gs[2][i])).max() > 0
        for m in ms:
            m.close()


def test_hostile_rays_through_the_backward_trunk(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 40 network: the gradients have the same bits on
    the three handles, NaN in the same places; the other rays' are finite; equal range counters."""
    sd_c, sd_f = _nets(oracle, "3x40")
    ro, rd = _hostile(oracle)
    cots = _cots(len(ro), 43)
    ms = _trio(sd_c, sd_f, 3, 2)
    ok = np.ones(len(ro), bool)
    ok[[3, 5, 7]] = False
    for kw in (dict(grad_rgb=cots["rgb_map"]), dict(cotangents={k: cots[k] for k in ("rgb_map", "acc_map", "rgb0", "acc0")})):
        gs = [m.render_rays_vjp(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, **kw) for m in ms]
        for i in range(2):
            assert _bits_equal(gs[0][i], gs[2][i]) and _bits_equal(gs[1][i], gs[2][i]), i
            assert np.isfinite(cpu(gs[2][i])[ok]).all() and np.abs(cpu(gs[2][i])[ok]).max() > 0
    assert ms[0].range_status() == ms[1].range_status() == ms[2].range_status()
    for m in ms:
        m.close()


def test_a_rays_gradient_on_chip_depends_on_nothing_but_the_ray(oracle):
    """3 x 128 at (5, 4) samples, 300 rays on the on-chip backward handle: all rays, the same rays reversed, the first 37 alone and all
    of them in 64-ray chunks give every ray's grad_o and grad_d the same bits (a ray's rows share a 128-point block with other
    neighbours each time)."""
    sd_c, sd_f = _nets(oracle, "3x128")
    n, near, far = 300, oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 22)
    cots = _cots(n, 23)
    m, = models(sd_c, sd_f, 5, 4, (dict(trunk="onchip", trunk_bwd="onchip"),))

    def run(sel):
        o, d = (np.ascontiguousarray(x[sel]) for x in (ro, rd))
        c = {k: np.ascontiguousarray(v[sel]) for k, v in cots.items()}
        go, gd = m.render_rays_vjp(o, d, near, far, cotangents=c)
        return [cpu(go), cpu(gd)], m.last_kernel_ms()[1]
    whole, chunks = run(slice(None))
    assert chunks == 1 and all(np.isfinite(x).all() and np.abs(x).max() > 0 for x in whole)
    rev, _ = run(slice(None, None, -1))
    few, _ = run(slice(0, 37))
    with small_chunks():
        cut, chunks = run(slice(None))
    assert chunks == (n + 63) // 64, chunks
    for k, a, b, c, d in zip(("grad_o", "grad_d"), whole, rev, few, cut):
        assert np.array_equal(a, b[::-1]), (k, "reversed")
        assert np.array_equal(a[:37], c), (k, "the first 37 alone")
        assert np.array_equal(a, d), (k, "64-ray chunks")
    assert m.range_status()["passes_rerun"] == 0
    m.close()


def test_the_backward_trunk_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays_vjp on the on-chip backward handle; the replay on rewritten input buffers equals the
    eager call."""
    import torch
    sd_c, sd_f = _nets(oracle, "3x100")
    ro, rd = _rays(oracle, 171, 27)
    m, = models(sd_c, sd_f, 3, 2, (dict(trunk="onchip", trunk_bwd="onchip"),))
    cot = torch.as_tensor(_cots(171, 29)["rgb_map"], device=m.device)
    eager = replay_equals_eager(m, ro, rd, lambda o, d: m.render_rays_vjp(o, d, oracle.YCBV_NEAR, oracle.YCBV_FAR, cot))
    assert all(np.isfinite(x).all() and np.abs(x).max() > 0 for x in eager.values())


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 24, 100, 128 and with the 96-column
    encoding on 171 rays, the range case and the hostile rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x100", "3x128", "3x40-L15")]
    runs.append(("range",) + _range_nets(oracle) + _rays(oracle, 256, 26))
    runs.append(("hostile",) + _nets(oracle, "3x40") + _hostile(oracle))
    return runs


def test_onchip_backward_trunk_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_trunk_bwd_h2 (tag 200000 + line).  A fresh process
    runs the cases above on the on-chip backward handle with a one-chunk and a 64-ray-chunk workspace; no check may trip, and every
    output equals the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_trunk_bwd", "_bounds_runs"), dict(trunk="onchip", trunk_bwd="onchip"),
                               ("16", "0.0001"), ("vjp_rgb", "vjp_cots"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 12, 4)
    assert {k: v[2] for k, v in got[0]["debug"].items()} == {k: v[2] for k, v in got[0]["release"].items()}
