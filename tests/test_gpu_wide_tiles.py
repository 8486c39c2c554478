"""GPU tests of EVERY tile form of the layered renderer's GEMM (gemm_split_body in csrc/nsr_wide_gemm.inc; run with -m gpu on an
MI355X).  gemm launches the body as <NJ, WM> = <4,4> <3,4> <2,4> <1,2> on a default handle and as <4,2> <2,2> <1,2> on one made
with NSRW_B3_WM=2 (128-row tiles), each with four epilogues on three arithmetics.  An output element's accumulator starts at 0 and
takes the k16 blocks in ascending order and its MFMAs in a fixed order per block, and the epilogue is one expression: nothing in
that depends on NJ, WM, the tile a row lands in, the grid or the rows that share the launch.  So the two tile heights agree BIT FOR
BIT, forward and backward, and a ray's result never depends on its company -- which is what these tests hold the kernels to, on
widths that reach every branch of the N partition (tests/test_wide_tiles_host.py restates it and guards the list).  The 128-row
handle is also held to the oracle with the bounds of test_gpu_wide.py::test_layered_renderer_on_random_network_shapes."""
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import assert_close
from test_wide_tiles_host import L_PTS, L_VIEWS, WIDTHS, forms, pad32, units

pytestmark = pytest.mark.gpu

MLPS3 = ["f16x2", "bf16x3", "fp32"]
TAPS = ("raw0", "raw", "weights0", "z_samples", "inds", "z_fine", "rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std")
OUTS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0")
POINTS = (1, 127, 128, 129, 255, 256, 257)


def cpu(t):
    return t.detach().cpu().numpy()


def _rel_rows(a, b):
    return np.linalg.norm(a - b, axis=1) / (np.linalg.norm(b, axis=1) + 1e-12)


def _same(a, b):
    return np.array_equal(cpu(a), cpu(b), equal_nan=True)


def _model(mlp, wm, *a, **k):
    """WideModel with the arithmetic and the tile height fixed: NSRW_B3_WM is read once, by nsrw_create"""
    from neural_sim_nerf_amd.wide import WideModel
    old = os.environ.pop("NSRW_B3_WM", None)
    if wm == 2:
        os.environ["NSRW_B3_WM"] = "2"
    try:
        return WideModel(*a, mlp=mlp, **k)
    finally:
        os.environ.pop("NSRW_B3_WM", None)
        if old is not None:
            os.environ["NSRW_B3_WM"] = old


@functools.lru_cache(maxsize=None)
def _rays(oracle, n, seed):
    K = oracle.scaled_K(40.0)
    pose = np.asarray(oracle.sweep_poses(1, seed=9))[0]
    ro, rd = (a.reshape(-1, 3) for a in oracle.get_rays(40, 40, K, pose[:3, :4]))
    sel = np.random.RandomState(seed).choice(len(ro), n, replace=False)
    return np.ascontiguousarray(ro[sel]), np.ascontiguousarray(rd[sel])


@functools.lru_cache(maxsize=None)
def _nets(oracle, W):
    """3 x W with view directions, one skip (after layer 0 or 1 in turn: the two-segment K path A1 | A2).  synth_weights_shape
    scales the density row by 50 * 256 / W for sample spacings of ~0.01; at 3 + 2 samples the spacing is ~0.5, a ray would be empty
    (disp = 0 / 0, a NaN gradient: NaN == NaN compares nothing) or opaque at its first sample (a zero gradient).  The row is scaled
    to an eighth of its nn.Linear size and the density bias set to +0.5: densities of 0.5 +- 0.25 on the rays used here, so every
    ray is translucent in both passes -- weights spread over its samples, finite disp and disp0, gradients through every layer.
    The last sample is dense too and its distance 1e10, so acc = 1 on every ray and the gradient of acc (and of white_bkgd's
    1 - acc) is rounding noise here: wide_onchip_cases.signed_nets is the variant on which it is a gradient."""
    i = WIDTHS.index(W)
    nets = []
    for s in (300, 400):
        sd = oracle.synth_weights_shape(s + i, 3, W, L_PTS, L_VIEWS, [i % 2], True)
        sd["alpha_linear.weight"] = (sd["alpha_linear.weight"] * np.float32(W / (400.0 * 256.0))).astype(np.float32)
        sd["alpha_linear.bias"] = np.full_like(sd["alpha_linear.bias"], 0.5)
        nets.append(sd)
    return tuple(nets)


def _cots(n, seed):
    rng = np.random.RandomState(seed)
    return {k: rng.standard_normal((n, 3) if k in ("rgb_map", "rgb0") else (n,)).astype(np.float32) for k in OUTS}


@pytest.mark.parametrize("mlp", MLPS3)
@pytest.mark.parametrize("W", WIDTHS)
def test_tile_heights_agree_bit_for_bit_and_128_row_tiles_hold_the_oracle(W, mlp, oracle):
    """3 x W at N_samples = 3, N_importance = 2 on 171 rays (513 coarse rows: one past two 256-row and four 128-row tiles) and on
    85 (255 rows), run_network on 1 .. 257 points: every forward tap, the network outputs, the rgb gradient and the gradient of all
    six outputs (kept activations, mask and accumulate epilogues, the coarse backward) equal between a default handle and an
    NSRW_B3_WM=2 one, bit for bit; the 128-row handle against the oracle stage by stage."""
    sd_c, sd_f = _nets(oracle, W)
    ns, ni = 3, 2
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    print("W %d (u = %d): default forms %s, NSRW_B3_WM=2 forms %s" % (W, units(pad32(W)), sorted(forms(W, 4)), sorted(forms(W, 2))))
    m4, m2 = (_model(mlp, wm, sd_c, sd_f, n_samples=ns, n_importance=ni) for wm in (4, 2))
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        r4, r2 = (m.render_rays(ro, rd, near, far, debug=True) for m in (m4, m2))
        for k in TAPS:
            assert _same(r4[k], r2[k]), (k, n)
        assert all(np.isfinite(cpu(r2[k])).all() for k in OUTS)               # (_nets: no empty ray, so no NaN == NaN below)
        zf = cpu(r4["z_fine"])
        cots = _cots(n, 31 + n)
        g4, g2 = (m.render_rays_vjp(ro, rd, near, far, cots["rgb_map"], z_fine=zf) for m in (m4, m2))
        a4, a2 = (m.render_rays_vjp(ro, rd, near, far, cotangents=cots, z_fine=zf) for m in (m4, m2))
        for x, y, what in ((g4, g2, "rgb gradient"), (a4, a2, "gradient of all six outputs")):
            assert _same(x[0], y[0]) and _same(x[1], y[1]), (what, n)
        assert np.isfinite(cpu(a2[0])).all() and np.isfinite(cpu(a2[1])).all() and np.abs(cpu(a2[0])).max() > 0
        assert not np.array_equal(cpu(a2[0]), cpu(g2[0]))                  # (the other five cotangents do arrive)
        if n != 171:
            continue
        # ---- the 128-row handle alone against the oracle, on its own intermediates
        vd = oracle.normalize_dirs(rd)
        z = oracle.coarse_z(np.full(n, near, np.float32), np.full(n, far, np.float32), n=ns)
        raw0 = oracle.run_network(sd_c, (ro[:, None] + rd[:, None] * z[..., None]).astype(np.float32), vd)
        k_raw0 = cpu(r2["raw0"])
        e_raw0 = np.abs(k_raw0[..., :4] - raw0[..., :4]).max()
        assert_close(k_raw0[..., :4], raw0[..., :4], atol=5e-5 * max(1.0, float(np.abs(raw0).max())), rtol=5e-5, what="coarse raw")
        rgb0, _, acc0, w0, _ = oracle.raw2outputs(k_raw0[..., :4], z, rd)
        assert_close(cpu(r2["weights0"]), w0, atol=2e-6, what="weights0 | own raw")
        assert_close(cpu(r2["rgb0"]), rgb0, atol=3e-6, what="rgb0 | own raw")
        assert_close(cpu(r2["acc0"]), acc0, atol=3e-6, what="acc0 | own raw")
        z_mid = (np.float32(0.5) * (z[:, 1:] + z[:, :-1])).astype(np.float32)
        s_, inds, _ = oracle.sample_pdf(z_mid, cpu(r2["weights0"])[:, 1:-1], ni)
        assert np.array_equal(cpu(r2["inds"]), inds) and np.array_equal(cpu(r2["z_samples"]), s_)
        assert np.array_equal(zf, np.sort(np.concatenate([z, s_], -1), -1))
        raw = oracle.run_network(sd_f, (ro[:, None] + rd[:, None] * zf[..., None]).astype(np.float32), vd)
        k_raw = cpu(r2["raw"])
        e_raw = np.abs(k_raw[..., :4] - raw[..., :4]).max()
        assert_close(k_raw[..., :4], raw[..., :4], atol=5e-5 * max(1.0, float(np.abs(raw).max())), rtol=5e-5, what="fine raw | own z")
        rgb, _, acc, _, _ = oracle.raw2outputs(k_raw[..., :4], zf, rd)
        e_rgb, e_acc = np.abs(cpu(r2["rgb_map"]) - rgb).max(), np.abs(cpu(r2["acc_map"]) - acc).max()
        assert_close(cpu(r2["rgb_map"]), rgb, atol=3e-6, what="rgb | own raw")
        assert_close(cpu(r2["acc_map"]), acc, atol=3e-6, what="acc | own raw")
        wo, wd, _ = oracle.render_rays_vjp(sd_c, sd_f, ro, rd, near, far, cots["rgb_map"], n_samples=ns, n_importance=ni, z_fine=zf)
        errs = []
        for a_, b_, what in ((cpu(g2[0]), wo, "grad_o"), (cpu(g2[1]), wd, "grad_d")):
            e = _rel_rows(a_, b_)
            nrm = np.linalg.norm(a_ - b_) / max(np.linalg.norm(b_), 1e-20)
            errs.append("%s p90 %.2e |d|/|g| %.2e" % (what, np.percentile(e, 90), nrm))
            assert np.isfinite(a_).all() and np.percentile(e, 90) < 2e-4 and nrm < 1e-2, (what, np.percentile(e, 90), e.max(), nrm)
        print("W %d %s, NSRW_B3_WM=2 against the oracle: raw0 %.2e (|raw0| <= %.1f)  raw %.2e (|raw| <= %.1f)  rgb %.2e  acc %.2e  %s"
              % (W, mlp, e_raw0, np.abs(raw0).max(), e_raw, np.abs(raw).max(), e_rgb, e_acc, "  ".join(errs)))
    # ---- run_network: ragged M of the GEMMs themselves, one row more / less than either tile height
    rng = np.random.RandomState(7)
    e_net = 0.0
    for P in POINTS:
        pts = (rng.rand(P, 3).astype(np.float32) - 0.5) * 0.4
        dirs = oracle.normalize_dirs(rng.standard_normal((P, 3)).astype(np.float32))
        for net_id, sd in ((0, sd_c), (1, sd_f)):
            o4, o2 = (cpu(m.run_network(pts, dirs, net_id)) for m in (m4, m2))
            assert np.array_equal(o4, o2, equal_nan=True), (P, net_id)
            want = oracle.run_network(sd, pts[:, None], dirs)[:, 0]
            e_net = max(e_net, np.abs(o2 - want).max())
            assert_close(o2, want, atol=5e-5 * max(1.0, float(np.abs(want).max())), rtol=5e-5, what="run_network on %d points" % P)
    print("W %d %s, NSRW_B3_WM=2 run_network on %s points against the oracle: %.2e" % (W, mlp, POINTS, e_net))
    for m in (m4, m2):
        st = m.range_status()
        assert st["passes_rerun"] == 0 and (st["passes"] > 0) == (mlp == "f16x2"), st       # f16x2: no pass was a bf16x3 re-run
        m.close()


@pytest.mark.parametrize("mlp", MLPS3)
def test_a_rays_result_depends_on_nothing_but_the_ray(mlp, oracle):
    """3 x 392 (u = 7: a 256-column tile and narrower ones) at (5, 4) samples, 300 rays, both tile heights: all rays, the same rays
    reversed, the first 37 alone, and all of them in 64-ray chunks -- every ray's outputs, raw and input gradient are the same bits
    in all four (and under both tile heights).  The fp32 and f16x2 bodies stage A differently from bf16x3, and the clamped rows of a
    ragged last M-block are computed next to other neighbours each time."""
    W, ns, ni, n = 392, 5, 4, 300
    sd_c, sd_f = _nets(oracle, W)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 22)
    cot = np.random.RandomState(23).standard_normal((n, 3)).astype(np.float32)
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw")
    per_height = []
    for wm in (4, 2):
        m = _model(mlp, wm, sd_c, sd_f, n_samples=ns, n_importance=ni)

        def run(sel):
            o, d, c = (np.ascontiguousarray(x[sel]) for x in (ro, rd, cot))
            r = m.render_rays(o, d, near, far, debug=True)
            chunks = m.last_kernel_ms()[1]
            go, gd = m.render_rays_vjp(o, d, near, far, c)
            return [cpu(r[k]) for k in keys] + [cpu(go), cpu(gd)], chunks
        whole, chunks = run(slice(None))
        assert chunks == 1 and np.isfinite(whole[0]).all() and np.isfinite(whole[5]).all() and np.abs(whole[5]).max() > 0
        rev, _ = run(slice(None, None, -1))
        few, _ = run(slice(0, 37))
        os.environ["NSR_WIDE_WORKSPACE_GB"] = "0.0001"        # the smallest workspace the library accepts: chunks of 64 rays
        try:
            cut, chunks = run(slice(None))
        finally:
            del os.environ["NSR_WIDE_WORKSPACE_GB"]
        assert chunks == (n + 63) // 64, chunks
        for k, a, b, c, d in zip(keys + ("grad_o", "grad_d"), whole, rev, few, cut):
            assert np.array_equal(a, b[::-1], equal_nan=True), (wm, k, "reversed")
            assert np.array_equal(a[:37], c, equal_nan=True), (wm, k, "the first 37 alone")
            assert np.array_equal(a, d, equal_nan=True), (wm, k, "64-ray chunks")
        st = m.range_status()
        assert st["passes_rerun"] == 0 and (st["passes"] > 0) == (mlp == "f16x2"), st
        per_height.append(whole)
        m.close()
    for k, a, b in zip(keys + ("grad_o", "grad_d"), *per_height):
        assert np.array_equal(a, b, equal_nan=True), (k, "256- vs 128-row tiles")


def test_two_coarse_samples_are_refused(oracle):
    """include/nsr_wide.h: N_samples is 3 .. NSRW_MAX_SAMPLES (sample_pdf needs one interior weight).  nsrw_create says so, and
    WideModel before it."""
    from neural_sim_nerf_amd import wide
    sd = _nets(oracle, 40)[0]
    with pytest.raises(NotImplementedError, match="N_samples must be 3"):
        wide.WideModel(sd, None, n_samples=2, n_importance=0, mlp="fp32")
    lib = wide.load()
    for bad in (2, 0, wide.MAX_SAMPLES + 1):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, bad, 0, 0)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
        assert "N_samples must be 3..%d" % wide.MAX_SAMPLES in lib.nsrw_last_error().decode()
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, 0)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    assert lib.nsrw_destroy(h) == 0
