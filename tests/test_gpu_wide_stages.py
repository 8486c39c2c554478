"""GPU tests of the layered renderer's wave-per-ray stages (csrc/nsr_wide_stages.inc; WideModel(stages="wave"), run with -m gpu on an
MI355X).  kw_composite_wave, kw_sample_pdf_wave and kw_composite_bwd_wave do the thread-per-ray kernels' IEEE operations on the same
values in the same order -- elementwise work on lane i % 64, every ordered sum or product on one lane -- so a stages="wave" handle
must give the bits of a stages="threads" handle of the same networks: every tap, every output, every gradient, NaN in the same
places, on every arithmetic, with every option, in any company of rays, under capture and in the bounds-checked build.  No
tolerance anywhere.  tests/test_wide_stages_host.py holds the plan (LDS per ray, rays per workgroup) to its rule."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import wide_onchip_cases as cases
from test_gpu_wide_tiles import OUTS, TAPS, _cots, _rays, _same, cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# (N_samples, N_importance, rays, network): the edges of the lane map (64 samples a round) and of ATen's cascade over the
# N_samples - 2 interior weights (8 lanes x 4 partials = 32 a round) -- one weight; seven, the scalar tail only; one vector; one
# full cascade round and a left-over vector; cascade, left-over vector and tail; 64 + 128, the timed case; one past it; three lane
# rounds of coarse samples and two importance samples; coarse only
COUNTS = ((3, 2, 171, "2x32"), (9, 1, 61, "3x40"), (10, 63, 5, "2x32"), (42, 64, 61, "3x40"), (47, 65, 171, "2x32"),
          (64, 128, 61, "3x40"), (65, 129, 5, "2x32"), (130, 2, 1, "3x40"), (64, 0, 61, "2x32"), (3, 0, 171, "3x40"))
SHAPES = {"2x32": (2, 32, [], True), "3x40": (3, 40, [1], True), "3x40-noviews": (3, 40, [0], False)}


@functools.lru_cache(maxsize=None)
def _nets(oracle, name):
    """(coarse, fine) of SHAPES[name] with wide_onchip_cases.scaled's density (0.5 +- 0.25: translucent rays at any sample count)"""
    i = sorted(SHAPES).index(name)
    return tuple(cases.scaled(oracle, s + i, *SHAPES[name]) for s in (700, 800))


def _pair(sd_c, sd_f, ns, ni, mlp, **kw):
    """(the thread-per-ray handle, the wave-per-ray handle) of the same networks and options"""
    return cases.models(sd_c, sd_f, ns, ni, (dict(kw, stages="threads"), dict(kw, stages="wave")), mlp=mlp)


def _stage_launches(ni, backward_passes):
    """wave launches of ONE chunk of a call: compositing per pass and the resampling (3, or 1 coarse-only), plus the compositing
    backward of each pass that has a cotangent -- a forward 3 (1), the last pass's gradient 4 (2), the coarse pass's too 5"""
    return (3 if ni > 0 else 1) + backward_passes


def _counted(mt, mw, want):
    """the thread handle never counts; the wave handle has counted `want` more launches than at the last look"""
    assert mt.stages_status() == dict(launches_wave=0)
    now = mw.stages_status()["launches_wave"]
    assert now - getattr(mw, "_seen", 0) == want, (now, getattr(mw, "_seen", 0), want)
    mw._seen = now


def _forward(mt, mw, ro, rd, O, extras=None, chunks=1, what=None):
    rt, rw = (m.render_rays(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, debug=True, extras=extras) for m in (mt, mw))
    assert set(rt) == set(rw) and (mw.n_importance == 0 or set(TAPS) <= set(rt))
    for k in rt:                                  # every name of TAPS; coarse-only handles: their own taps
        assert _same(rt[k], rw[k]), (k, what)
    _counted(mt, mw, chunks * _stage_launches(mw.n_importance, 0))
    return rt


def _gradient(mt, mw, ro, rd, O, cots, extras=None, chunks=1, what=None, **kw):
    """cots: {output: cotangent} (nsrw_render_rays_vjp_cot) or an rgb cotangent (nsrw_render_rays_vjp); the gradients and the
    forward's outputs of the same call"""
    call = (lambda m: m.render_rays_vjp(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, cotangents=cots, extras=extras, with_forward=True, **kw)) \
        if isinstance(cots, dict) else (lambda m: m.render_rays_vjp(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, cots, extras=extras, with_forward=True, **kw))
    gt, gw = call(mt), call(mw)
    assert len(gt) == len(gw) == (4 if extras and extras.get("viewdirs") is not None else 3)
    for i in range(len(gt) - 1):                  # grad_o, grad_d[, grad_v]
        assert _same(gt[i], gw[i]), (("grad_o", "grad_d", "grad_v")[i], what)
    for k in gt[-1]:
        assert _same(gt[-1][k], gw[-1][k]), (k, what)
    passes = 1 if not isinstance(cots, dict) else (any(k in cots for k in ("rgb_map", "disp_map", "acc_map")) +
                                                   any(k in cots for k in ("rgb0", "disp0", "acc0")))
    _counted(mt, mw, chunks * _stage_launches(mw.n_importance, passes))
    return gw


def _all_cots(n, ni, seed):
    c = _cots(n, seed)
    return c if ni > 0 else {k: c[k] for k in ("rgb_map", "disp_map", "acc_map")}


def _close(*ms):
    for m in ms:
        m.close()


def test_the_workspace_is_the_same_in_both_modes(oracle):
    """carve_chunk does not know the option: a handle chunks its rays the same way in both modes (the unit of an f16x2 re-run)"""
    for name, ns, ni in (("3x40", 64, 128), ("2x32", 3, 0)):
        for mlp in ("f16x2", "fp32"):
            mt, mw = _pair(*_nets(oracle, name), ns, ni, mlp)
            for rays in (1, 64, 171, 4096):
                for grad in (0, 1, 2):
                    assert mt._need(rays, grad) == mw._need(rays, grad) > 0, (name, mlp, rays, grad)
            _counted(mt, mw, 0)
            _close(mt, mw)


@pytest.mark.parametrize("mlp", ["f16x2", "fp32", "bf16x3"])
@pytest.mark.parametrize("ns,ni,n,net", COUNTS)
def test_sample_counts_at_the_edges_of_the_lane_map_and_of_the_cascade(ns, ni, n, net, mlp, oracle):
    """forward taps on the three arithmetics; on fp32 and f16x2 (the gscale path) the gradient of every output too"""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, net)
    mt, mw = _pair(sd_c, sd_f if ni else None, ns, ni, mlp)
    for stage, s in (("composite", ns), ("composite", ns + ni), ("composite_bwd", ns + ni)) + ((("sample_pdf", ns),) if ni else ()):
        assert wide.stage_plan(stage, s, ni)["mode"] == "wave"
    ro, rd = _rays(oracle, n, 31)
    r = _forward(mt, mw, ro, rd, oracle, what=(ns, ni, n))
    assert np.isfinite(cpu(r["rgb_map"])).all() and np.isfinite(cpu(r["disp_map"])).all()
    if mlp != "bf16x3":
        g = _gradient(mt, mw, ro, rd, oracle, _all_cots(n, ni, 33), what=(ns, ni, n))
        assert np.isfinite(cpu(g[0])).all() and np.abs(cpu(g[1])).max() > 0
    assert mt.range_status() == mw.range_status() and mw.range_status()["passes_rerun"] == 0
    _close(mt, mw)


def test_the_lds_limit_one_composite_workgroup_per_two_rays(oracle):
    """(512, 512): 1024 samples a ray in the fine pass -- compositing holds two rays a workgroup, its backward and the resampling
    four, at 16 and 8 KiB a ray"""
    from neural_sim_nerf_amd import wide
    assert wide.stage_plan("composite", 1024)["rays_per_group"] == 2 and wide.stage_plan("composite_bwd", 1024)["rays_per_group"] == 4
    mt, mw = _pair(*_nets(oracle, "2x32"), 512, 512, "f16x2")
    ro, rd = _rays(oracle, 5, 35)
    r = _forward(mt, mw, ro, rd, oracle)
    assert np.isfinite(cpu(r["rgb_map"])).all()
    _gradient(mt, mw, ro, rd, oracle, _cots(5, 37))
    _close(mt, mw)


OPTIONS = ("white_bkgd", "lindisp", "bounds_and_viewdirs", "perturb", "noise", "z_fine", "noviews")


@pytest.mark.parametrize("mlp", ["f16x2", "fp32"])
@pytest.mark.parametrize("option", OPTIONS)
def test_options(option, mlp, oracle):
    """(10, 13) samples on 61 rays of the signed-density 3 x 40 networks (0 < acc < 1: acc's gradient is one; some rays are empty),
    forward -- retraw's raw arrays among the taps -- and the gradient of all six outputs, per option of render()"""
    ns, ni, n = 10, 13, 61
    O = oracle
    nets = _nets(O, "3x40-noviews") if option == "noviews" else cases.signed_nets(O, "3x40")
    kw = {option: True} if option in ("white_bkgd", "lindisp") else {}
    mt, mw = _pair(*nets, ns, ni, mlp, **kw)
    ro, rd = _rays(O, n, 41)
    rng = np.random.RandomState(43)
    extras = None
    if option == "bounds_and_viewdirs":
        extras = dict(near=(O.YCBV_NEAR * (1 + 0.2 * rng.rand(n))).astype(f32), far=(O.YCBV_FAR * (1 - 0.2 * rng.rand(n))).astype(f32),
                      viewdirs=O.normalize_dirs(rng.standard_normal((n, 3)).astype(f32)))
    elif option == "perturb":
        extras = dict(t_rand=rng.rand(n, ns).astype(f32), u=rng.rand(n, ni).astype(f32))
    elif option == "noise":
        extras = dict(noise0=rng.standard_normal((n, ns)).astype(f32), noise1=rng.standard_normal((n, ns + ni)).astype(f32))
    r = _forward(mt, mw, ro, rd, O, extras=extras, what=option)
    assert cpu(r["raw"]).shape == (n, ns + ni, 5 if option == "noviews" else 4) and np.isfinite(cpu(r["rgb_map"])).all()
    more = {}
    if option == "z_fine":                        # given depths for the fine pass: the forward's own, moved and sorted again
        z = cpu(r["z_fine"])
        more = dict(z_fine=np.sort(z + (0.01 * rng.rand(*z.shape)).astype(f32), -1).astype(f32))
    g = _gradient(mt, mw, ro, rd, O, _cots(n, 45), extras=extras, what=option, **more)
    assert np.isfinite(cpu(g[0])).any() and np.nanmax(np.abs(cpu(g[0]))) > 0
    _close(mt, mw)


@pytest.mark.parametrize("mlp", ["f16x2", "fp32"])
def test_cotangents_one_by_one_and_rgb_only(mlp, oracle):
    """the rgb-only entry (nsrw_render_rays_vjp), each cotangent alone -- a coarse one alone runs the coarse backward only -- and on a
    coarse-only handle"""
    O = oracle
    ns, ni, n = 10, 13, 61
    ro, rd = _rays(O, n, 47)
    cots = _cots(n, 49)
    mt, mw = _pair(*cases.signed_nets(O, "3x40"), ns, ni, mlp)
    _gradient(mt, mw, ro, rd, O, cots["rgb_map"], what="rgb only")
    for k in OUTS:
        _gradient(mt, mw, ro, rd, O, {k: cots[k]}, what=k)
    _gradient(mt, mw, ro, rd, O, {k: cots[k] for k in ("rgb_map", "acc0")}, what="rgb_map and acc0")
    _close(mt, mw)
    mt, mw = _pair(cases.signed_nets(O, "3x40")[0], None, ns, 0, mlp, white_bkgd=True)
    _gradient(mt, mw, ro, rd, O, cots["rgb_map"], what="coarse only, rgb")
    for k in ("disp_map", "acc_map"):
        _gradient(mt, mw, ro, rd, O, {k: cots[k]}, what=("coarse only", k))
    _close(mt, mw)


@pytest.mark.parametrize("mlp", ["f16x2", "bf16x3"])
def test_several_chunks(mlp, oracle):
    """171 rays through a 64-ray workspace: three chunks (64, 64, 43 rays: a last workgroup of three rays), the same bits as one
    chunk and as the thread handle"""
    O = oracle
    ns, ni, n = 10, 13, 171
    ro, rd = _rays(O, n, 51)
    cots = _cots(n, 53)
    mt, mw = _pair(*_nets(O, "3x40"), ns, ni, mlp)
    whole = _forward(mt, mw, ro, rd, O)
    gwhole = _gradient(mt, mw, ro, rd, O, cots)
    with cases.small_chunks():
        cut = _forward(mt, mw, ro, rd, O, chunks=3)
        assert mw.last_kernel_ms()[1] == 3
        gcut = _gradient(mt, mw, ro, rd, O, cots, chunks=3)
    cases.taps_equal(whole, cut)
    cases.grads_equal([gwhole[:2], gcut[:2]])
    _close(mt, mw)


def test_resampling_edges(oracle):
    """Per-ray u rows built on the host from the thread handle's weights0 with the oracle's sample_pdf arithmetic: u = 0, u = 1, u
    equal to cdf entries (the ties of searchsorted(right=True)) and u inside a bin whose cdf step is below 1e-5 (denom -> 1).  The
    signed-density networks alone give no such bin at any density scale tried (the oracle's render: densities of order 1 are never
    opaque at these spacings, and a ray that is opaque is so at its first sample, which is no interior weight), so the density
    noise of raw_noise_std -- an input of render() -- makes every third ray opaque at ONE interior sample and empty elsewhere (total
    = 1 + 22e-5, so the empty bins' pdf is below 1e-5) and every seventh ray empty.  The oracle says that each kind occurs and what
    inds and z_samples are; the two handles give them, and the same z_fine and z_std."""
    O = oracle
    ns, n = 24, 61
    nc = ns - 1
    ni = 2 + nc + 15
    ro, rd = _rays(O, n, 55)
    noise0 = np.zeros((n, ns), f32)
    for r in range(0, n, 3):
        noise0[r] = -1e4
        noise0[r, 2 + r % (ns - 4)] = 1e4
    noise0[::7] = -1e4
    mt, mw = _pair(*cases.signed_nets(O, "3x40"), ns, ni, "fp32")
    first = mt.render_rays(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, debug=True, extras=dict(noise0=noise0))
    w0 = cpu(first["weights0"])
    z = O.coarse_z(np.full(n, O.YCBV_NEAR, f32), np.full(n, O.YCBV_FAR, f32), n=ns)
    bins = (f32(0.5) * (z[:, 1:] + z[:, :-1])).astype(f32)
    _, _, cdf = O.sample_pdf(bins, w0[:, 1:-1], 1, u=np.zeros(1, f32))
    step = np.diff(cdf, axis=-1)
    rng = np.random.RandomState(57)
    u = rng.rand(n, ni).astype(f32)
    u[:, 0], u[:, 1] = 0.0, 1.0
    u[:, 2:2 + nc] = cdf
    tiny_rays = 0
    for r in range(n):
        js = np.nonzero(step[r] < 1e-5)[0]
        tiny_rays += len(js) > 0
        for c, j in enumerate(js[:15]):
            u[r, 2 + nc + c] = f32(0.5) * (cdf[r, j] + cdf[r, j + 1])
    want_s, want_i, _ = O.sample_pdf(bins, w0[:, 1:-1], ni, u=u)
    # each kind occurs, by the oracle
    below, above = np.maximum(want_i - 1, 0), np.minimum(want_i, nc - 1)
    c0, c1 = np.take_along_axis(cdf, below, -1), np.take_along_axis(cdf, above, -1)
    assert tiny_rays >= 15 and ((c1 - c0 < 1e-5) & (above > below) & (u > c0) & (u < c1)).any(-1).sum() >= 15      # (18 rays are made so)
    assert (c0[:, 2:2 + nc] == u[:, 2:2 + nc]).all() and (want_i[:, 2:2 + nc] >= 1 + np.arange(nc)).all()      # ties go right
    assert (want_i[:, 0] == 1).all() and (want_i[:, 1] >= nc - 1).all() and (want_i[:, 1] == nc).any()
    assert (w0.sum(-1) == 0).sum() >= n // 7 and np.isnan(cpu(first["disp0"])).sum() >= n // 7                   # empty rays
    ex = dict(noise0=noise0, u=u)
    r = _forward(mt, mw, ro, rd, O, extras=ex)
    assert np.array_equal(cpu(r["weights0"]), w0)
    for m in (mt, mw):
        got = m.render_rays(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, debug=True, extras=ex)
        assert np.array_equal(cpu(got["inds"]), want_i) and np.array_equal(cpu(got["z_samples"]), want_s)
        assert np.array_equal(cpu(got["z_fine"]), np.sort(np.concatenate([z, want_s], -1), -1))
    _close(mt, mw)


def _hostile(oracle, n=64):
    """wide_onchip_cases' hostile rays (NaN origin 3, zero direction 5, infinite direction 7) and, through the density noise, a NaN
    density (ray 9), infinite ones of either sign (10, 11) and an empty ray with acc = 0 (12)"""
    ro, rd = cases.hostile(oracle, n)
    ns, ni = 10, 13
    rng = np.random.RandomState(59)
    noise0, noise1 = (0.1 * rng.standard_normal((n, ns))).astype(f32), (0.1 * rng.standard_normal((n, ns + ni))).astype(f32)
    for noise in (noise0, noise1):
        noise[9, 4], noise[10, 5], noise[11, 2] = np.nan, np.inf, -np.inf
        noise[12] = -1e4
    return ns, ni, ro, rd, dict(noise0=noise0, noise1=noise1)


@pytest.mark.parametrize("mlp", ["f16x2", "fp32"])
def test_hostile_rays_and_company(mlp, oracle):
    """every tap and every gradient equal with NaN in the same places; and a ray's bits do not depend on its neighbours in the
    workgroup: the same ray alone (one wave of one group) and among 60 others.  The company is the hostile set without the three
    rays whose NaN / inf reach the network: on an f16x2 handle those re-run the chunk's passes on bf16x3, for every ray of the
    chunk -- the GEMMs' unit of a re-run, not the stages' doing.  The NaN and infinite densities and the empty ray stay in it; for
    the gradient on f16x2 the NaN density becomes a number, because a NaN row of dL/draw re-runs the chunk's backward likewise."""
    O = oracle
    ns, ni, ro, rd, ex = _hostile(O)
    n = len(ro)
    cots = _cots(n, 61)
    mt, mw = _pair(*cases.signed_nets(O, "3x40"), ns, ni, mlp)
    r = _forward(mt, mw, ro, rd, O, extras=ex)
    rgb, acc = cpu(r["rgb_map"]), cpu(r["acc_map"])
    ok = np.ones(n, bool)
    ok[[3, 5, 7, 9, 10, 11]] = False
    assert np.isfinite(rgb[ok]).all() and not np.isfinite(rgb[[3, 7, 9]]).any() and acc[12] == 0 and np.isnan(cpu(r["disp_map"])[12])
    g = _gradient(mt, mw, ro, rd, O, cots, extras=ex)
    assert np.isfinite(cpu(g[0])[ok]).any() and np.isnan(cpu(g[1])[12]).all()       # (acc = 0: disp's cotangent makes grad_d NaN)
    keep = np.array([i for i in range(n) if i not in (3, 5, 7)])
    assert len(keep) == 61
    ro, rd, ex, cots = ro[keep], rd[keep], {k: v[keep] for k, v in ex.items()}, {k: v[keep] for k, v in cots.items()}
    exg = ex if mlp == "fp32" else {k: np.where(np.isnan(v), f32(0.3), v) for k, v in ex.items()}
    st = mw.range_status()
    assert (st["passes_rerun"] > 0) == (mlp == "f16x2")                                   # (the two calls on the hostile set)
    r = _forward(mt, mw, ro, rd, O, extras=ex)
    g = _gradient(mt, mw, ro, rd, O, cots, extras=exg)
    for j in (0, 6, 9, 30, 60):                   # 6: the NaN density; 9: the empty ray
        one = lambda a: np.ascontiguousarray(a[j:j + 1])
        r1 = mw.render_rays(one(ro), one(rd), O.YCBV_NEAR, O.YCBV_FAR, debug=True, extras={k: one(v) for k, v in ex.items()})
        for k in TAPS:
            assert np.array_equal(cpu(r1[k]), cpu(r[k])[j:j + 1], equal_nan=True), (k, j)
        g1 = mw.render_rays_vjp(one(ro), one(rd), O.YCBV_NEAR, O.YCBV_FAR, cotangents={k: one(v) for k, v in cots.items()},
                                extras={k: one(v) for k, v in exg.items()})
        for a, b in zip(g1, g):
            assert np.array_equal(cpu(a), cpu(b)[j:j + 1], equal_nan=True), ("gradient", j)
    assert mw.range_status()["passes_rerun"] == st["passes_rerun"]                        # no company re-ran a pass
    _close(mt, mw)


ONCHIP = dict(trunk="onchip", heads="onchip", trunk_bwd="onchip", trunk_keep="onchip")


def test_with_every_onchip_form_and_through_a_rerun(oracle):
    """one f16x2 handle with the trunk, the heads, the backward trunk and the kept forward on chip and the stages per wave, against the
    same handle per thread; then with a coarse network that leaves fp16's range in every pass: the passes re-run on bf16x3 go
    through the same stage kernels, the counters and the bits are equal"""
    O = oracle
    ns, ni, n = 10, 13, 171
    ro, rd = _rays(O, n, 63)
    cots = _cots(n, 65)
    nets = cases.trunk_nets(O, "3x40")
    for sd_c, sd_f, rerun in (nets + (False,), cases._with_bias(nets, "pts_linears.1.bias") + (True,)):
        mt, mw = _pair(sd_c, sd_f, ns, ni, "f16x2", **ONCHIP)
        r = _forward(mt, mw, ro, rd, O, what=rerun)
        assert np.isfinite(cpu(r["rgb_map"])).all()
        _gradient(mt, mw, ro, rd, O, cots, what=rerun)
        st = mw.range_status()
        assert mt.range_status() == st and (st["passes_rerun"] > 0) == rerun, st
        assert mt.keep_status() == mw.keep_status() and mw.keep_status()["passes_onchip"] > 0
        _close(mt, mw)


def test_capture_and_replay(oracle):
    """one forward and one gradient call captured with torch.cuda.graph and replayed after rewriting the rays: the eager call's bits,
    which are the thread handle's"""
    import torch
    O = oracle
    ns, ni, n = 10, 13, 61
    ro, rd = _rays(O, n, 67)
    nets = _nets(O, "3x40")
    mt, mw, mw2 = cases.models(*nets, ns, ni, (dict(stages="threads"), dict(stages="wave"), dict(stages="wave")))
    cots = {k: torch.as_tensor(v, device=mw.device) for k, v in _cots(n, 69).items()}
    want = mt.render_rays(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, debug=True)
    want_g = mt.render_rays_vjp(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, cotangents=cots)
    eager = cases.replay_equals_eager(mw, ro, rd, lambda o, d: mw.render_rays(o, d, O.YCBV_NEAR, O.YCBV_FAR, debug=True))
    for k in TAPS:
        assert np.array_equal(eager[k], cpu(want[k]), equal_nan=True), k
    eager = cases.replay_equals_eager(mw2, ro, rd, lambda o, d: mw2.render_rays_vjp(o, d, O.YCBV_NEAR, O.YCBV_FAR, cotangents=cots))
    for i in (0, 1):
        assert np.array_equal(eager[i], cpu(want_g[i]), equal_nan=True) and np.abs(eager[i]).max() > 0, i
    mt.close()


# ---- the bounds-checked build: cases (47, 65) and (512, 512) and the hostile rays in a fresh process per build
BOUNDS_SCRIPT = r'''
import sys
sys.path[:0] = %r
import test_gpu_wide_stages
test_gpu_wide_stages.bounds_child(sys.argv[1])
'''


def bounds_child(out_dir):
    """(in the fresh process) wave handles on the library NSR_LIB_PATH names: the taps and the gradient of all outputs of each case
    into res.npz, and printed last {case: (built_with_checks, first_bad_line)}"""
    import nerf_oracle as O
    from neural_sim_nerf_amd.wide import WideModel
    hns, hni, hro, hrd, hex_ = _hostile(O)
    runs = (("47+65", _nets(O, "2x32"), 47, 65) + _rays(O, 171, 31) + (None,),
            ("512+512", _nets(O, "2x32"), 512, 512) + _rays(O, 5, 35) + (None,),
            ("hostile", cases.signed_nets(O, "3x40"), hns, hni, hro, hrd, hex_))
    out, res = {}, []
    for tag, nets, ns, ni, ro, rd, ex in runs:
        m = WideModel(*nets, n_samples=ns, n_importance=ni, mlp="f16x2", stages="wave")
        r = m.render_rays(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, debug=True, extras=ex)
        g = m.render_rays_vjp(ro, rd, O.YCBV_NEAR, O.YCBV_FAR, cotangents=_cots(len(ro), 71), extras=ex)
        res += [cpu(r[k]) for k in TAPS] + [cpu(x) for x in g]
        assert m.stages_status()["launches_wave"] == 3 + 5
        out[tag] = m.debug_bounds_status()
        m.close()
    np.savez(out_dir + "/res.npz", *res)
    print(out)


def test_bounds_checked_build(tmp_path):
    """libnsr_debug.so checks every data-dependent LDS and global index of the three kernels (tag 300000 + line): no violation, and
    the arrays of the release build"""
    csrc = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc")
    dbg = os.path.join(csrc, "libnsr_debug.so")
    if not os.path.exists(dbg):
        pytest.skip("libnsr_debug.so not built (make debug)")
    code = BOUNDS_SCRIPT % ([ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")],)
    res = {}
    for name, lib in (("debug", dbg), ("release", os.path.join(csrc, "libnsr.so"))):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([sys.executable, "-c", code, str(d)], env=dict(os.environ, NSR_LIB_PATH=lib), capture_output=True, text=True,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        res[name] = eval(p.stdout.strip().splitlines()[-1])
    assert res["debug"] == {k: (True, 0) for k in ("47+65", "512+512", "hostile")}, res["debug"]
    assert res["release"] == {k: (False, 0) for k in ("47+65", "512+512", "hostile")}, res["release"]
    a, b = np.load(tmp_path / "debug" / "res.npz"), np.load(tmp_path / "release" / "res.npz")
    assert len(a.files) == len(b.files) == 3 * (len(TAPS) + 2)
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
