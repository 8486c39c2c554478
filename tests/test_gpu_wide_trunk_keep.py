"""GPU tests of the layered renderer's ON-CHIP KEPT FORWARD (kw_keep_h2, kw_keep_bwd_h2, kw_mask_pack / kw_mask_unpack in
csrc/nsr_wide_trunk.inc; WideModel(trunk="onchip", trunk_bwd="onchip", trunk_keep="onchip"); run with -m gpu on an MI355X).  On such a
handle the f16x2 pass of a forward that keeps its activations for a backward is one launch -- kw_trunk_h2's arithmetic row for row --
which leaves the relu masks of the layers 0 .. D - 2 as one bit per (point, unit) and the fp32 rows the backward's head launches mask
by; the on-chip backward reads the bits.  A bf16x3 re-run stays layer by layer on fp32 activations: behind a re-run forward the bits
are packed from them, in front of a re-run backward they are unpacked into 1 / 0.  So a keep handle must give the bits of the handle
without the flag and of a trunk="layers" handle: every gradient, every forward tap, the range safety net's counters and re-runs,
hostile rays, any company of rays, under capture, and in the bounds-checked build.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from test_gpu_wide_tiles import _cots, _rays, _same, cpu
from wide_onchip_cases import EXTRA, L_PTS, RANGE_LOG2
from wide_onchip_cases import TRUNK_NETS as NETS
from wide_onchip_cases import bounds_checked_build, bounds_clean_and_equal, fine_3x136, head_range_nets, models, replay_equals_eager
from wide_onchip_cases import small_chunks, taps_equal, trunk_range_nets
from wide_onchip_cases import bwd_nets as _nets
from wide_onchip_cases import bwd_range_nets as _bwd_range_nets
from wide_onchip_cases import hostile as _hostile
from wide_onchip_cases import signed_nets as _signed_nets

pytestmark = pytest.mark.gpu

ONCHIP = dict(trunk="onchip", trunk_bwd="onchip")
KEEP = dict(ONCHIP, trunk_keep="onchip")
# (a) layer by layer; (b) trunk and backward trunk on chip, fp32 activations kept; (c) (b) with the kept forward on chip; (b') and
# (d) the same two with the heads on chip.  KEPT: which of them launch kw_keep_h2
MODES = (dict(trunk="layers"), ONCHIP, KEEP, dict(ONCHIP, heads="onchip"), dict(KEEP, heads="onchip"))
KEPT = (False, False, True, False, True)


def _handles(sd_c, sd_f, ns, ni):
    return models(sd_c, sd_f, ns, ni, MODES)


def _all_same(gs, what):
    """every handle's gradients are the last handle's bits (NaN in the same places)"""
    for h, g in enumerate(gs[:-1]):
        assert len(g) == len(gs[-1]), what
        for i in range(len(g)):
            assert _same(g[i], gs[-1][i]), (what, "handle", h, "gradient", i)


def _kept_passes(ms):
    return [m.keep_status()["passes_onchip"] for m in ms]


def _close(ms):
    for m in ms:
        m.close()


@pytest.mark.parametrize("name", sorted(NETS) + sorted(EXTRA))
def test_kept_forward_on_chip_equals_the_per_layer_chain_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past four 128-row blocks; 855 fine rows) and 85 (255 rows:
    one short of two; 425): the rgb gradient, the gradient of all six outputs at the forward's z_fine (both networks' kept forwards),
    with given view directions where the network has them, and every forward tap are the same bits on the five handles; equal pass
    counts, no re-run; the keep handles launched kept passes on chip and the others none."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    if name in NETS:
        (D, W, skips, views), L = NETS[name], L_PTS
    else:
        (D, W, skips, L), views = EXTRA[name], True
    for sd in (sd_c, sd_f):
        for heads in wide.HEADS:
            plan = wide.trunk_keep_plan(sd, "f16x2", heads=heads)
            assert plan["mode"] == "onchip" and plan["nj"] == (1 if W <= 64 else 2) and plan["tile_rows"] == 128, plan
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ms = _handles(sd_c, sd_f, 3, 2)
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
        for r in rs[:-1]:
            taps_equal(r, rs[-1], n)
        zf = cpu(rs[0]["z_fine"])
        cots = _cots(n, 31 + n)
        calls = [("rgb gradient", dict(grad_rgb=cots["rgb_map"])), ("gradient of all six outputs", dict(cotangents=cots))]
        if views:
            calls.append(("gradient of all six outputs with given view directions",
                          dict(cotangents=cots, extras=dict(viewdirs=oracle.normalize_dirs(rd)))))
        for what, kw in calls:
            gs = [m.render_rays_vjp(ro, rd, near, far, z_fine=zf, **kw) for m in ms]
            assert len(gs[-1]) == (3 if "extras" in kw else 2), what
            _all_same(gs, (what, n))
            for i, g in enumerate(gs[-1]):
                g = cpu(g)
                assert np.isfinite(g).all() and np.abs(g).max() > 0, (what, i, n)      # (so that NaN == NaN proves nothing by accident)
    st = [m.range_status() for m in ms]
    assert all(s == st[-1] for s in st) and st[-1]["passes"] > 0 and st[-1]["passes_rerun"] == 0, st
    kept = _kept_passes(ms)
    # per ray set: the fine network's kept forward in each of the gradient calls, the coarse network's second one under coarse cotangents
    want = 2 * (1 + 2 * (2 if views else 1))
    assert kept == [want if k else 0 for k in KEPT], (kept, want)
    _close(ms)
    if name != "3x40":
        return
    # once more on the signed-density variant: acc = 1 on every ray above, so the acc cotangents compared there differentiate a
    # constant; here acc and acc0 vary from ray to ray
    ms = _handles(*_signed_nets(oracle, name), 3, 2)
    ro, rd = ro_all[:171], rd_all[:171]
    rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
    for r in rs[:-1]:
        taps_equal(r, rs[-1], "signed")
    for k in ("acc_map", "acc0"):
        acc = cpu(rs[-1][k])
        assert ((acc > 0.05) & (acc < 0.95)).sum() >= 171 // 4, ("signed", k)
    zf = cpu(rs[0]["z_fine"])
    cots = _cots(171, 33)
    for what, cot in (("acc and acc0", {k: cots[k] for k in ("acc_map", "acc0")}), ("all six", cots)):
        gs = [m.render_rays_vjp(ro, rd, near, far, cotangents=cot, z_fine=zf) for m in ms]
        _all_same(gs, ("signed", what))
        for i in range(2):
            g = cpu(gs[-1][i])
            assert np.isfinite(g).any() and np.nanmax(np.abs(g)) > 0, ("signed", what, i)
            if what == "acc and acc0":
                assert np.isfinite(g).all() and (np.abs(g).max(1) > 0).sum() >= 171 // 4, ("signed", what, i)
    st = [m.range_status() for m in ms]
    assert all(s == st[-1] for s in st) and st[-1]["passes_rerun"] == 0, st
    assert _kept_passes(ms) == [4 if k else 0 for k in KEPT]
    _close(ms)


@pytest.mark.parametrize("case", ["trunk-1", "trunk-2", "feature", "views", "trunk-1-unread"])
def test_an_activation_that_leaves_the_fp16_range_in_a_kept_pass_reruns_it(case, oracle):
    """The range safety net through the kept kernel (the pack path).  N_importance = 0 handles, so that the coarse network -- the one
    whose unit 5 reaches 7e4 on every point: inside the trunk, on its last layer, in feature_linear's or in views_linears.0's output
    -- is the kept one; 256 rays in 64-ray chunks.  Every kept pass is re-run on bf16x3, layer by layer, which rewrites the fp32
    activations; the bits the on-chip backward then reads are packed from those.  Equal counters and gradient bits on all handles.
    On these four networks 7e4 saturates the density and the colours: the gradient is zero or NaN on every handle.  "trunk-1-unread" is
    trunk-1 with layer 2 reading unit 5 by zero weights: the f16x2 pass still leaves the range (and computes 0 x inf = NaN behind it,
    whose mask bits are 0), the re-run's activations are ordinary ones, and the gradient is a gradient -- equal to the per-layer
    handle's only if the bits were packed from the re-run."""
    sd_c = (trunk_range_nets(oracle, int(case[6])) if case.startswith("trunk") else head_range_nets(oracle, case))[0]
    if case == "trunk-1-unread":
        sd_c = {k: v.copy() for k, v in sd_c.items()}
        sd_c["pts_linears.2.weight"][:, 5] = 0.0
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 256, 26)
    cots = {k: v for k, v in _cots(256, 41).items() if k in ("rgb_map", "disp_map", "acc_map")}
    with small_chunks():
        ms = _handles(sd_c, None, 3, 0)
        gs = [m.render_rays_vjp(ro, rd, near, far, cotangents=cots) for m in ms]
        assert [m.last_kernel_ms()[1] for m in ms] == [4] * len(ms)
        st = [m.range_status() for m in ms]
        # per chunk one kept forward, re-run, and one backward
        assert st[0]["passes"] == 8 and 4 <= st[0]["passes_rerun"] <= 8, st[0]
        assert all(s == st[0] for s in st), st
        assert _kept_passes(ms) == [4 if k else 0 for k in KEPT]
        _all_same(gs, case)
        if case == "trunk-1-unread":
            for g in gs[-1]:
                assert np.isfinite(cpu(g)).all() and np.abs(cpu(g)).max() > 0
        _close(ms)


def test_a_gradient_that_leaves_the_fp16_range_behind_a_kept_pass_reruns_the_backward(oracle):
    """The range safety net with the forward in range (the unpack path): 256 rays in 64-ray chunks, each of which decides for itself.
    On the trunk="layers" handle the forward stays in range and the gradient call re-runs at least one pass; the re-run masks by fp32
    activations, which a keep handle first writes as 1 / 0 from its bits.  Identical counters and gradient bits on all handles."""
    sd_c, sd_f = _bwd_range_nets(oracle)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 256, 26)
    cot = _cots(256, 41)["rgb_map"]
    with small_chunks():
        ms = _handles(sd_c, sd_f, 3, 2)
        rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
        assert [m.last_kernel_ms()[1] for m in ms] == [4] * len(ms)
        after_forward = [m.range_status() for m in ms]
        assert after_forward[0]["passes"] == 8 and after_forward[0]["passes_rerun"] == 0, after_forward[0]
        zf = cpu(rs[0]["z_fine"])
        gs = [m.render_rays_vjp(ro, rd, near, far, cot, z_fine=zf) for m in ms]
        assert [m.last_kernel_ms()[1] for m in ms] == [4] * len(ms)
        st = [m.range_status() for m in ms]
        print("range event in the backward: weight 2^%d, %d of %d passes of the gradient call re-run"
              % (RANGE_LOG2, st[0]["passes_rerun"], st[0]["passes"] - 8))
        assert st[0]["passes_rerun"] >= 1, st[0]
        assert all(s == after_forward[0] for s in after_forward) and all(s == st[0] for s in st), (after_forward, st)
        assert _kept_passes(ms) == [4 if k else 0 for k in KEPT]
        for r in rs[:-1]:
            taps_equal(r, rs[-1])
        _all_same(gs, "backward range event")
        for g in gs[-1]:
            assert np.isfinite(cpu(g)).all() and np.abs(cpu(g)).max() > 0
        _close(ms)


def test_a_mixed_handle(oracle):
    """Coarse 3 x 40 (kept on chip) with fine 3 x 136 (padded width 160: layer by layer, and trunk_keep_plan says why), with all six
    cotangents and with the coarse three only: both kept forwards of one gradient call, one of each kind."""
    from neural_sim_nerf_amd import wide
    sd_c = _nets(oracle, "3x40")[0]
    sd_f = fine_3x136(oracle)
    assert wide.trunk_keep_plan(sd_c, "f16x2")["mode"] == "onchip"
    assert wide.trunk_keep_plan(sd_f, "f16x2") == dict(mode="layers", reason="the backward trunk is not on chip")
    assert wide.trunk_keep_plan(sd_f, "f16x2", trunk_width=256) == dict(mode="layers", reason="the backward trunk is not on chip")
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ms = _handles(sd_c, sd_f, 3, 2)
    ro, rd = _rays(oracle, 171, 25)
    rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
    for r in rs[:-1]:
        taps_equal(r, rs[-1])
    zf = cpu(rs[0]["z_fine"])
    cots = _cots(171, 77)
    for kw in (dict(cotangents=cots), dict(cotangents={k: cots[k] for k in ("rgb0", "disp0", "acc0")})):
        gs = [m.render_rays_vjp(ro, rd, near, far, z_fine=zf, **kw) for m in ms]
        _all_same(gs, sorted(kw["cotangents"]))
        for g in gs[-1]:
            assert np.isfinite(cpu(g)).all() and np.abs(cpu(g)).max() > 0
    st = [m.range_status() for m in ms]
    assert all(s == st[0] for s in st) and st[0]["passes_rerun"] == 0, st
    assert _kept_passes(ms) == [2 if k else 0 for k in KEPT]          # the coarse network's kept forward of either call, never the fine one's
    _close(ms)


def test_hostile_rays_through_the_kept_forward(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 40 network: the gradients have the same bits on
    all handles, NaN in the same places (a NaN activation has the mask bit 0, as NaN > 0 has); the other rays' are finite; equal range
    counters."""
    sd_c, sd_f = _nets(oracle, "3x40")
    ro, rd = _hostile(oracle)
    cots = _cots(len(ro), 43)
    ms = _handles(sd_c, sd_f, 3, 2)
    ok = np.ones(len(ro), bool)
    ok[[3, 5, 7]] = False
    for kw in (dict(grad_rgb=cots["rgb_map"]), dict(cotangents={k: cots[k] for k in ("rgb_map", "acc_map", "rgb0", "acc0")})):
        gs = [m.render_rays_vjp(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, **kw) for m in ms]
        _all_same(gs, sorted(kw))
        for g in gs[-1]:
            assert np.isfinite(cpu(g)[ok]).all() and np.abs(cpu(g)[ok]).max() > 0
    st = [m.range_status() for m in ms]
    assert all(s == st[0] for s in st), st
    assert _kept_passes(ms) == [3 if k else 0 for k in KEPT]
    _close(ms)


@pytest.mark.parametrize("heads", ["layers", "onchip"])
def test_a_rays_gradient_behind_a_kept_forward_depends_on_nothing_but_the_ray(heads, oracle):
    """3 x 128 at (5, 4) samples, 300 rays on a keep handle: all rays, the same rays reversed, the first 37 alone and all of them in
    64-ray chunks give every ray's grad_o and grad_d the same bits (a ray's rows share a 128-point block, and its mask words, with
    other neighbours each time)."""
    sd_c, sd_f = _nets(oracle, "3x128")
    n, near, far = 300, oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 22)
    cots = _cots(n, 23)
    m, = models(sd_c, sd_f, 5, 4, (dict(KEEP, heads=heads),))

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
    assert m.keep_status()["passes_onchip"] == 2 * (3 + chunks)
    m.close()


def test_the_kept_launches_are_capturable(oracle):
    """One torch.cuda.graph capture of render_rays_vjp on the keep handle with the heads on chip; the replay on rewritten input
    buffers equals the eager call."""
    import torch
    sd_c, sd_f = _nets(oracle, "3x100")
    ro, rd = _rays(oracle, 171, 27)
    m, = models(sd_c, sd_f, 3, 2, (dict(KEEP, heads="onchip"),))
    cot = torch.as_tensor(_cots(171, 29)["rgb_map"], device=m.device)
    eager = replay_equals_eager(m, ro, rd, lambda o, d: m.render_rays_vjp(o, d, oracle.YCBV_NEAR, oracle.YCBV_FAR, cot))
    assert all(np.isfinite(x).all() and np.abs(x).max() > 0 for x in eager.values())


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 24, 100, 128 and with the 96-column
    encoding on 171 rays, the two range cases (an activation of the coarse network, whose kept forward the coarse cotangents run: the
    pack path; a gradient of the fine one: the unpack path) and the hostile rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x100", "3x128", "3x40-L15")]
    runs.append(("range_forward",) + trunk_range_nets(oracle, 1) + _rays(oracle, 256, 26))
    runs.append(("range_backward",) + _bwd_range_nets(oracle) + _rays(oracle, 256, 26))
    runs.append(("hostile",) + _nets(oracle, "3x40") + _hostile(oracle))
    return runs


@pytest.mark.parametrize("heads", ["layers", "onchip"])
def test_kept_forward_in_the_bounds_checked_build(heads, tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_keep_h2, kw_keep_bwd_h2 and the two mask kernels
    (tag 200000 + line).  A fresh process runs the cases above on the keep handle with a one-chunk and a 64-ray-chunk workspace; no
    check may trip, and every output equals the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_trunk_keep", "_bounds_runs"), dict(KEEP, heads=heads), ("16", "0.0001"),
                               ("vjp_rgb", "vjp_cots"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 14, 4)
    assert {k: v[2] for k, v in got[0]["debug"].items()} == {k: v[2] for k, v in got[0]["release"].items()}


def test_nsrw_create_refuses_the_flag_without_what_it_needs():
    """NSRW_FLAG_TRUNK_KEEP without NSRW_FLAG_TRUNK_BWD, without NSRW_FLAG_TRUNK_ONCHIP and on a bf16x3 handle: nsrw_create names the
    missing flag for a caller of the C interface; with all four it makes a handle, whose counter starts at 0."""
    from neural_sim_nerf_amd import wide
    lib = wide.load()
    keep, bwd, on, f16, b3 = wide.FLAG_TRUNK_KEEP, wide.FLAG_TRUNK_BWD, wide.FLAG_TRUNK_ONCHIP, wide.FLAG_MLP_F16X2, wide.FLAG_MLP_BF16X3
    for flags, names in ((keep | on | f16, "NSRW_FLAG_TRUNK_KEEP needs NSRW_FLAG_TRUNK_BWD"), (keep | f16, "NSRW_FLAG_TRUNK_KEEP needs NSRW_FLAG_TRUNK_BWD"),
                         (keep | bwd | f16, "needs NSRW_FLAG_TRUNK_ONCHIP"), (keep | bwd | on | b3, "needs NSRW_FLAG_MLP_F16X2"),
                         (keep | bwd | on, "needs NSRW_FLAG_MLP_F16X2")):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value, flags
        assert names in lib.nsrw_last_error().decode(), (flags, lib.nsrw_last_error())
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, keep | bwd | on | f16)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    n = ctypes.c_ulonglong(7)
    assert lib.nsrw_keep_status(h, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.nsrw_destroy(h) == 0
