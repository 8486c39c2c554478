"""The row-granular re-run of the layered renderer's f16x2 passes (WideModel(rerun="rows"), NSRW_FLAG_RERUN_ROWS; DESIGN.md 8
"Row-granular re-run") on the GPU.  The contract: every point of every pass is computed either by the f16x2 chain or by the bf16x3
chain, and which one depends on that point's own values only -- so a ray's bits depend on that ray only.  Every comparison here is
bit for bit with NaN in the same places; there is no tolerance.

These tests fail without the feature (the keyword does not exist).  The cases "layer-0 overflow on chosen rays", "inner-layer
overflow only", "company" and "the neighbour test" fail on a rerun="pass" handle as well: there one flagged ray gives every ray of
its chunk bf16x3's bits, so the clean rays do not keep the bits of their own f16x2 render."""
import os

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_wide_tiles import TAPS, _cots, _model, _rays, cpu
from test_oracle_golden import wide_case
from wide_onchip_cases import L_PTS, RANGE_LOG2, bounds_checked_build, bounds_clean_and_equal, bwd_range_nets, grads_equal, models
from wide_onchip_cases import small_chunks, taps_equal, trunk_nets, trunk_range_nets

pytestmark = pytest.mark.gpu

NS, NI = 3, 2
N2 = 257                                    # rays of the chosen-rays cases: 771 coarse rows, 1285 fine ones
FLAGGED = np.zeros(N2, bool)
FLAGGED[[0, 256]] = True
FLAGGED[85:171] = True                      # ray 85's coarse rows 255 .. 257 straddle a tile edge; rows 256 .. 511 -- one whole 256-row tile -- are flagged
FP16_MAX = 65504.0


def rows_of(flagged, samples):
    """the rows (points) of the flagged rays of a pass with `samples` samples per ray, as row bits"""
    rows = np.repeat(np.asarray(flagged, bool), samples)
    return np.packbits(np.pad(rows, (0, (-len(rows)) % 32)), bitorder="little").view(np.uint32)


def some_tile_is_clean(flagged, tile):
    """whether some tile block of `tile` rows of the coarse or of the fine pass holds no flagged ray's row"""
    from neural_sim_nerf_amd import wide
    for s in (NS, NS + NI):
        M = len(flagged) * s
        if len(wide.rerun_rows_plan(rows_of(flagged, s), M, tile)) < (M + tile - 1) // tile:
            return True
    return False


def rays_with_offset(oracle, flagged, offset, seed=31):
    ro, rd = (x.copy() for x in _rays(oracle, len(flagged), seed))
    ro[flagged, 0] += np.float32(offset)
    return ro, rd


def coarse_points(oracle, ro, rd):
    """the coarse pass's points (RN:439-444, 463): near (1 - t) + far t at t = linspace(0, 1, N_samples)"""
    t = np.linspace(0.0, 1.0, NS, dtype=np.float32)
    z = np.float32(oracle.YCBV_NEAR) * (1 - t) + np.float32(oracle.YCBV_FAR) * t
    return (ro[:, None] + rd[:, None] * z[None, :, None]).astype(np.float32)


def rays_taps_equal(ra, ia, rb, ib, what):
    """the taps of the rays ia of one render and of the rays ib of another: the same bits, NaN in the same places"""
    for k in TAPS:
        assert np.array_equal(cpu(ra[k])[ia], cpu(rb[k])[ib], equal_nan=True), (k, what)


def chosen_rays_case(oracle, nets, ro, rd, flagged, make_rows, what):
    """The expectations of the chosen-rays cases on the rows handle make_rows(): a clean f16x2 render of the other rays alone re-runs
    nothing; the flagged rays' taps are a bf16x3 handle's for those rays; every other ray's taps are those of that clean render;
    rows_rerun is the flagged rays' point count, coarse plus fine, and rows every point."""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    f, c = np.nonzero(flagged)[0], np.nonzero(~flagged)[0]
    plain, b3 = models(nets[0], nets[1], NS, NI, (dict(rerun="pass"),))[0], models(nets[0], nets[1], NS, NI, ({},), mlp="bf16x3")[0]
    clean = plain.render_rays(ro[c], rd[c], near, far, debug=True)
    assert plain.range_status()["passes_rerun"] == 0, plain.range_status()
    want_f = b3.render_rays(ro[f], rd[f], near, far, debug=True)
    m = make_rows()
    assert m.rerun == "rows"
    got = m.render_rays(ro, rd, near, far, debug=True)
    st = m.range_status()
    print(what, st, "chunks", m.last_kernel_ms()[1])
    rays_taps_equal(got, f, want_f, slice(None), (what, "flagged rays against bf16x3"))
    rays_taps_equal(got, c, clean, slice(None), (what, "the other rays against their own f16x2 render"))
    assert st["rows"] == len(ro) * (2 * NS + NI) and st["rows_rerun"] == len(f) * (2 * NS + NI), st
    assert st["passes_rerun"] >= 1 and st["passes"] == 2 * m.last_kernel_ms()[1], st
    for x in (plain, b3, m):
        x.close()
    return got


def test_nothing_overflows(oracle):
    """clean rays: a rows handle equals a "pass" handle in every tap and gradient, re-runs nothing, and counts every point"""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    sd_c, sd_f = trunk_nets(oracle, "3x100")
    ro, rd = _rays(oracle, 171, 21)
    ms = models(sd_c, sd_f, NS, NI, (dict(rerun="pass"), dict(rerun="rows"), dict(rerun="rows", stages="wave")))
    rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
    for r in rs[1:]:
        taps_equal(rs[0], r)
    cots = _cots(171, 33)
    zf = cpu(rs[0]["z_fine"])
    grads_equal([m.render_rays_vjp(ro, rd, near, far, cots["rgb_map"]) for m in ms], "rgb gradient")
    grads_equal([m.render_rays_vjp(ro, rd, near, far, cotangents=cots, z_fine=zf) for m in ms], "gradient of all six outputs")
    st = [m.range_status() for m in ms]
    # render: coarse + fine; vjp: coarse, fine (kept), the fine backward; vjp with coarse cotangents: those three, the coarse forward again, its backward
    rows = 171 * ((NS + NS + NI) + (NS + 2 * (NS + NI)) + (NS + 2 * (NS + NI) + 2 * NS))
    assert st[0]["rows"] == 0 and st[0]["rows_rerun"] == 0 and st[0]["passes_rerun"] == 0, st
    for s in st[1:]:
        assert s["passes"] == st[0]["passes"] == 10 and s["passes_rerun"] == 0 and s["rows_rerun"] == 0 and s["rows"] == rows, (s, rows)
    for m in ms:
        m.close()


def test_workspace_grows_with_the_flag_only(oracle):
    """nsrw_workspace_bytes of a handle without the flag is what the flags that existed before give (the per-ray stages' flag changes
    no workspace), for every gradient mode; with the flag it grows by the row bits and the two lists of a chunk's points, one
    256-byte-aligned region"""
    sd_c, sd_f = trunk_nets(oracle, "3x100")
    old, base, rows = models(sd_c, sd_f, NS, NI, (dict(stages="wave"), dict(rerun="pass"), dict(rerun="rows")))
    for rays in (1, 64, 65, 257, 4096, 100000):
        for grad in (0, 1, 2):
            R = (rays + 63) // 64 * 64
            P = R * (NS + NI)
            extra = 4 * ((P + 31) // 32 + 2 + (P + 127) // 128 + (P + 255) // 256)
            assert base._need(rays, grad) == old._need(rays, grad), (rays, grad)
            assert rows._need(rays, grad) == base._need(rays, grad) + (extra + 255) // 256 * 256, (rays, grad)
    for m in (old, base, rows):
        m.close()


@pytest.mark.parametrize("variant", ["one chunk", "64-ray chunks", "128-row tiles", "wave stages"])
def test_layer0_overflow_on_chosen_rays(oracle, variant):
    """257 rays at (3, 2) samples: 771 coarse rows and 1285 fine ones, neither a multiple of 32, several 256-row tiles.  The rays 0,
    85 .. 170 and 256 get a finite origin offset of 7e4 in x, so the encoding's identity column flags their points at layer 0, in
    both passes.  (Fails on a rerun="pass" handle too: there every ray of the call has bf16x3's bits.)"""
    nets = trunk_nets(oracle, "3x100")
    ro, rd = rays_with_offset(oracle, FLAGGED, 7.0e4)
    big = np.abs(coarse_points(oracle, ro, rd)).max(axis=(1, 2)) >= FP16_MAX
    assert np.array_equal(big, FLAGGED) and np.isfinite(ro).all()                   # exactly the chosen rays leave the range
    assert np.abs(rd).max() * oracle.YCBV_FAR < 100.0                                # ... at any depth: the fine pass's points too
    assert FLAGGED[85] and not FLAGGED[84] and 85 * NS == 255                      # ray 85's rows 255 .. 257 straddle a tile edge
    assert some_tile_is_clean(FLAGGED, 256) and some_tile_is_clean(FLAGGED, 128)
    make = lambda **kw: models(nets[0], nets[1], NS, NI, (dict(rerun="rows", **kw),))[0]
    if variant == "one chunk":
        got = chosen_rays_case(oracle, nets, ro, rd, FLAGGED, make, variant)
        pts = ro[:, None] + rd[:, None] * cpu(got["z_fine"])[..., None]
        assert np.array_equal(np.abs(pts).max(axis=(1, 2)) >= FP16_MAX, FLAGGED)
    elif variant == "64-ray chunks":
        with small_chunks():
            chosen_rays_case(oracle, nets, ro, rd, FLAGGED, make, variant)
    elif variant == "128-row tiles":
        chosen_rays_case(oracle, nets, ro, rd, FLAGGED, lambda: _model("f16x2", 2, nets[0], nets[1], n_samples=NS, n_importance=NI, rerun="rows"), variant)
    else:
        chosen_rays_case(oracle, nets, ro, rd, FLAGGED, lambda: make(stages="wave"), variant)


def inner_nets(oracle):
    """3 x 100 in which hidden unit 5 of layer 0 reads x with the weight 8, in both networks: at x = 3e4 -- inside fp16's range, so
    layer 0's GEMM flags nothing -- it is 2.4e5, which layer 1's GEMM meets when it splits its input"""
    nets = []
    for sd in trunk_nets(oracle, "3x100"):
        sd = {k: v.copy() for k, v in sd.items()}
        sd["pts_linears.0.weight"][5, 0] = np.float32(8.0)
        nets.append(sd)
    return tuple(nets)


def layer0_f64(sd, pts):
    """float64 numpy forward of pts_linears.0 on the encoding (RH:39-48: x, then per band sin and cos of 2^l x)"""
    x = pts.reshape(-1, 3).astype(np.float64)
    cols = [x]
    for l in range(L_PTS):
        cols += [np.sin(x * 2.0 ** l), np.cos(x * 2.0 ** l)]
    e = np.concatenate(cols, axis=1)
    h = e @ sd["pts_linears.0.weight"].astype(np.float64).T + sd["pts_linears.0.bias"].astype(np.float64)
    return np.maximum(h, 0.0).reshape(pts.shape[:-1] + (-1,))


@pytest.mark.parametrize("variant", ["one chunk", "64-ray chunks"])
def test_inner_layer_overflow_only(oracle, variant):
    """The chosen rays stay inside fp16's range themselves (|x| < 65504 / 2) but their first hidden layer exceeds 2 x 65504 at every
    point -- predicted by a float64 forward of layer 0 -- so the bits are set by layer 1's GEMM, not by layer 0's, and the bf16x3
    chain recomputes those rows from layer 0 on.  (Fails on a rerun="pass" handle too.)"""
    nets = inner_nets(oracle)
    ro, rd = rays_with_offset(oracle, FLAGGED, 3.0e4)
    pts = coarse_points(oracle, ro, rd)
    assert np.abs(pts).max() < FP16_MAX / 2
    h0 = layer0_f64(nets[0], pts)
    assert (h0[FLAGGED].max(axis=-1) > 2 * FP16_MAX).all() and np.isfinite(h0).all()      # every coarse point of the chosen rays
    assert h0[~FLAGGED].max() < FP16_MAX / 2                                              # ... and no point of the others
    make = lambda: models(nets[0], nets[1], NS, NI, (dict(rerun="rows"),))[0]
    if variant == "one chunk":
        got = chosen_rays_case(oracle, nets, ro, rd, FLAGGED, make, "inner layer")
        fine = ro[:, None] + rd[:, None] * cpu(got["z_fine"])[..., None]                  # the fine pass's points, and the fine network
        assert np.abs(fine).max() < FP16_MAX / 2
        h1 = layer0_f64(nets[1], fine.astype(np.float32))
        assert (h1[FLAGGED].max(axis=-1) > 2 * FP16_MAX).all() and h1[~FLAGGED].max() < FP16_MAX / 2
    else:
        with small_chunks():
            chosen_rays_case(oracle, nets, ro, rd, FLAGGED, make, "inner layer, 64-ray chunks")


def test_every_row_overflows(oracle):
    """trunk_range_nets: hidden unit 5 is 7e4 on every point of the coarse pass.  The rows handle walks every tile and stores every
    row: every tap and the pass counters equal the "pass" handle's."""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 171, 26)
    for layer in (1, 2):
        sd_c, sd_f = trunk_range_nets(oracle, layer)
        mp, mr = models(sd_c, sd_f, NS, NI, (dict(rerun="pass"), dict(rerun="rows")))
        rp, rr = (m.render_rays(ro, rd, near, far, debug=True) for m in (mp, mr))
        taps_equal(rp, rr, layer)
        sp, sr = mp.range_status(), mr.range_status()
        assert (sp["passes"], sp["passes_rerun"]) == (sr["passes"], sr["passes_rerun"]) == (2, 1), (sp, sr)
        assert sr["rows"] == 171 * (2 * NS + NI) and sr["rows_rerun"] == 171 * NS, sr
        assert np.isfinite(cpu(rr["rgb_map"])).all()
        mp.close()
        mr.close()


def bwd_gain_nets(oracle, log2):
    """bwd_range_nets with the weight 2^log2 in place of 2^RANGE_LOG2"""
    sd_c, sd_f = bwd_range_nets(oracle)
    sd_f = {k: v.copy() for k, v in sd_f.items()}
    sd_f["pts_linears.2.weight"][:, 5] = np.float32(2.0 ** log2)
    return sd_c, sd_f


def backward_case(oracle, nets, n=171):
    """the rgb gradient on a "pass" and a rows handle -> (gradients of the two, the rows of the fine backward, how many were flagged)"""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 27)
    cot = _cots(n, 29)["rgb_map"]
    mp, mr = models(nets[0], nets[1], NS, NI, (dict(rerun="pass"), dict(rerun="rows")))
    gp, gr = (m.render_rays_vjp(ro, rd, near, far, cot) for m in (mp, mr))
    sp, sr = mp.range_status(), mr.range_status()
    assert sp["passes"] == sr["passes"] == 3 and sp["passes_rerun"] == sr["passes_rerun"] == 1, (sp, sr)      # the backward, and no forward
    assert sr["rows"] == n * (NS + 2 * (NS + NI)), sr
    # ... and the first 37 rays alone have the bits they have in company, whatever was flagged
    few = mr.render_rays_vjp(ro[:37], rd[:37], near, far, cot[:37])
    for a, b in zip(gr, few):
        assert np.array_equal(cpu(a)[:37], cpu(b), equal_nan=True)
    mp.close()
    mr.close()
    return [cpu(x) for x in gp], [cpu(x) for x in gr], n * (NS + NI), sr["rows_rerun"]


def test_backward_all_rows(oracle):
    """bwd_range_nets with the gain 2^(RANGE_LOG2 + 8): the fine backward sends a gradient out of fp16's range at every point (the sum
    of a point's layer-2 gradients, normalised to 2^7 .. 2^8 in the largest entry, would have to be below 2^-6 to stay inside) and no
    forward does.  The rows handle's gradients are finite where the "pass" handle's are, and with every row of the backward flagged
    they are its bits."""
    gp, gr, rows, flagged = backward_case(oracle, bwd_gain_nets(oracle, RANGE_LOG2 + 8))
    print("backward rows", rows, "flagged", flagged)
    assert 0 < flagged <= rows
    for a, b in zip(gp, gr):
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.abs(b[np.isfinite(b)]).max() > 0
        if flagged == rows:
            assert np.array_equal(a, b, equal_nan=True)
    assert flagged == rows, (flagged, rows)


def test_backward_some_rows(oracle):
    """bwd_range_nets as it is, gain 2^RANGE_LOG2: dL/d(pre-activation of layer 1)[5] is the gain times the sum of a point's layer-2
    gradients, which depends on the point's relu masks and signs -- below 4 on some points, above on others -- so the backward flags
    some rows and not others.  The gradients are finite where the "pass" handle's are, and (backward_case) a ray's gradient does not
    depend on its company."""
    gp, gr, rows, flagged = backward_case(oracle, bwd_range_nets(oracle))
    print("backward rows", rows, "flagged", flagged)
    assert 0 < flagged < rows, (flagged, rows)
    for a, b in zip(gp, gr):
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.abs(b[np.isfinite(b)]).max() > 0


def test_company(oracle):
    """wide_onchip_cases.company_case's scheme, restated because its rays are clean and it asserts that no pass re-runs: 300 rays with
    the flagged rays of the chosen-rays case among them -- all rays, the rays reversed, the first 37 alone and 64-ray chunks give every
    ray the same bits, forward taps and rgb gradient.  (Fails on a rerun="pass" handle: the first 37 alone hold one flagged ray whose
    chunk is then all bf16x3, and in 64-ray chunks two of five chunks hold none.)"""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    n = 300
    flagged = np.zeros(n, bool)
    flagged[:N2] = FLAGGED
    ro, rd = rays_with_offset(oracle, flagged, 7.0e4, seed=22)
    cot = np.random.RandomState(23).standard_normal((n, 3)).astype(np.float32)
    sd_c, sd_f = trunk_nets(oracle, "3x100")
    m, = models(sd_c, sd_f, NS, NI, (dict(rerun="rows"),))
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw", "raw0")

    def run(sel):
        o, d, c = (np.ascontiguousarray(x[sel]) for x in (ro, rd, cot))
        r = m.render_rays(o, d, near, far, debug=True)
        chunks = m.last_kernel_ms()[1]
        go, gd = m.render_rays_vjp(o, d, near, far, c)
        return [cpu(r[k]) for k in keys] + [cpu(go), cpu(gd)], chunks
    whole, chunks = run(slice(None))
    assert chunks == 1 and np.isfinite(whole[0][~flagged]).all() and np.isfinite(whole[6][~flagged]).all() and np.abs(whole[6]).max() > 0
    rev, _ = run(slice(None, None, -1))
    few, _ = run(slice(0, 37))
    with small_chunks():
        cut, chunks = run(slice(None))
    assert chunks == (n + 63) // 64, chunks
    for k, a, b, c, d in zip(keys + ("grad_o", "grad_d"), whole, rev, few, cut):
        assert np.array_equal(a, b[::-1], equal_nan=True), (k, "reversed")
        assert np.array_equal(a[:37], c, equal_nan=True), (k, "the first 37 alone")
        assert np.array_equal(a, d, equal_nan=True), (k, "64-ray chunks")
    st = m.range_status()
    assert st["passes_rerun"] > 0 and 0 < st["rows_rerun"] < st["rows"], st
    m.close()


def g25_b_bad_rays(oracle):
    g = load_golden("g25_wide_networks")
    sd_c, sd_f, ns, ni = wide_case(oracle, g, "b")
    ro, rd = g["rays_o"].copy(), g["rays_d"].copy()
    bad_o, bad_d = ro.copy(), rd.copy()
    bad_o[5, 1] = np.nan
    bad_d[17, 0] = np.inf
    ok = np.ones(len(ro), bool)
    ok[[5, 17]] = False
    return sd_c, sd_f, ns, ni, (ro, rd), (bad_o, bad_d), ok


def test_neighbours_of_nan_and_infinite_rays_keep_their_bits(oracle):
    """test_gpu_wide.py::test_layered_renderer_nan_rays_stay_nan_and_alone had to drop the neighbours' bit equality on f16x2 (the
    infinite ray re-runs its passes, and the neighbours then carry bf16x3's bits).  On a rows handle it holds again: g25 case b with
    ro[5, 1] = NaN and rd[17, 0] = inf -- every output of every other ray equals the clean render's, the two bad rays are NaN, and
    the rows re-run are ray 17's points that hold an infinity.  A NaN does not flag (it compares false on both sides), and that
    decides the count: ray 17's 48 coarse points are o + inf z, infinite, and flag; its coarse weights are NaN, so its 100 resampled
    depths are NaN and those fine points are NaN in every coordinate -- they do not flag; the 48 fine points at the coarse depths do.
    Measured: rows_rerun = 96 = 48 + 48 of the ray's 48 + 148 points, which is the number the ray's own values give on the CPU below.
    (Fails on a rerun="pass" handle.)"""
    sd_c, sd_f, ns, ni, (ro, rd), (bo, bd), ok = g25_b_bad_rays(oracle)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    m, = models(sd_c, sd_f, ns, ni, (dict(rerun="rows"),))
    clean = m.render_rays(ro, rd, near, far)
    assert m.range_status()["rows_rerun"] == 0
    bad = m.render_rays(bo, bd, near, far, debug=True)
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std"):
        a, b = cpu(bad[k]), cpu(clean[k])
        assert np.array_equal(a[ok], b[ok], equal_nan=True), k
        if k != "z_std":
            assert np.isnan(a[~ok]).all(), k
    st = m.range_status()
    # ray 17's points with an infinite coordinate: every coarse one (z > 0), and the fine ones whose depth is a number
    with np.errstate(invalid="ignore"):
        fine = bo[17][None] + bd[17][None] * cpu(bad["z_fine"])[17][:, None]
    inf_fine = int((np.abs(fine) >= FP16_MAX).any(axis=1).sum())
    print("ray 17: fine points with an infinity", inf_fine, "of", ns + ni, st)
    assert st["passes_rerun"] >= 1 and st["rows_rerun"] == ns + inf_fine, (st, inf_fine)
    # ... which is 48 whatever the handle says: z_fine is the sorted union of the 48 coarse depths and the 100 resampled ones (RN:477), and
    # the resampled ones are NaN -- so the count is pinned apart from the tap as well
    assert inf_fine == ns == 48 and st["rows_rerun"] == 96, (inf_fine, st)
    m.close()


def test_capture_and_replay_with_other_rays_flagged(oracle):
    """One torch.cuda.graph capture of a render on the rows handle; the replay on rewritten input buffers equals the eager call,
    first with the chosen rays flagged, then with ANOTHER set of rays flagged: the counts, the lists and the masks are read on the
    device.  (wide_onchip_cases.replay_equals_eager's scheme, restated because that helper asserts that no pass re-runs and replays
    once: here the capture runs on clean rays and two flagged sets are replayed through it.)"""
    import torch
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    sd_c, sd_f = trunk_nets(oracle, "3x100")
    m, = models(sd_c, sd_f, NS, NI, (dict(rerun="rows"),))
    other = np.zeros(N2, bool)
    other[[3, 100, 101, 255]] = True
    sets = [rays_with_offset(oracle, FLAGGED, 7.0e4), rays_with_offset(oracle, other, 7.0e4)]
    host = lambda r: {k: cpu(r[k]) for k in TAPS}
    eager = [host(m.render_rays(o, d, near, far, debug=True)) for o, d in sets]
    assert not np.array_equal(eager[0]["rgb_map"], eager[1]["rgb_map"])
    dev = m.device
    clean = _rays(oracle, N2, 31)
    to, td = (torch.as_tensor(x, device=dev) for x in clean)               # clean rays while capturing
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        m.render_rays(to, td, near, far, debug=True)                       # this stream's workspace exists before the capture
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            r = m.render_rays(to, td, near, far, debug=True)
    before = m.range_status()["rows_rerun"]
    for (o, d), want, n_flagged in zip(sets, eager, (int(FLAGGED.sum()), int(other.sum()))):
        to.copy_(torch.as_tensor(o, device=dev))
        td.copy_(torch.as_tensor(d, device=dev))
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        got = host(r)
        for k in TAPS:
            assert np.array_equal(got[k], want[k], equal_nan=True), (k, n_flagged)
        after = m.range_status()["rows_rerun"]
        assert after - before == n_flagged * (2 * NS + NI), (before, after, n_flagged)
        before = after
    m.close()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the chosen-rays case and the backward case"""
    return [("range_chosen",) + trunk_nets(oracle, "3x100") + rays_with_offset(oracle, FLAGGED, 7.0e4),
            ("range_backward",) + bwd_range_nets(oracle) + _rays(oracle, 171, 27)]


def test_rows_mode_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks the word index of the f16x2 kernels' bit stores, the list position, the listed
    M-block against M and the word index of the masked epilogue (tag 100000 + line), and the list kernel's indices.  A fresh process runs
    the chosen-rays case and the backward case on a rows handle with a one-chunk and a 64-ray-chunk workspace; no check may trip, and
    every output equals the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_rerun_rows", "_bounds_runs"), dict(rerun="rows"), ("16", "0.0001"), ("render", "vjp_rgb"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 4, 6)
    assert {k: v[2] for k, v in got[0]["debug"].items()} == {k: v[2] for k, v in got[0]["release"].items()}


@pytest.mark.parametrize("tile", [128, 256])
def test_list_kernel_is_the_plan(tile):
    """kw_rows_list (through the handle-free entry nsrw_rerun_rows_list) on the row words of the chosen-rays case, coarse and fine, and
    on words with every bit behind row M set: the listed blocks are nsrw_rerun_rows_plan's (the kernel appends in no fixed order), the
    range word says whether there is one, and the counters hold M and the flagged rows below M"""
    from neural_sim_nerf_amd import wide
    none = np.zeros(N2, bool)
    last = np.zeros(N2, bool)
    last[-1] = True
    for flagged in (FLAGGED, none, ~none, last):
        for s in (NS, NS + NI):
            M = N2 * s
            w = rows_of(flagged, s)
            junk = np.concatenate([w, np.full(3, 0xffffffff, np.uint32)])
            junk[len(w) - 1] |= np.uint32((0xffffffff << (M % 32)) & 0xffffffff)
            want = wide.rerun_rows_plan(w, M, tile)
            for words in (w, junk):
                blocks, seen, n_flagged, word = wide.rerun_rows_list(words, M, tile)
                assert sorted(blocks) == want and len(set(blocks)) == len(blocks), (tile, s, blocks, want)
                assert (seen, n_flagged, word) == (M, int(flagged.sum()) * s, int(len(want) > 0)), (tile, s, seen, n_flagged, word)


def test_dropin_api_reaches_rows_mode(oracle):
    """NSR_WIDE_RERUN=rows reaches the handle the drop-in render() builds, and the strict neighbour equality holds there: g25 case b
    through render(rays=...) with the NaN and the infinite ray -- every other ray's outputs are the clean call's bits."""
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    sd_c, sd_f, ns, ni, (ro, rd), (bo, bd), ok = g25_b_bad_rays(oracle)
    D, W, in_ch, in_v, skips, _ = oracle.net_shape(sd_c)
    old = os.environ.get("NSR_WIDE_RERUN")
    os.environ["NSR_WIDE_RERUN"] = "rows"
    try:
        nets = []
        for sd in (sd_c, sd_f):
            net = R.NeRF(D=D, W=W, input_ch=in_ch, output_ch=5, skips=skips, input_ch_views=in_v, use_viewdirs=True)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            nets.append(net.to(R.device))
        kw = dict(network_query_fn=None, perturb=False, N_importance=ni, network_fine=nets[1], N_samples=ns, network_fn=nets[0],
                  use_viewdirs=True, white_bkgd=False, raw_noise_std=0., ndc=False, lindisp=False, near=oracle.YCBV_NEAR, far=oracle.YCBV_FAR)
        m = R._model_for(nets[0], nets[1], ni, kw)
        assert m.mlp == "layered-f16x2" and m.rerun == "rows"
        call = lambda o, d: R.render(400, 400, oracle.YCBV_K, chunk=4096, rays=torch.stack([torch.from_numpy(o), torch.from_numpy(d)], 0).to(R.device), **kw)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            clean = call(ro, rd)
            bad = call(bo, bd)
        for i, k in enumerate(("rgb_map", "disp_map", "acc_map")):
            a, b = cpu(bad[i]), cpu(clean[i])
            assert np.array_equal(a[ok], b[ok], equal_nan=True) and np.isnan(a[~ok]).all(), k
        for k in ("rgb0", "disp0", "acc0"):
            a, b = cpu(bad[3][k]), cpu(clean[3][k])
            assert np.array_equal(a[ok], b[ok], equal_nan=True), k
        st = m.range_status()
        assert st["passes_rerun"] >= 1 and 0 < st["rows_rerun"] <= ns + (ns + ni) and st["rows_rerun"] < 0.1 * st["rows"], st
        assert "_nsr_force_mlp" not in nets[0].__dict__                   # the share of ROWS decides, and it is tiny
    finally:
        if old is None:
            del os.environ["NSR_WIDE_RERUN"]
        else:
            os.environ["NSR_WIDE_RERUN"] = old
