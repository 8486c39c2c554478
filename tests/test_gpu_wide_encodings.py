"""GPU tests that hold BOTH renderers' encodings to true sin / cos, element by element (run with -m gpu on an MI355X): kw_embed of
the layered renderer in its points form and its rays form (sincos_enc in csrc/nsr_wide.hip), the on-chip encoder at arguments of the
library path, the encoder's VJP (kw_embed_vjp) and the fused library's Embedder.embed (enc_trig in csrc/nsr_kernels.hip).  The
arguments, the float64 reference, the bound and its derivation are tests/encoding_cases.py's:

    |got - true| <= 2 ulp32(true) + |a| 2^-52   for |a| < 2^24,      1 ulp32(true) beyond (layered),      NaN beyond (fused)

The layered encoder has no entry point of its own, so its values are read through SELECTION networks: on an mlp="fp32" handle every
product of such a network is 1 e or 0 e and every sum has one non-zero term, so run_network returns the encoding's columns
themselves (tests/test_encodings_host.py holds the networks to that on the CPU).  A row in which a column is not finite -- x, or
2^l x, is inf or NaN -- is NaN throughout (0 * NaN), which is what the tests ask of it.

Each body returns what it measured -- the largest error in ulp of the result, the largest ratio to the bound, and the arguments that
gave them -- and prints it; profiles/r20/extra/encodings.txt is those lines."""
import numpy as np
import pytest

import encoding_cases as EC

pytestmark = pytest.mark.gpu

SMALL_P = (1, 15, 17, 257)            # the 16-point workgroups of kw_embed: one point, a tail of 15, one past a group, one past 16 groups


def cpu(t):
    return t.detach().cpu().numpy()


class Worst:
    """the largest error in ulp of the result and the largest ratio to the bound, each with the argument that gave it"""

    def __init__(self, what):
        self.what, self.ulps, self.ratio, self.n, self.n_bad, self.first_bad = what, (0.0, 0.0), (0.0, 0.0), 0, 0, None

    def take(self, j, a, what):
        a = np.broadcast_to(a, j["bad"].shape)
        for key in ("ulps", "ratio"):
            i = np.unravel_index(np.argmax(j[key]), j[key].shape)
            if j[key][i] > getattr(self, key)[0]:
                setattr(self, key, (float(j[key][i]), float(a[i])))
        self.n += j["bad"].size
        nb = int(j["bad"].sum())
        if nb and self.first_bad is None:
            i = np.unravel_index(np.argmax(j["bad"]), j["bad"].shape)
            self.first_bad = (what, float(a[i]), float(j["ulps"][i]), float(j["ratio"][i]))
        self.n_bad += nb

    def line(self):
        return ("%-32s %9d elements: worst %8.3f ulp of the result at a = %-12.9g ratio to the bound %.3f at a = %.9g"
                % ((self.what, self.n) + self.ulps + self.ratio))

    def check(self):
        print(self.line())
        assert self.n_bad == 0, "%s: %d of %d elements miss the bound, the first (what, a, ulp, ratio) %r" % (self.what, self.n_bad, self.n, self.first_bad)
        return self


def judge_reference_rows(w, got, idx, L, nan_coord, exact_nan_row=None):
    """got [P, 3 + 6 L] against the encoding of the points args(L)[idx] (idx [P, 3]) by the shared reference(L): the identity columns
    exact, every trig column to the bound at its argument 2^l x; nan_coord [P, 3]: the coordinates whose trig columns must be NaN
    beside those with a non-finite argument; exact_nan_row [P]: rows whose identity columns are NaN too (behind a network)"""
    x, a, s, c = EC.reference(L)
    ident = x[idx] if exact_nan_row is None else np.where(exact_nan_row[:, None], np.float32(np.nan), x[idx])
    assert got.shape == (len(idx), 3 + 6 * L) and got.dtype == np.float32
    assert np.array_equal(got[:, :3], ident, equal_nan=True), (w.what, "identity columns")
    for l in range(L):
        al = a[l][idx]
        w.take(EC.judge(got[:, 3 + 6 * l:6 + 6 * l], al, s[l][idx], nan_coord), al, "sin band %d" % l)
        w.take(EC.judge(got[:, 6 + 6 * l:9 + 6 * l], al, c[l][idx], nan_coord), al, "cos band %d" % l)


# ---- kw_embed, points form ----------------------------------------------------------------------------------------------------
def select_models(L, output_ch=32, n_importance=0):
    """[(columns, an mlp="fp32" handle on the selection network of those columns)]"""
    from neural_sim_nerf_amd.wide import WideModel
    return [(cols, WideModel(sd, sd if n_importance else None, n_samples=3, n_importance=n_importance, mlp="fp32"))
            for cols, sd in EC.select_nets(L, output_ch)]


def encode_points(ms, pts, L):
    """[P, 3 + 6 L]: kw_embed's row of every point, read through the selection networks' run_network"""
    out = np.empty((len(pts), 3 + 6 * L), np.float32)
    for cols, m in ms:
        raw = cpu(m.run_network(pts, None, 0))
        assert raw.shape == (len(pts), 32) and not np.nan_to_num(raw[:, len(cols):]).any()
        out[:, cols] = raw[:, :len(cols)]
    return out


def points_form(L):
    x = EC.args(L)
    idx = EC.point_index(x, L)
    pts = EC.points(x, L)
    nan_row = EC.poisoned(pts, L).any(1)
    nan_coord = np.repeat(nan_row[:, None], 3, 1)
    assert nan_row.any() and not nan_row.all()
    ms = select_models(L)
    w = Worst("kw_embed points form, L = %d" % L)
    got = encode_points(ms, pts, L)
    judge_reference_rows(w, got, idx, L, nan_coord, nan_row)
    for P in SMALL_P:                                   # the workgroup tails and every padded row length on few points
        sel = np.unique(np.linspace(0, len(pts) - 1, P).astype(np.int64))
        few = encode_points(ms, np.ascontiguousarray(pts[sel]), L)
        assert np.array_equal(few, got[sel], equal_nan=True), (L, P)
    for _, m in ms:
        m.close()
    return w.check()


@pytest.mark.parametrize("L", [0, 1, 4, 10, 15])
def test_kw_embed_points_form(L):
    """run_network of an mlp="fp32" handle on select_nets(L) over args(L) as [P, 3], each coordinate taking each value: every trig
    column inside the bound, the identity columns exact, a row with a non-finite column NaN; the same rows alone -- 1, 15, 17 and
    257 points -- give the same bits (row lengths 32, 64 and 96 floats: L = 0 .. 4, 10, 15)"""
    points_form(L)


# ---- kw_embed, rays form --------------------------------------------------------------------------------------------------------
def _hard_rays(n=301):
    """rays whose points o + d z reach arguments from 1e-3 to 2^23 at 3 + 2 samples between near = 2 and far = 6"""
    rng = np.random.RandomState(41)
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(2.0 ** 19), (n, 3)))
    ro = (mag * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
    rd = (rng.standard_normal((n, 3)) * np.exp(rng.uniform(np.log(1e-2), np.log(1e3), (n, 1)))).astype(np.float32)
    ro[:8] = [[0, -0.0, 1e-30], [np.pi, -np.pi / 2, np.pi / 4], [1e5, -3e5, 5e5]] + [[0.5, 1.5, 2.5]] * 5
    return ro, rd


def rays_form(oracle, L=4):
    near, far = 2.0, 6.0
    ro, rd = _hard_rays()
    n = len(ro)
    z0 = oracle.coarse_z(np.full(n, near, np.float32), np.full(n, far, np.float32), n=3)
    w = Worst("kw_embed rays form, L = %d" % L)
    pt = lambda z: (ro[:, None, :] + (rd[:, None, :] * z[:, :, None]).astype(np.float32)).astype(np.float32)     # fl(o + fl(d z))
    for cols, m in select_models(L, output_ch=4, n_importance=2):
        r = m.render_rays(ro, rd, near, far, debug=True)
        zf = cpu(r["z_fine"])
        assert np.isfinite(zf).all() and zf.shape == (n, 5)
        for tap, z in (("raw0", z0), ("raw", zf)):
            raw = cpu(r[tap]).reshape(-1, 4)
            x3 = pt(z).reshape(-1, 3)
            assert np.isfinite(x3).all() and np.abs(x3).max() * 2.0 ** (L - 1) < EC.SWITCH
            a = EC.band_args(x3, L)
            for j, col in enumerate(cols):
                if col < 3:
                    assert np.array_equal(raw[:, j], x3[:, col]), (tap, col)
                    continue
                l, k = divmod(col - 3, 6)
                s, c = EC.true_sincos(a[l][:, k % 3])
                w.take(EC.judge(raw[:, j], a[l][:, k % 3], c if k >= 3 else s), a[l][:, k % 3], "%s column %d" % (tap, col))
            assert not raw[:, len(cols):].any()
        m.close()
    return w.check()


def test_kw_embed_rays_form(oracle):
    """render_rays(debug=True) at 3 + 2 samples on the output_ch = 4 selection networks of L = 4, one handle per four columns: the
    raw0 and raw taps are the encodings of the points fl(o + fl(d z)) -- the product not contracted -- at the linspace depths and at
    the z_fine tap: identity columns exact, trig columns inside the bound at a = fl(x 2^l)"""
    rays_form(oracle)


# ---- the on-chip encoder at arguments of the library path ---------------------------------------------------------------------
def _peak_activation(oracle, sd, pts, dirs):
    """per point, the largest magnitude among the operands of the network's GEMMs behind the encodings (the oracle, fp32)"""
    keep = {}
    _, W, input_ch, in_v, _, _ = oracle.net_shape(sd)
    ed = oracle.embed(dirs, (in_v - 3) // 6)
    oracle.mlp(sd, oracle.embed(pts, (input_ch - 3) // 6), keep=keep, views=ed)
    h = keep["h%d" % (len(keep) - 1)]
    feat = h @ sd["feature_linear.weight"].T + sd["feature_linear.bias"]
    hv = np.concatenate([feat, ed], 1) @ sd["views_linears.0.weight"].T + sd["views_linears.0.bias"]
    return np.max([np.abs(v).max(1) for v in list(keep.values()) + [feat, hv]], 0)


def test_the_on_chip_encoder_at_hard_finite_arguments(oracle):
    """The f16x2 network 3x40-L15 on (trunk="onchip", embed="layers") and (trunk="onchip", embed="onchip"): run_network on 1031
    points with 1024 <= |x| < 60000, chosen with the oracle so that no activation comes within a factor 4 of fp16's largest number:
    no range event, what leaves is what the on-chip encoder computed.  In trunk_rows_encode a wave owns 32 consecutive points and a
    lane eight columns of one of them.  Band 14 is the library routine's at every one of these points, so in every wave some lane
    meets such an argument, the wave-wide ballot fires and the wave computes every column once more through embed_col_hard, where
    sincos_enc branches lane by lane: among the 32 points of every wave, bands 11 .. 13 hold arguments on either side of 2^24.
    Then the same points with every other one, and every other wave as a whole, replaced by a point of |x| < 1 -- lanes that met no
    such argument beside lanes that did, and waves in which the ballot does not fire beside waves in which it does.  Then three
    coordinates above 65504: a re-run.  Equal bits and equal range counters each time, and the encodings ran on chip."""
    from wide_onchip_cases import bwd_nets, models
    sd_c, sd_f = bwd_nets(oracle, "3x40-L15")
    rng = np.random.RandomState(43)
    N, P = 8000, 1031
    mag = np.exp(rng.uniform(np.log(1024.0), np.log(60000.0), (N, 3)))
    pts = np.minimum(mag, 59999.0).astype(np.float32) * rng.choice([-1.0, 1.0], (N, 3)).astype(np.float32)
    dirs = oracle.normalize_dirs(rng.standard_normal((N, 3)).astype(np.float32))
    small = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)
    peak = lambda p: np.maximum(_peak_activation(oracle, sd_c, p, dirs), _peak_activation(oracle, sd_f, p, dirs))
    calm = (peak(pts) < 65504.0 / 4) & (peak(small) < 65504.0 / 4)
    assert calm.sum() >= P
    pts, small, dirs = (np.ascontiguousarray(v[calm][:P]) for v in (pts, small, dirs))
    assert (np.abs(pts) >= 1024).all() and (np.abs(pts) < 60000).all()
    for band in (11, 12, 13):
        wave = (np.abs(pts[: P // 32 * 32]) * 2.0 ** band >= EC.SWITCH).reshape(-1, 32 * 3)
        assert (wave.any(1) & ~wave.all(1)).all(), band                       # the 32 points of every wave hold both kinds
    row = np.arange(P)
    mixed = np.where((((row // 32) % 2 == 1) | (row % 2 == 1))[:, None], small, pts)
    beyond = pts.copy()
    beyond[[5, 300, 777], [0, 1, 2]] = [70000.0, -1.0e6, 3.0e9]
    ml, mo = models(sd_c, sd_f, 3, 2, (dict(trunk="onchip", embed="layers"), dict(trunk="onchip", embed="onchip")))
    for net_id in (0, 1):
        for what, p in (("hard", pts), ("mixed", mixed)):
            before = [m.range_status() for m in (ml, mo)]
            a, b = (cpu(m.run_network(p, dirs, net_id)) for m in (ml, mo))
            assert np.array_equal(a, b) and np.isfinite(b).all(), (net_id, what)
            mid = [m.range_status() for m in (ml, mo)]
            assert mid[0] == mid[1] and mid[0]["passes"] > before[0]["passes"] and mid[0]["passes_rerun"] == before[0]["passes_rerun"], (what, before, mid)
        a, b = (cpu(m.run_network(beyond, dirs, net_id)) for m in (ml, mo))
        assert np.array_equal(a, b, equal_nan=True), net_id
        after = [m.range_status() for m in (ml, mo)]
        assert after[0] == after[1] and after[0]["passes_rerun"] > mid[0]["passes_rerun"], (mid, after)
    assert mo.embed_status()["passes_onchip"] >= 6 and ml.embed_status()["passes_onchip"] == 0
    ml.close()
    mo.close()


# ---- the encoder's VJP --------------------------------------------------------------------------------------------------------
def _cotangents(P, L, seed):
    """[P, 3 + 6 L] float32 of mixed magnitude: N(0, 1) times 10^(a row's exponent + a column's), from 1e-6 to 1e3"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((P, 3 + 6 * L), dtype=np.float32)
    g *= (10.0 ** rng.uniform(-4, 2, (P, 1))).astype(np.float32)
    g *= (10.0 ** rng.uniform(-2, 1, (1, 3 + 6 * L))).astype(np.float32)
    return g


def vjp_form(L):
    """wide.embed_vjp on args(L) against float64, element by element.  gx[c] = g[c] + sum_l 2^l (g_sin cos(a_l) - g_cos sin(a_l)): the
    device's sin / cos carry the encoding bound B, its fp64 products and sum are exact to 2^-53 each and it rounds once, so
        |got - true| <= sum_l 2^l (|g_sin| B(cos a_l) + |g_cos| B(sin a_l)) + (2 L + 2) 2^-24 (|g[c]| + sum_l |terms|)"""
    from neural_sim_nerf_amd import wide
    x, a, s, c = EC.reference(L)
    idx = EC.point_index(x, 0)
    pts = np.ascontiguousarray(x[idx])
    P = len(pts)
    g = _cotangents(P, L, 50 + L)
    got = cpu(wide.embed_vjp(pts, g, L)).astype(np.float64)
    assert got.shape == (P, 3)
    true = g[:, :3].astype(np.float64)
    mags = np.abs(true)
    slack = np.zeros((P, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(L):
            al, sl, cl = a[l][idx], s[l][idx], c[l][idx]
            gs, gc = (g[:, 3 + 6 * l + k:6 + 6 * l + k].astype(np.float64) for k in (0, 3))
            true += 2.0 ** l * (gs * cl - gc * sl)
            mags += 2.0 ** l * (np.abs(gs * cl) + np.abs(gc * sl))
            slack += 2.0 ** l * (np.abs(gs) * EC.bound(al, cl) + np.abs(gc) * EC.bound(al, sl))
        want_nan = EC.poisoned(pts, L) if L else np.zeros((P, 3), bool)          # (L = 0: no argument, gx = g whatever x is)
        limit = slack + (2 * L + 2) * 2.0 ** -24 * mags
        err = np.abs(got - true)
        bad = np.where(want_nan, ~np.isnan(got), ~(err <= limit))
        ratio = np.where(want_nan, 0.0, err / limit)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%-32s %9d elements: worst ratio to the bound %.3f at x = %.9g (error %.3e, bound %.3e)"
          % ("embed_vjp, L = %d" % L, ratio.size, ratio[i], pts[i], err[i], limit[i]))
    assert want_nan.any() == (L > 0) and not bad.any(), (L, int(bad.sum()), pts[bad][:5], got[bad][:5], true[bad][:5])
    if L == 0:
        assert np.array_equal(got.astype(np.float32), g[:, :3], equal_nan=True)
    for n in (1, 255, 257):                             # one thread, a block's tail, one past a block
        sel = np.unique(np.linspace(0, P - 1, n).astype(np.int64))
        few = cpu(wide.embed_vjp(np.ascontiguousarray(pts[sel]), np.ascontiguousarray(g[sel]), L)).astype(np.float64)
        assert np.array_equal(few, got[sel], equal_nan=True), (L, n)
    return float(ratio[i]), float(pts[i])


@pytest.mark.parametrize("L", [0, 4, 15])
def test_embed_vjp(L):
    """nsrw_embed_vjp on args(L) with cotangents over nine orders of magnitude, against float64 with a bound per element computed
    from the float64 terms; NaN exactly where an argument is not finite; 1, 255 and 257 points alone give the same bits"""
    vjp_form(L)


# ---- the fused library's Embedder.embed ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused(synth_nets):
    from neural_sim_nerf_amd.engine import NsrModel
    m = NsrModel(synth_nets[0], synth_nets[1])
    yield m
    m.close()


def fused_form(model, L):
    x = EC.args(L)
    idx = EC.point_index(x, 0)
    pts = np.ascontiguousarray(x[idx])
    with np.errstate(invalid="ignore"):
        outside = ~(np.abs(pts.astype(np.float64)) * 2.0 ** (L - 1) < EC.SWITCH)          # enc_domain: NaN there, inf and NaN included
    below = np.nextafter(np.float32(EC.SWITCH), np.float32(0)) * np.float32(2.0 ** -(L - 1))      # the top band one float below 2^24
    assert (pts == below).any() and (pts == -below).any() and not outside[np.abs(pts) == below].any()
    assert outside[np.abs(pts) == np.float32(EC.SWITCH * 2.0 ** -(L - 1))].all() and outside.any()
    w = Worst("fused Embedder.embed, L = %d" % L)
    got = cpu(model.embed(pts, L))
    judge_reference_rows(w, got, idx, L, outside)
    for P in SMALL_P:
        sel = np.unique(np.linspace(0, len(pts) - 1, P).astype(np.int64))
        assert np.array_equal(cpu(model.embed(np.ascontiguousarray(pts[sel]), L)), got[sel], equal_nan=True), (L, P)
    return w.check()


@pytest.mark.parametrize("L", [1, 4, 10, 16])
def test_fused_embed(fused, L):
    """nsr_embed (k_embed: enc_domain, enc_trig) on args(L): the identity columns exact; a coordinate's trig columns NaN exactly where
    2^(L-1) |x| >= 2^24 (inf and NaN too), and finite and inside the bound everywhere else, one float below that edge included"""
    fused_form(fused, L)
