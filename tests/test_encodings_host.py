"""CPU tests of the cases of the encodings' element-by-element tests (tests/encoding_cases.py, used on the device by
tests/test_gpu_wide_encodings.py): the float64 reference against 200-bit arithmetic, the reference implementation's own float32
sin / cos inside the bound, the selection networks exact through the oracle's float32 arithmetic, and five deliberately wrong
encoders, each of which the bound must catch."""
import numpy as np
import pytest

import encoding_cases as EC


def test_the_argument_set_covers_what_it_says():
    bulk, special = EC.targets()
    for L in (0, 1, 4, 10, 15, 16):
        x = EC.args(L)
        a = EC.band_args(x, L) if L else x[None]
        assert x.dtype == np.float32 and x.size < 1.35e6
        want = np.concatenate([bulk, special[np.isfinite(special)]]).view(np.uint32)          # (as bits: -0 is not +0)
        missing = want[~np.isin(want, a[np.isfinite(a)].view(np.uint32))]
        assert not missing.size, (L, missing.size, missing[:5].view(np.float32))
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        if L:       # every bulk coordinate is inside the fused encoder's domain: its top band stays below 2^24
            n_bulk = bulk.size
            assert (np.abs(a[L - 1, :n_bulk]) < EC.SWITCH).all()
    k = np.arange(1, EC.K_NEAR + 1) * (np.pi / 2)
    assert np.isin(k.astype(np.float32), bulk).all()
    edge = np.float32(EC.SWITCH)
    for v in (0.0, -0.0, 1e-45, EC.SWITCH - 1, np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, np.float32(np.inf)), 2.0 ** 127,
              EC.FLT_MAX):
        assert np.float32(v) in special and np.float32(-v) in special
    assert np.signbit(special[special == 0]).any() and not np.signbit(special[special == 0]).all()


def test_the_bound_at_zero_and_among_the_denormals():
    """ulp32 is float32's spacing, 2^-149 at a zero result and among the denormals; the bound at a = 0 is two denormal steps, so
    nothing but a zero or the two smallest denormals passes for sin(0), and cos(0) has 2 ulp of 1 (the spacing above 1)"""
    t = np.array([0.0, -0.0, 1e-45, 1e-40, 2.0 ** -126, 2.0 ** -125, 0.75, 1.0, -1.0, np.nan])
    assert np.array_equal(EC.ulp32(t), 2.0 ** np.array([-149, -149, -149, -149, -149, -148, -24, -23, -23, -23.0]))
    with np.errstate(invalid="ignore"):
        f = t[np.isfinite(t)].astype(np.float32)
        assert np.array_equal(EC.ulp32(f.astype(np.float64)), np.spacing(np.abs(f)).astype(np.float64))
    zero = np.float32([0.0, -0.0])
    assert np.array_equal(EC.bound(zero, np.zeros(2)), np.full(2, 2.0 ** -148))
    for got, bad in ((0.0, False), (-0.0, False), (2.0 ** -148, False), (-2.0 ** -148, False), (4.3e-45, True), (1e-40, True), (-1e-40, True),
                     (1e-7, True), (np.nan, True)):
        assert EC.judge(np.float32([got, got]), zero, np.zeros(2))["bad"].tolist() == [bad, bad], got
    for got, bad in ((1.0, False), (1.0 - 2.0 ** -22, False), (1.0 - 2.0 ** -21, True), (1.0 + 2.0 ** -22, False), (1.0 + 2.0 ** -21, True)):
        assert EC.judge(np.float32([got, got]), zero, np.ones(2))["bad"].tolist() == [bad, bad], got


def test_true_sincos_agrees_with_200_bit_arithmetic():
    """numpy's float64 sin / cos of 10^4 of the band arguments of args(15) -- near multiples of pi / 2, tiny, huge -- is within one
    float64 rounding (1 ulp of float64) of mpmath's value at 200 bits (FLT_MAX needs 128 bits of pi and 53 of result)"""
    import mpmath
    _, a, s, c = EC.reference(15)
    flat = np.flatnonzero(np.isfinite(a.ravel()))
    pick = np.random.RandomState(3).choice(flat, 10000, replace=False)
    pick[:4] = [flat[np.argmax(a.ravel()[flat])], flat[np.argmin(a.ravel()[flat])], flat[0], flat[-1]]
    worst = 0.0
    with mpmath.workprec(200):
        for i in pick:
            x = mpmath.mpf(float(a.ravel()[i]))
            for got, want in ((s.ravel()[i], mpmath.sin(x)), (c.ravel()[i], mpmath.cos(x))):
                _, e = np.frexp(abs(float(want)))
                ulp64 = 2.0 ** (max(int(e), -1021) - 53)
                err = float(abs(mpmath.mpf(float(got)) - want)) / ulp64
                worst = max(worst, err)
                assert err <= 1.0, (float(x), float(got), err)
    print("true_sincos against mpmath at 200 bits: worst %.3f ulp of float64" % worst)


def test_the_reference_implementations_own_float32_sin_cos_is_inside_the_bound():
    """torch's float32 sin / cos on the CPU -- the reference's arithmetic (RH:39-48) -- on every band argument of args(15): inside
    the bound by itself, so that the bound asks nothing of a kernel the reference does not deliver"""
    import torch
    _, a, s, c = EC.reference(15)
    worst, n_bad = 0.0, 0
    for l in range(a.shape[0]):
        t = torch.from_numpy(a[l].copy())
        for got, true in ((torch.sin(t).numpy(), s[l]), (torch.cos(t).numpy(), c[l])):
            j = EC.judge(got, a[l], true)
            n_bad += int(j["bad"].sum())
            worst = max(worst, float(j["ulps"].max()))
    print("torch float32 sin / cos on args(15): worst %.3f ulp of the result" % worst)
    assert n_bad == 0 and worst <= 1.0, (n_bad, worst)


@pytest.mark.parametrize("L,output_ch", [(0, 32), (1, 32), (4, 32), (4, 4), (10, 32), (15, 32)])
def test_the_selection_networks_copy_the_encoding_exactly(L, output_ch, oracle):
    """embed + mlp of the oracle in float32 (run_network's arithmetic, RN:26-40) on the selection networks: output j of a network
    is its column j of oracle.embed, bit for bit (but for the sign of a zero), on 20 000 rows of args(L) -- FLT_MAX and denormals
    among them; a row with a non-finite column (x or 2^l x is inf or NaN) is NaN throughout; the groups cover every column once"""
    pts = EC.points(EC.args(L), L)
    pts = np.ascontiguousarray(np.concatenate([pts[:: max(1, len(pts) // 20000)], pts[-6000:]]))
    with np.errstate(invalid="ignore", over="ignore"):
        e = oracle.embed(pts, L)
    nan_row = EC.poisoned(pts, L).any(1)
    assert nan_row.any() and np.isfinite(e[~nan_row]).all() and not np.isfinite(e[nan_row]).all(1).any()
    e[nan_row] = np.nan
    nets = EC.select_nets(L, output_ch)
    assert sorted(c for g, _ in nets for c in g) == list(range(3 + 6 * L)) and len(nets) == -(-(3 + 6 * L) // output_ch)
    for cols, sd in nets:
        assert oracle.net_shape(sd) == (2, 64, 3 + 6 * L, 0, [], False)
        with np.errstate(invalid="ignore"):
            out = oracle.mlp(sd, np.where(nan_row[:, None], np.float32(np.nan), e), views=np.zeros((len(pts), 0), np.float32), all_rows=True)
        assert out.shape == (len(pts), output_ch) and out.dtype == np.float32
        assert np.array_equal(out[:, :len(cols)], e[:, cols], equal_nan=True)
        assert not out[~nan_row, len(cols):].any()


def _control_arguments():
    x = EC.args(4)[::3]
    a = EC.band_args(x, 4).ravel()
    return (a,) + EC.true_sincos(a)


def test_the_restated_device_formulas_are_inside_the_bound():
    """the numpy restatement of sincos_enc (the controls' starting point) meets the bound on every argument of the controls"""
    a, s, c = _control_arguments()
    es, ec = EC.emulate(a)
    js, jc = EC.judge(es, a, s), EC.judge(ec, a, c)
    print("restated sincos_enc: worst %.3f ulp of the result, worst ratio to the bound %.3f"
          % (max(js["ulps"].max(), jc["ulps"].max()), max(js["ratio"].max(), jc["ratio"].max())))
    assert not js["bad"].any() and not jc["bad"].any()


@pytest.mark.parametrize("wrong", EC.VARIANTS)
def test_a_wrong_encoder_breaks_the_bound(wrong):
    """each of the five wrong encoders misses the bound on at least 1 % of the arguments it touches (sin and cos counted together)"""
    a, s, c = _control_arguments()
    es, ec = EC.emulate(a, wrong)
    t = EC.touched(a, wrong)
    bad = (EC.judge(es, a, s)["bad"] & t).sum() + (EC.judge(ec, a, c)["bad"] & t).sum()
    frac = bad / (2.0 * t.sum())
    print("%s: %d arguments touched, %.1f %% of their results beyond the bound" % (wrong, t.sum(), 100 * frac))
    assert t.sum() > 1000 and frac >= 0.01, (wrong, frac)
