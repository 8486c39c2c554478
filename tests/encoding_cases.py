"""The cases of the encodings' element-by-element tests (tests/test_encodings_host.py, tests/test_gpu_wide_encodings.py): the
arguments at which a sin / cos with an explicit range reduction goes wrong, the float64 reference, the bound per element, the
networks that copy encoding columns to the output exactly, a numpy restatement of the device formulas and five deliberately wrong
versions of it.  Pure numpy.

THE BOUND.  Both renderers reduce with ONE fp64 product (sincos_enc_fast in csrc/nsr_wide.hip, enc_trig in csrc/nsr_kernels.hip: the
same lines): t = a * fl64(2 / pi), n = rint(t) and f = t - n exactly, r = fl32(f * fl64(pi / 2)), polynomials in r.  The constant
and the product each round at 2^-53 relative, so t is off by at most |t| 2^-52, and r = f pi / 2 by |t| 2^-52 pi / 2 = |a| 2^-52
radians -- sin and cos have slope <= 1, so that is the error the reduction leaves in the result, whatever the result's size.  What
follows it -- r rounded to fp32, a minimax polynomial, the fmas -- is held to the project's "2 ulp of 1"
(tests/test_gpu_parity.py::test_embed_large_arguments) made relative: 2 ulp of the true value.  So, for |a| < 2^24:

    |got - true| <= 2 ulp32(true) + |a| 2^-52

(enc_trig's reduction is sincos_enc_fast's, constant for constant: the same term.)  For |a| >= 2^24 the layered renderer takes the
fp64 library routine and rounds once: 1 ulp32(true); the fused renderer answers NaN there.  inf and NaN give NaN.  The sign of a
zero result is not part of the bound."""
import functools

import numpy as np

f32 = np.float32
SWITCH = 16777216.0                       # 2^24: sincos_enc_is_fast, enc_domain
TWO_OVER_PI = 0.63661977236758134308
PI_OVER_2 = 1.57079632679489661923
K_NEAR = 300000                           # the float nearest to k pi / 2 and its two neighbours, k = 1 .. K_NEAR
N_RANDOM_K = 200000
N_LOG = 100000                            # log-uniform |a| in [1e-30, 2^24), both signs
N_BEYOND = 4000                           # log-uniform |a| in [2^24, FLT_MAX]: the layered slow path, the fused NaN domain
FLT_MAX = float(np.finfo(f32).max)


# ---- the arguments ----------------------------------------------------------------------------------------------------------
def _neighbours(a):
    a = a.astype(f32)
    return np.concatenate([np.nextafter(a, f32(-np.inf)), a, np.nextafter(a, f32(np.inf))])


@functools.lru_cache(maxsize=None)
def targets():
    """(bulk, special): float32 band arguments.  bulk: every one finite with |a| < 2^24, each wanted in one band; special: the few
    wanted in every band -- zeros, denormals, the switch, powers of two, FLT_MAX, inf, NaN."""
    rng = np.random.RandomState(20)
    near = _neighbours(np.arange(1, K_NEAR + 1, dtype=np.float64) * (np.pi / 2))
    kmax = int(SWITCH * 2 / np.pi) - 1
    rand = (rng.randint(1, kmax, N_RANDOM_K).astype(np.float64) * (np.pi / 2)).astype(f32)
    logu = np.exp(rng.uniform(np.log(1e-30), np.log(SWITCH), N_LOG)).astype(f32)
    logu = np.minimum(logu, np.nextafter(f32(SWITCH), f32(0)))
    sign = lambda v: (v * rng.choice([-1.0, 1.0], v.shape)).astype(f32)
    bulk = np.concatenate([near, -near[::20], sign(rand), sign(logu)]).astype(f32)
    assert np.isfinite(bulk).all() and (np.abs(bulk) < SWITCH).all()
    tiny = np.finfo(f32).tiny
    edge = f32(SWITCH)
    pos = [0.0, 1.401298464324817e-45, 1e-42, float(np.nextafter(f32(tiny), f32(0))), float(tiny),
           SWITCH - 1.0, float(np.nextafter(edge, f32(0))), SWITCH, float(np.nextafter(edge, f32(np.inf))), FLT_MAX, np.inf]
    pos += [2.0 ** e for e in range(-126, 128)]
    beyond = np.exp(rng.uniform(np.log(SWITCH), np.log(FLT_MAX), N_BEYOND))
    special = np.array(pos, dtype=np.float64)
    special = np.concatenate([special, -special, np.minimum(beyond, FLT_MAX) * rng.choice([-1.0, 1.0], N_BEYOND), [np.nan]]).astype(f32)
    return bulk, special


@functools.lru_cache(maxsize=None)
def args(L):
    """float32 coordinates x whose band arguments x 2^l, l < L (L = 0: x itself), cover targets(): x = a 2^-l, exact.  A bulk
    argument goes to one band, in turn -- or to the top band where a lower one would put 2^(L-1) |x| at 2^24 or beyond, so that
    every bulk argument stays inside the fused encoder's domain too; every special argument goes to every band (a denormal one that
    2^-l would round: to band 0 alone).  The other bands of an x are arguments as well, and are checked like these."""
    bulk, special = targets()
    nb = max(L, 1)
    band = np.arange(bulk.size) % nb
    band = np.where(np.abs(bulk.astype(np.float64)) * 2.0 ** (nb - 1 - band) >= SWITCH, nb - 1, band)
    xs = [np.ldexp(bulk, -band).astype(f32)]
    assert np.array_equal(np.ldexp(xs[0], band), bulk)
    for l in range(nb):
        x = np.ldexp(special, -l).astype(f32)
        keep = np.ldexp(x, l) == special
        xs.append(x[keep | np.isnan(special)] if l else x)
    x = np.concatenate(xs)
    x.setflags(write=False)
    return x


def band_args(x, L):
    """[L, ...]: the fp32 arguments 2^l x (exact but for overflow to inf, which the device shares)"""
    with np.errstate(over="ignore"):
        return np.stack([(x.astype(f32) * f32(2.0 ** l)).astype(f32) for l in range(L)]) if L else np.zeros((0,) + x.shape, f32)


def point_index(v, L=0, stride=7919):
    """[P, 3] indices into v of the points in which each coordinate takes each value of v: the values whose every band argument is
    finite in three rotations of the list, so that a row holds three unrelated values, and a row [w, w, w] for every other w
    (behind a network a non-finite encoding column makes the whole row NaN: 0 * NaN)"""
    bad = poisoned(v, L)
    i, j = np.flatnonzero(~bad), np.flatnonzero(bad)
    s = stride % max(i.size, 1)
    return np.concatenate([np.stack([i, np.roll(i, s), np.roll(i, 2 * s)], 1), np.repeat(j[:, None], 3, 1)])


def points(v, L=0):
    """[P, 3] float32: v at point_index(v, L)"""
    return np.ascontiguousarray(v[point_index(v, L)].astype(f32))


def poisoned(x, L):
    """mask of the coordinates with a non-finite encoding column: x itself or its top band argument 2^(L-1) x is inf or NaN"""
    with np.errstate(over="ignore"):
        return ~np.isfinite((x.astype(f32) * f32(2.0 ** max(L - 1, 0))).astype(f32))


# ---- the reference and the bound -----------------------------------------------------------------------------------------------
def true_sincos(a):
    """(sin, cos) of the fp32 arguments, in float64: numpy's libm on float64(a) (held to mpmath in test_encodings_host.py)"""
    a64 = np.asarray(a).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.sin(a64), np.cos(a64)


def ulp32(t):
    """the spacing of float32 at the float64 value t: 2^(floor(log2 |t|) - 23), and 2^-149 at zero and among the denormals"""
    t = np.abs(np.where(np.isfinite(t), t, 1.0))
    _, e = np.frexp(t)
    return np.where(t == 0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def bound(a, true):
    """the largest |got - true| allowed at the argument a (finite): 2 ulp32(true) + |a| 2^-52 below the switch, 1 ulp32(true) at
    and beyond it"""
    mag = np.abs(np.asarray(a).astype(np.float64))
    u = ulp32(true)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(mag < SWITCH, 2.0 * u + mag * 2.0 ** -52, u)


def judge(got, a, true, nan_where=False):
    """got (float32) against the float64 `true` at the arguments a, element by element.  A non-finite a must give NaN, and so
    must the elements of the mask nan_where (the fused renderer outside its domain); every other one is held to bound().
    -> dict(bad = mask of the elements that miss, ulps = |err| / ulp32(true), ratio = |err| / bound; the last two 0 where NaN is
    the answer)"""
    got64 = np.asarray(got).astype(np.float64)
    a64 = np.asarray(a).astype(np.float64)
    want_nan = ~np.isfinite(a64) | nan_where
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got64 - true)
        b = bound(a64, true)
        miss = np.where(want_nan, ~np.isnan(got64), ~(err <= b))
        ulps = np.where(want_nan, 0.0, err / ulp32(true))
        ratio = np.where(want_nan, 0.0, err / b)
    return dict(bad=miss, ulps=ulps, ratio=ratio)


@functools.lru_cache(maxsize=2)
def reference(L):
    """(x, a [L, n], sin [L, n], cos [L, n]) of args(L): computed once, shared, never written"""
    x = args(L)
    a = band_args(x, L)
    s, c = true_sincos(a)
    for v in (a, s, c):
        v.setflags(write=False)
    return x, a, s, c


# ---- networks that copy encoding columns to the output -----------------------------------------------------------------------
def select_net(L, cols, output_ch=32, W=64):
    """A network without view directions whose output j is encoding column cols[j], exactly: pts_linears.0 unit 2 j reads the
    column with weight +1 and unit 2 j + 1 with -1, pts_linears.1 is the identity, output_linear row j is h[2 j] - h[2 j + 1] =
    relu(e) - relu(-e) = e; every bias 0.  In fp32 every product is 1 e or 0 e and every sum has one non-zero term."""
    C = 3 + 6 * L
    assert len(cols) <= output_ch and 2 * output_ch <= W and all(0 <= c < C for c in cols)
    w0, w1, wo = np.zeros((W, C), f32), np.eye(W, dtype=f32), np.zeros((output_ch, W), f32)
    for j, c in enumerate(cols):
        w0[2 * j, c], w0[2 * j + 1, c] = 1.0, -1.0
        wo[j, 2 * j], wo[j, 2 * j + 1] = 1.0, -1.0
    return {"pts_linears.0.weight": w0, "pts_linears.0.bias": np.zeros(W, f32), "pts_linears.1.weight": w1,
            "pts_linears.1.bias": np.zeros(W, f32), "output_linear.weight": wo, "output_linear.bias": np.zeros(output_ch, f32),
            "views_linears.0.weight": np.zeros((W // 2, W), f32), "views_linears.0.bias": np.zeros(W // 2, f32)}


def select_nets(L, output_ch=32):
    """[(columns, state dict)] covering the 3 + 6 L columns in groups of output_ch (L = 15: 93 columns, three networks)"""
    C = 3 + 6 * L
    groups = [list(range(lo, min(lo + output_ch, C))) for lo in range(0, C, output_ch)]
    return [(g, select_net(L, g, output_ch)) for g in groups]


# ---- the device formulas in numpy, and five wrong versions --------------------------------------------------------------------
VARIANTS = ("sign", "swap", "f32-reduction", "degree-7", "fast-beyond")


def _fma(x, y, z):
    """fp32 fma of fp32 operands: the product is exact in float64, the sum rounds there once and once more to fp32"""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f32)


def emulate(a, wrong=None):
    """(sin, cos) of the fp32 arguments a by sincos_enc's formulas (csrc/nsr_wide.hip), fp32 where the device is and fp64 where it
    is; wrong: one of VARIANTS -- the n & 2 sign dropped, sin and cos not swapped for odd n, the reduction in fp32, the sine's
    degree-7 coefficient dropped, the fast path beyond 2^24 as well.  (A restatement for the controls: the fma rounds twice.)"""
    assert wrong is None or wrong in VARIANTS
    a = np.asarray(a, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        if wrong == "f32-reduction":
            t = (a * f32(TWO_OVER_PI)).astype(f32)
            nf = np.rint(t)
            f = (t - nf).astype(f32)
            r = (f * f32(PI_OVER_2)).astype(f32)
            n = np.where(np.isfinite(nf), nf, 0).astype(np.int64)
        else:
            magic = 6755399441055744.0
            t = a.astype(np.float64) * TWO_OVER_PI
            tm = t + magic
            n = tm.view(np.int64) & 0xffffffff                                         # __double2loint
            f = t - (tm - magic)
            r = (f * PI_OVER_2).astype(f32)
        z = (r * r).astype(f32)
        ps = _fma(np.full_like(z, 0.0 if wrong == "degree-7" else -1.9515295891e-4), z, np.full_like(z, 8.3321608736e-3))
        ps = _fma(ps, z, np.full_like(z, -1.6666654611e-1))
        ps = _fma((ps * z).astype(f32), r, r)
        pc = _fma(np.full_like(z, 2.443315711809948e-5), z, np.full_like(z, -1.388731625493765e-3))
        pc = _fma(pc, z, np.full_like(z, 4.166664568298827e-2))
        pc = _fma((pc * z).astype(f32), z, _fma(np.full_like(z, -0.5), z, np.ones_like(z)))
        odd = (n & 1).astype(bool) & (wrong != "swap")
        vs, vc = np.where(odd, pc, ps), np.where(odd, ps, pc)
        if wrong != "sign":
            vs = np.where(n & 2, -vs, vs)
            vc = np.where((n + 1) & 2, -vc, vc)
        fast = (np.abs(a) < f32(SWITCH)) | ((wrong == "fast-beyond") & np.isfinite(a))
        ts, tc = true_sincos(a)
        return np.where(fast, vs, ts.astype(f32)).astype(f32), np.where(fast, vc, tc.astype(f32)).astype(f32)


def touched(a, wrong):
    """mask of the arguments a wrong variant computes by other formulas than the right one"""
    a64 = np.abs(np.asarray(a).astype(np.float64))
    return np.isfinite(a64) & ((a64 >= SWITCH) if wrong == "fast-beyond" else (a64 < SWITCH))
