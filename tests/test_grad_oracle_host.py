"""CPU checks of the fp64 autograd oracle of the layered gradient call (oracle/grad_oracle.py) and of the fixtures the GPU test
tests/test_gpu_wide_grad_oracle.py holds the kernels to it on -- so that the GPU test cannot go hollow.

The bound of the GPU test is per ray and has no percentile: on every CERTIFIED ray the floored relative error of
[grad_o | grad_d | grad_viewdirs] against the float64 oracle is at most FACTOR x E32, E32 being the largest error of the SAME graph
differentiated by torch in float32 over the certified rays of the case.  A ray is certified by float64 reference quantities only
(`certified`): no relu'd unit of any of its points within vjp_census.MARGIN of its kink, no density within SIGMA_MARGIN of the
density relu's, a row that is no small remainder of cancelling terms (ROW_MIN), and on the signed-density fixtures every pass that
is differentiated either empty (acc = 0, decided by the density margin: disp = 0 / 0 in every evaluation) or neither nearly empty
nor opaque and carried by two samples (_pass_ok: disp = depth / acc and d acc are no cancellations there).  The networks are small
enough that most rays qualify, and this module asserts it: at least half of every case's rays are certified, and where the
cotangent is acc's at least a quarter of those carry a gradient above the row floor.

E32 below is the table the GPU test reads; test_the_yardstick recomputes it.  It is a maximum of float32 rounding errors whose
association order belongs to the host's BLAS and vector width -- between two hosts the figures of this table differed by factors of
0.6 to 2.5 --, so the recomputed figure is held to the table within a factor of BAND either way, and to the conditioning cap
E32_CAP; the GPU bound comes from the table alone."""
import functools

import numpy as np
import pytest
import torch

import grad_oracle as G
from conftest import assert_close, load_golden
from test_gpu_output_grads import FLOOR, _check, _rel_rows
from test_gpu_wide_tiles import _cots
from wide_onchip_cases import EXTRA, SIGNED
from wide_onchip_cases import TRUNK_NETS as NETS
from wide_onchip_cases import bwd_nets as _nets
from wide_onchip_cases import signed_nets as _signed_nets
from test_output_grads_host import case_nets

NETWORKS = sorted(NETS) + sorted(EXTRA)
N_RAYS, NS, NI = 256, 3, 2
RAY_SEED, COT_SEED = 21, 57
FACTOR = 16                 # the GPU bound is FACTOR x E32: summation order (a small factor) x f16x2's 22-bit operand split (4)
BAND = 3.0                  # see the module docstring
E32_CAP = 1e-5              # a case whose float32 autograd is further than this from float64 is badly conditioned
SIGMA_MARGIN = 1e-3         # |sigma| / max |sigma|: the density relu's kink, and with it emptiness and opacity (the 1e10 last distance)
ACC_MIN, ACC_MAX = 0.15, 0.95   # signed fixtures: a pass's acc is 0 (empty, by SIGMA_MARGIN) or within these (_pass_ok) ...
W_MIN = 0.1                 # ... and at least two of its samples weigh this share of acc
# a row far below the typical one is a sum of per-sample contributions that cancel, and its relative error the others' times typical /
# row: a certified row is at least this share of the median row that is not zero, or exactly zero or NaN (an empty pass)
ROW_MIN = 0.25
COND = 2.5e-6                # a ray is chosen for a fixture only if float32 autograd is this close to float64 on it (`rays`)
POOL, N_EMPTY = 128, 16     # signed fixtures: the image the rays are chosen from (`rays`), the empty rays of either pass among them
# 3x40-L15 encodes up to sin(2^14 x): the fp32 rounding of a point x = o + d z of size 1 moves that phase by 1e-3, and no choice
# of rays makes the gradient of such a scene a sharp thing to compare.  Its scene is 2^-10 the size (rays_o and rays_d scaled, an
# exact operation; densities x 2^10 to keep sigma x distance): the 96 encoding columns stay, the top bands see phases of order 1
RAY_SCALE = {"3x40-L15": 2.0 ** -10}
FOUR = ("rgb_map", "disp_map", "rgb0", "disp0")
# fixture -> cotangent set -> (outputs, white_bkgd)
COTS = {"translucent": {"rgb_map": (("rgb_map",), False), "disp_map": (("disp_map",), False), "rgb0": (("rgb0",), False),
                        "disp0": (("disp0",), False), "four": (FOUR, False)},
        "signed": {"acc_map": (("acc_map",), False), "acc0": (("acc0",), False), "disp_map": (("disp_map",), False),
                   "disp0": (("disp0",), False), "six": (G.OUTS, False), "rgb_white": (("rgb_map",), True)}}
ACC_SETS = ("acc_map", "acc0", "rgb_white")
# variants of a case: view directions given as an input of their own, lindisp depths, a coarse-only handle
VARIANT_CASES = [("3x40", "translucent", "four", "viewdirs"), ("3x128", "signed", "six", "viewdirs"), ("5x100", "translucent", "four", "viewdirs"),
                 ("3x100", "translucent", "four", "lindisp"), ("3x40", "signed", "six", "coarse-only"),
                 ("3x100", "translucent", "four", "coarse-only")]
CASES = [(n, f, c, "") for n in NETWORKS for f in COTS for c in COTS[f]] + VARIANT_CASES
# the deliberately wrong backward (grad_oracle.MUTATIONS) -> the case whose certified rays show it beyond the GPU bound
TEETH = {"no_dists_norm": ("3x40", "translucent", "rgb_map", ""), "no_dir_jacobian": ("3x100", "translucent", "rgb0", ""),
         "no_skip_grad": ("5x100", "translucent", "four", ""), "views_relu_all_on": ("3x128", "translucent", "rgb_map", ""),
         "sigma_relu_all_on": ("3x40", "signed", "acc_map", ""), "white_no_sum": ("3x24", "signed", "rgb_white", ""),
         "untransposed": ("2x128", "translucent", "disp_map", "")}

# E32: "network/fixture/cotangents[/variant]" -> the yardstick (see the module docstring; written from test_the_yardstick's output)
E32 = {
    "2x128/translucent/rgb_map": 1.8e-06, "2x128/translucent/disp_map": 5.0e-07, "2x128/translucent/rgb0": 1.4e-06,
    "2x128/translucent/disp0": 4.2e-07, "2x128/translucent/four": 1.2e-06, "2x128/signed/acc_map": 1.0e-06,
    "2x128/signed/acc0": 8.3e-07, "2x128/signed/disp_map": 2.5e-06, "2x128/signed/disp0": 2.1e-06, "2x128/signed/six": 2.9e-06,
    "2x128/signed/rgb_white": 1.3e-06, "3x100/translucent/rgb_map": 2.3e-06, "3x100/translucent/disp_map": 3.9e-07,
    "3x100/translucent/rgb0": 2.4e-06, "3x100/translucent/disp0": 4.0e-07, "3x100/translucent/four": 1.1e-06,
    "3x100/signed/acc_map": 8.2e-07, "3x100/signed/acc0": 9.5e-07, "3x100/signed/disp_map": 1.3e-06,
    "3x100/signed/disp0": 2.6e-06, "3x100/signed/six": 4.8e-06, "3x100/signed/rgb_white": 9.4e-07,
    "3x128/translucent/rgb_map": 1.9e-06, "3x128/translucent/disp_map": 4.3e-07, "3x128/translucent/rgb0": 1.5e-06,
    "3x128/translucent/disp0": 4.2e-07, "3x128/translucent/four": 1.4e-06, "3x128/signed/acc_map": 7.1e-07,
    "3x128/signed/acc0": 2.5e-06, "3x128/signed/disp_map": 1.5e-06, "3x128/signed/disp0": 2.9e-06, "3x128/signed/six": 3.4e-06,
    "3x128/signed/rgb_white": 1.0e-06, "3x24/translucent/rgb_map": 1.5e-06, "3x24/translucent/disp_map": 4.2e-07,
    "3x24/translucent/rgb0": 1.6e-06, "3x24/translucent/disp0": 4.8e-07, "3x24/translucent/four": 8.2e-07,
    "3x24/signed/acc_map": 9.2e-07, "3x24/signed/acc0": 2.4e-06, "3x24/signed/disp_map": 1.6e-06, "3x24/signed/disp0": 1.3e-06,
    "3x24/signed/six": 2.0e-06, "3x24/signed/rgb_white": 1.1e-06, "3x40/translucent/rgb_map": 9.6e-07,
    "3x40/translucent/disp_map": 5.1e-07, "3x40/translucent/rgb0": 1.5e-06, "3x40/translucent/disp0": 4.4e-07,
    "3x40/translucent/four": 8.4e-07, "3x40/signed/acc_map": 1.6e-06, "3x40/signed/acc0": 1.1e-06,
    "3x40/signed/disp_map": 2.1e-06, "3x40/signed/disp0": 2.6e-06, "3x40/signed/six": 2.6e-06, "3x40/signed/rgb_white": 1.2e-06,
    "3x40-noviews/translucent/rgb_map": 2.7e-06, "3x40-noviews/translucent/disp_map": 4.9e-07,
    "3x40-noviews/translucent/rgb0": 2.3e-06, "3x40-noviews/translucent/disp0": 5.4e-07,
    "3x40-noviews/translucent/four": 2.7e-06, "3x40-noviews/signed/acc_map": 1.0e-06, "3x40-noviews/signed/acc0": 9.0e-07,
    "3x40-noviews/signed/disp_map": 3.6e-06, "3x40-noviews/signed/disp0": 2.7e-06, "3x40-noviews/signed/six": 3.2e-06,
    "3x40-noviews/signed/rgb_white": 3.9e-06, "5x100/translucent/rgb_map": 1.5e-06, "5x100/translucent/disp_map": 4.7e-07,
    "5x100/translucent/rgb0": 2.0e-06, "5x100/translucent/disp0": 4.8e-07, "5x100/translucent/four": 1.7e-06,
    "5x100/signed/acc_map": 1.5e-06, "5x100/signed/acc0": 1.4e-06, "5x100/signed/disp_map": 3.0e-06,
    "5x100/signed/disp0": 1.2e-06, "5x100/signed/six": 3.8e-06, "5x100/signed/rgb_white": 1.1e-06,
    "3x100-L0/translucent/rgb_map": 1.9e-06, "3x100-L0/translucent/disp_map": 4.7e-07, "3x100-L0/translucent/rgb0": 2.2e-06,
    "3x100-L0/translucent/disp0": 3.4e-07, "3x100-L0/translucent/four": 2.1e-06, "3x100-L0/signed/acc_map": 8.6e-07,
    "3x100-L0/signed/acc0": 1.1e-06, "3x100-L0/signed/disp_map": 1.6e-06, "3x100-L0/signed/disp0": 3.3e-06,
    "3x100-L0/signed/six": 3.5e-06, "3x100-L0/signed/rgb_white": 9.1e-07, "3x40-L15/translucent/rgb_map": 1.6e-06,
    "3x40-L15/translucent/disp_map": 6.0e-07, "3x40-L15/translucent/rgb0": 2.4e-06, "3x40-L15/translucent/disp0": 4.4e-07,
    "3x40-L15/translucent/four": 1.3e-06, "3x40-L15/signed/acc_map": 2.3e-06, "3x40-L15/signed/acc0": 7.4e-07,
    "3x40-L15/signed/disp_map": 2.2e-06, "3x40-L15/signed/disp0": 2.6e-06, "3x40-L15/signed/six": 4.4e-06,
    "3x40-L15/signed/rgb_white": 2.6e-06, "3x40/translucent/four/viewdirs": 8.1e-07, "3x128/signed/six/viewdirs": 3.5e-06,
    "5x100/translucent/four/viewdirs": 1.7e-06, "3x100/translucent/four/lindisp": 9.3e-07,
    "3x40/signed/six/coarse-only": 2.7e-06, "3x100/translucent/four/coarse-only": 1.5e-06,
}


def key(name, fixture, cotname, variant=""):
    return "/".join(x for x in (name, fixture, cotname, variant) if x)


def fixture_nets(oracle, name, fixture):
    """(coarse, fine) of a fixture: wide_onchip_cases.bwd_nets or .signed_nets, the density rows x 1 / RAY_SCALE"""
    nets = (_nets if fixture == "translucent" else _signed_nets)(oracle, name)
    if name not in RAY_SCALE:
        return nets
    out = []
    for sd in nets:
        sd = {k: v.copy() for k, v in sd.items()}
        sd["alpha_linear.weight"] *= np.float32(1.0 / RAY_SCALE[name])
        sd["alpha_linear.bias"] *= np.float32(1.0 / RAY_SCALE[name])
        out.append(sd)
    return tuple(out)


def cotangents(fixture, cotname, variant="", n=N_RAYS):
    """({output: cotangent}, white_bkgd) of a case; a coarse-only handle has the last pass's three outputs"""
    outs, white = COTS[fixture][cotname]
    if variant == "coarse-only":
        outs = tuple(k for k in outs if not k.endswith("0"))
    cots = _cots(n, COT_SEED)
    return {k: cots[k] for k in outs}, white


@functools.lru_cache(maxsize=None)
def _pool(oracle):
    """the POOL x POOL image of the pose of test_gpu_wide_tiles._rays, in a seeded order"""
    pose = np.asarray(oracle.sweep_poses(1, seed=9))[0]
    ro, rd = (a.reshape(-1, 3) for a in oracle.get_rays(POOL, POOL, oracle.scaled_K(400.0 / POOL), pose[:3, :4]))
    sel = np.random.RandomState(RAY_SEED).permutation(len(ro))
    return np.ascontiguousarray(ro[sel]), np.ascontiguousarray(rd[sel])


def _z_fine(oracle, sd_c, sd_f, ro, rd, lindisp=False):
    return oracle.render_rays(sd_c, sd_f, ro, rd, oracle.normalize_dirs(rd), oracle.YCBV_NEAR, oracle.YCBV_FAR, NS, NI, extras=True,
                              lindisp=lindisp)["z_fine"]


def _pass_ok(acc, weights):
    """a pass of a ray on a signed fixture: empty, or neither nearly empty nor opaque and with two samples that count"""
    with np.errstate(invalid="ignore", divide="ignore"):
        two = (weights >= W_MIN * acc[:, None]).sum(1) >= 2
    return (acc == 0) | ((acc >= ACC_MIN) & (acc <= ACC_MAX) & two)


@functools.lru_cache(maxsize=None)
def rays(oracle, name, fixture):
    """The 256 rays of a fixture (x RAY_SCALE), chosen from _pool by torch alone.  With densities of either sign most rays of an
    image are opaque at their last sample (the distance 1e10: acc = 1, its gradient a cancellation), empty, or carried by one sample
    (disp = 1 / z of that sample, its gradient a cancellation), and on the deeper networks half of the rays have a relu without its
    margin.  A fixture is the first rays of the pool that are certified for all of its outputs on the float64 reference (`certified`)
    and whose gradient is well conditioned for every cotangent set -- measured: float32 autograd within COND of float64 autograd on
    that ray, relative to the row itself --; a signed fixture has 2 * N_EMPTY of its 256 rays from those whose coarse pass, or
    whose fine pass, is empty (disp = 0 / 0: NaN rows that must coincide).  The choice makes the ray set, and keeps the yardstick
    E32 near COND on any host; whether a ray is certified is decided afresh, from float64 quantities only, wherever the set is used."""
    s = np.float32(RAY_SCALE.get(name, 1.0))
    signed = fixture == "signed"
    ro, rd = (x[:len(x) if signed else 8 * N_RAYS] * s for x in _pool(oracle))
    sd_c, sd_f = fixture_nets(oracle, name, fixture)
    both = "six" if signed else "four"
    ref = G.render_rays_grad(sd_c, sd_f, ro, rd, G.coarse_depths(len(ro), oracle.YCBV_NEAR, oracle.YCBV_FAR, NS),
                             _z_fine(oracle, sd_c, sd_f, ro, rd), cotangents(fixture, both, n=len(ro))[0])
    ok = certified(ref, fixture, both)
    e0, e1 = ref["acc0"] == 0, ref["acc_map"] == 0
    n_empty = N_EMPTY if signed else 0
    groups = [np.flatnonzero(ok & ~e0 & ~e1)[:4 * N_RAYS], np.flatnonzero(ok & e0 & ~e1)[:4 * n_empty], np.flatnonzero(ok & e1 & ~e0)[:4 * n_empty]]
    cand = np.concatenate(groups)
    keep = np.ones(len(cand), bool)
    zc, zf = G.coarse_depths(len(cand), oracle.YCBV_NEAR, oracle.YCBV_FAR, NS), _z_fine(oracle, sd_c, sd_f, ro[cand], rd[cand])
    for cotname in COTS[fixture]:
        cots, white = cotangents(fixture, cotname, n=len(cand))
        a, b = (G.stacked(G.render_rays_grad(sd_c, sd_f, ro[cand], rd[cand], zc, zf, cots, white_bkgd=white, dtype=t))
                for t in (torch.float32, torch.float64))
        with np.errstate(invalid="ignore"):
            keep &= ~(np.linalg.norm(a - b, axis=1) > COND * np.linalg.norm(b, axis=1))          # (a NaN row of an empty pass stays)
    take = np.concatenate([g[np.isin(g, cand[keep])][:n] for g, n in zip(groups, (N_RAYS - 2 * n_empty, n_empty, n_empty))])
    rest = np.setdiff1d(np.arange(len(ro)), take)[:N_RAYS - len(take)]          # (a pool short of such rays: the caps will say so)
    sel = np.sort(np.concatenate([take, rest]))
    return np.ascontiguousarray(ro[sel]), np.ascontiguousarray(rd[sel])


@functools.lru_cache(maxsize=None)
def host_z_fine(oracle, name, fixture, lindisp=False):
    """the fine depths of the oracle's own fp32 forward (the GPU test takes each handle's own instead)"""
    return _z_fine(oracle, *fixture_nets(oracle, name, fixture), *rays(oracle, name, fixture), lindisp=lindisp)


def reference(oracle, name, fixture, cotname, variant="", z_fine=None, dtype=torch.float64, mutate=None, scale=1.0):
    """grad_oracle.render_rays_grad of a case at z_fine (default: host_z_fine)"""
    sd_c, sd_f = fixture_nets(oracle, name, fixture)
    ro, rd = rays(oracle, name, fixture)
    cots, white = cotangents(fixture, cotname, variant)
    lindisp = variant == "lindisp"
    if variant == "coarse-only":
        sd_f, z_fine = None, None
    elif z_fine is None:
        z_fine = host_z_fine(oracle, name, fixture, lindisp)
    zc = G.coarse_depths(N_RAYS, oracle.YCBV_NEAR, oracle.YCBV_FAR, NS, lindisp)
    vd = oracle.normalize_dirs(rd) if variant == "viewdirs" else None
    return G.render_rays_grad(sd_c, sd_f, ro, rd, zc, z_fine, {k: v * np.float32(scale) for k, v in cots.items()}, viewdirs=vd,
                              white_bkgd=white, dtype=dtype, mutate=mutate)


def certified(ref, fixture, cotname):
    """[N] bool from a float64 reference's own quantities (see the module docstring): the margins, and on a signed fixture _pass_ok
    of every pass that has an output among the cotangents"""
    ok = (ref["relu_margin"] > G.MARGIN) & (ref["sigma_margin"] > SIGMA_MARGIN)
    if fixture == "signed":
        outs = COTS[fixture][cotname][0]
        if "acc0" in ref and any(k.endswith("0") for k in outs):
            ok &= _pass_ok(ref["acc0"], ref["weights0"])
        if "acc0" not in ref or any(k.endswith("_map") for k in outs):
            ok &= _pass_ok(ref["acc_map"], ref["weights"])
    if "grad_o" in ref:
        with np.errstate(invalid="ignore"):
            nb = np.linalg.norm(G.stacked(ref), axis=1)
            ok &= ~(nb < ROW_MIN * np.nanmedian(nb[nb > 0])) | (nb == 0)
    return ok


def ray_errors(got, ref, ok):
    """got: [N, 6 or 9] rows of another evaluation, ref: the float64 reference.  On the certified rays NaN rows must coincide; returns
    the floored relative error (_rel_rows) of the finite certified rows, their ray indices and how many sit above the floor."""
    want = G.stacked(ref)
    got = np.asarray(got, np.float64)
    nan_g, nan_w = np.isnan(got).any(1), np.isnan(want).any(1)
    assert np.array_equal(nan_g[ok], nan_w[ok]), "NaN rows %s vs the reference's %s" % (np.flatnonzero(nan_g & ok), np.flatnonzero(nan_w & ok))
    idx = np.flatnonzero(ok & ~nan_w)
    assert np.isfinite(got[idx]).all()
    nb = np.linalg.norm(want[idx], axis=1)
    return _rel_rows(got[idx], want[idx]), idx, int((nb >= FLOOR * nb.max()).sum())


@functools.lru_cache(maxsize=None)
def measured(oracle, name, fixture, cotname, variant):
    """(certified share, finite certified rays, of them above the floor, E32) of a case at the host's depths"""
    r64 = reference(oracle, name, fixture, cotname, variant)
    r32 = reference(oracle, name, fixture, cotname, variant, dtype=torch.float32)
    ok = certified(r64, fixture, cotname)
    e, idx, above = ray_errors(G.stacked(r32), r64, ok)
    return int(ok.sum()), len(idx), above, float(e.max())


def test_the_oracle_agrees_with_the_handwritten_backprop_to_float64_rounding(oracle):
    """oracle.render_rays_vjp(exact=True) is the hand-written float64 backprop of rgb_map on the same float64 forward.  A gradient
    entry is a sum over <= 5 samples of a chain of <= 8 matrix products of <= 160 terms: (8 x 160 + 5) roundings of 1.1e-16, 1.4e-13
    of the sum of the terms' magnitudes, which the floor of _rel_rows lets exceed the row by at most 1 / FLOOR = 1e3: 1.4e-10."""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    worst = 0.0
    for name, fixture, cotname, variant in [(n, "translucent", "rgb_map", "") for n in NETWORKS] + \
            [("3x40", "signed", "rgb_white", ""), ("3x128", "translucent", "rgb_map", "viewdirs")]:
        sd_c, sd_f = fixture_nets(oracle, name, fixture)
        ro, rd = rays(oracle, name, fixture)
        zf = host_z_fine(oracle, name, fixture)
        cots, white = cotangents(fixture, cotname)
        ref = reference(oracle, name, fixture, cotname, variant)
        parts = {}
        oracle.render_rays_vjp(sd_c, sd_f, ro, rd, near, far, cots["rgb_map"], NS, NI, z_fine=zf, white_bkgd=white, parts=parts,
                               exact=True, viewdirs=oracle.normalize_dirs(rd) if variant else None)
        hand = np.concatenate([parts[k] for k in ("grad_o", "grad_d", "grad_v") if k in parts], 1)
        e = _rel_rows(G.stacked(ref), hand)
        worst = max(worst, e.max())
        assert e.max() < 1.4e-10, (name, fixture, cotname, variant, e.max())
    print("autograd against the hand-written float64 backprop: %.1e" % worst)


@pytest.mark.parametrize("fixture", sorted(COTS))
def test_the_oracles_forward_is_render_rays(fixture, oracle):
    """all six outputs against oracle.render_rays (numpy fp32) with the bounds of test_output_grads_host: sums of <= 5 weights in
    [0, 1] to a few fp32 ulp (3e-6), disp to 1e-4 relative, NaN in the same places"""
    for name in NETWORKS:
        for white in ((False, True) if fixture == "signed" else (False,)):
            sd_c, sd_f = fixture_nets(oracle, name, fixture)
            ro, rd = rays(oracle, name, fixture)
            want = oracle.render_rays(sd_c, sd_f, ro, rd, oracle.normalize_dirs(rd), oracle.YCBV_NEAR, oracle.YCBV_FAR, NS, NI,
                                      extras=True, white_bkgd=white)
            ref = reference(oracle, name, fixture, "rgb_white" if white else "disp_map", z_fine=want["z_fine"])
            ok = certified(ref, fixture, "six" if fixture == "signed" else "four")
            for k in G.OUTS:
                if k.startswith("disp"):
                    assert np.array_equal(np.isnan(ref[k])[ok], np.isnan(want[k])[ok]), (name, k)
                    assert_close(ref[k][ok], want[k][ok], rtol=1e-4, atol=1e-6, what="%s %s" % (name, k))
                else:
                    assert_close(ref[k], want[k], atol=3e-6, what="%s %s" % (name, k))


@pytest.mark.parametrize("tag", "acde")
def test_the_oracle_against_the_references_own_autograd(tag, oracle):
    """g28 (8 x 256 at 64 + 128 samples, the reference's fp32 autograd; c: white_bkgd, d: coarse only, e: empty rays, NaN): every
    output alone and all together within the bounds test_gpu_output_grads holds the kernels to on that file"""
    from test_gpu_output_grads import P90, P90_DISP_ACC, _outs
    g = load_golden("g28_output_grads")
    sd_c, sd_f, white = case_nets(oracle, g, tag)
    ns, ni, _ = (int(x) for x in g[tag + "_shape"])
    ro, rd = g[tag + "_rays_o"], g[tag + "_rays_d"]
    zc = G.coarse_depths(len(ro), oracle.YCBV_NEAR, oracle.YCBV_FAR, ns)
    outs = _outs(g, tag)
    for k in (["all"] if tag in "ac" else outs + ["all"]):
        cot = {o: g["%s_cot_%s" % (tag, o)] for o in (outs if k == "all" else [k])}
        ref = G.render_rays_grad(sd_c, sd_f, ro, rd, zc, g[tag + "_z_fine"] if ni > 0 else None, cot, white_bkgd=white)
        bound = P90 if k in ("rgb_map", "rgb0") else P90_DISP_ACC
        _check("%s %s grad_o" % (tag, k), ref["grad_o"], g["%s_grad_o_%s" % (tag, k)], p90_bound=bound)
        _check("%s %s grad_d" % (tag, k), ref["grad_d"], g["%s_grad_d_%s" % (tag, k)], p90_bound=bound)


def test_the_signed_fixtures_vary_acc(oracle):
    """every network has a signed variant, and on it acc_map and acc0 are strictly between ACC_MIN and 0.999 on a quarter of the rays
    (on the translucent fixtures: on none -- which is why acc's cotangents live here)"""
    assert sorted(SIGNED) == sorted(NETWORKS)
    for name in NETWORKS:
        ref = reference(oracle, name, "signed", "six")
        flat = reference(oracle, name, "translucent", "four")
        for k in ("acc_map", "acc0"):
            n = int(((ref[k] > ACC_MIN) & (ref[k] < 0.999)).sum())
            assert n >= N_RAYS // 4, (name, k, n)
            assert not (flat[k] < 0.999).any(), (name, k)


@pytest.mark.parametrize("name", NETWORKS)
def test_the_caps(name, oracle):
    """at least half of the rays certified in every case; where acc is differentiated, at least a quarter of the certified rays
    above the row floor"""
    for n, fixture, cotname, variant in CASES:
        if n != name:
            continue
        cert, finite, above, _ = measured(oracle, n, fixture, cotname, variant)
        print("%-36s certified %3d of %d, finite %3d, above the floor %3d" % (key(n, fixture, cotname, variant), cert, N_RAYS, finite, above))
        assert 2 * cert >= N_RAYS, (n, fixture, cotname, variant, cert)
        if cotname in ACC_SETS:
            assert 4 * above >= cert, (n, fixture, cotname, variant, above, cert)


@pytest.mark.parametrize("name", NETWORKS)
def test_the_yardstick(name, oracle):
    """E32 of every case: within the conditioning cap, and the table of this module is what this test computes"""
    for n, fixture, cotname, variant in CASES:
        if n != name:
            continue
        k = key(n, fixture, cotname, variant)
        e32 = measured(oracle, n, fixture, cotname, variant)[3]
        print('    "%s": %.1e,' % (k, e32))
        assert e32 <= E32_CAP, (k, e32)
        assert E32[k] / BAND <= e32 <= BAND * E32[k], (k, e32, E32[k])
    assert len(E32) == len(CASES)


@pytest.mark.parametrize("mutation", sorted(G.MUTATIONS))
def test_teeth(mutation, oracle):
    """a float64 reference with one term of the backward wrong is further than the GPU bound from the right one on at least a
    quarter of the certified rays of TEETH[mutation]: the fixtures exercise the path, and the bound would notice its loss"""
    name, fixture, cotname, variant = TEETH[mutation]
    ref = reference(oracle, name, fixture, cotname, variant)
    bad = reference(oracle, name, fixture, cotname, variant, mutate=mutation)
    ok = certified(ref, fixture, cotname)
    e, idx, _ = ray_errors(G.stacked(bad), ref, ok)
    caught = int((e > FACTOR * E32[key(name, fixture, cotname, variant)]).sum())
    print("%s on %s: beyond the bound on %d of %d certified rays (median error %.1e)" % (mutation, key(name, fixture, cotname, variant),
                                                                                       caught, ok.sum(), np.median(e)))
    assert 4 * caught >= ok.sum(), (mutation, caught, int(ok.sum()))
    assert sorted(TEETH) == sorted(G.MUTATIONS)
