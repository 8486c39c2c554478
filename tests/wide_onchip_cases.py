"""The networks, rays and reusable bodies of the GPU tests of the layered renderer's on-chip forms (tests/test_gpu_wide_{trunk,heads,
trunk256,trunk_bwd}.py; DESIGN.md 8 has the table of forms) and of the gradient oracle's tests, which run on the same networks.  Every
form is held to one claim -- the bits of the per-layer path -- so every file asks the same questions of its own handles: every tap
equal, a range event re-runs the pass, hostile rays, a ray's result depends on nothing but the ray, capture and replay, and the
bounds-checked build.  The questions are stated here once."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np

from conftest import assert_close
from test_gpu_wide_tiles import OUTS, POINTS, TAPS, _cots, _rays, _same, cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_PTS, L_VIEWS = 4, 2
COARSE_TAPS = ("rgb0", "acc0", "weights0", "raw0", "inds", "z_samples", "z_fine")

# ---- the 128-row trunk's networks: name -> (D, W, skips, use_viewdirs).  3 x W with one skip after layer 0 or 1 in turn (NJ = 1: 24,
# 40; NJ = 2: 100, 128 -- a width below, at and off the 32-column blocks of either form), two skips, no skip at the full 128 columns,
# and a network without view directions (output_linear behind the trunk instead of the feature / alpha heads)
TRUNK_NETS = {"3x24": (3, 24, [0], True), "3x40": (3, 40, [1], True), "3x100": (3, 100, [0], True), "3x128": (3, 128, [1], True),
              "5x100": (5, 100, [0, 2], True), "2x128": (2, 128, [], True), "3x40-noviews": (3, 40, [0], False)}
# At W = 24 the trunk's activations are large against the fixed density bias (synth_weights_shape scales the trunk by sqrt(256 / W)) and
# most seeds give rays with an empty stretch (disp = 0 / 0 in the reference too); these two keep the density above 0.15 everywhere
# between near and far on the rays used here (checked with the oracle's run_network)
TRUNK_SEEDS = {"3x24": (301, 305)}
# ---- the heads' networks: name -> (D, W, skips, multires_views or None for a network without view directions, the trunk's name of
# the same network or None, seeds).  3x66: Wp = 96 is three column blocks of the four in feature_linear's image, W2 = 33 makes
# views_linears.0 two column blocks wide (W2p = 64), and Cv = 64; 2x64-v15: Cv = 96, the widest direction encoding; 3x40-noviews:
# output_linear.  The seeds of the networks that are new here keep the density above 0.15 everywhere between near and far on the rays
# used (checked with the oracle's run_network, as for the trunk's 3x24).
HEADS_NETS = {"3x24": (3, 24, [0], 2, "3x24", None), "3x40-v4": (3, 40, [1], 4, None, (505, 601)), "3x66-v6": (3, 66, [0], 6, None, (502, 602)),
              "3x100": (3, 100, [0], 2, "3x100", None), "3x128-v4": (3, 128, [1], 4, None, (503, 603)),
              "2x64-v15": (2, 64, [], 15, None, (504, 604)), "2x128": (2, 128, [], 2, "2x128", None),
              "3x40-noviews": (3, 40, [0], None, "3x40-noviews", None)}
# ---- the wide form's networks: name -> (D, W, skips, use_viewdirs).  Padded widths 160 (five column blocks computed, six in the
# weight image: the last quarter of the workgroup idles), 192 (six and six), 224 (seven of eight) and 256; the skip after layer 0 or
# 1, two skips, none; a network without view directions (output_linear behind the trunk)
WIDE_NETS = {"3x136": (3, 136, [1], True), "3x192": (3, 192, [0], True), "3x200": (3, 200, [1], True), "3x256": (3, 256, [1], True),
             "5x256": (5, 256, [0, 2], True), "2x256": (2, 256, [], True), "3x160-noviews": (3, 160, [], False)}
NARROW = (3, 40, [1], True)                          # the coarse network of the wide form's mixed handle
# ---- the backward trunk's networks beside TRUNK_NETS: name -> (D, W, skips, multires).  A 96-column encoding on a narrow network
# (NJ = 2 by the encoding alone: its transposed image has three column blocks of weights, the hidden ones two) and the identity
# encoding (one column block, so that the second wave column computes nothing in an encoding row)
EXTRA = {"3x40-L15": (3, 40, [1], 15), "3x100-L0": (3, 100, [0], 0)}
# name -> (scale, bias) of the coarse and of the fine network's density row in the SIGNED-density variant (signed_nets), searched on
# the CPU per network so that many rays of the image have, in both passes, a last sample of negative density behind two that count
# (tests/test_grad_oracle_host.py chooses its rays among them and holds the result to its caps).  SIGNED_ROWS: the seed of a density
# row drawn anew, N(0, 1 / W), where no scaling of the network's own row gives such rays (2 x 128's coarse density falls or rises
# along every ray) or only one so large that the density is a badly conditioned multiple of a cancelling dot product (3x40-L15)
SIGNED = {"2x128": (1.4, 1.2, -27.0, -2.3), "3x100": (28.0, 0.69, -4.1, 0.2), "3x128": (-95.0, -3.6, -6.6, -0.018),
          "3x24": (-7.7, 2.7, 6.1, -0.4), "3x40": (-8.7, -0.094, 5.8, 0.19), "3x40-noviews": (-5.5, -0.45, -8.4, -0.41),
          "5x100": (-3.8, -0.26, 23.0, -0.3), "3x100-L0": (-76.0, 0.099, 6.1, 0.29), "3x40-L15": (0.34, 0.23, 0.31, -0.17)}
SIGNED_ROWS = {"2x128": (1004, None), "3x40-L15": (3002, 4001)}
RANGE_LOG2 = 14             # log2 of the weight that sends one gradient out of fp16's range (bwd_range_nets)


def scaled(oracle, seed, D, W, skips, views, multires=L_PTS, multires_views=L_VIEWS):
    """a synthetic network with the density scaling of test_gpu_wide_tiles._nets: the density row at an eighth of its nn.Linear size
    and its bias +0.5, so that every ray is translucent at 3 + 2 samples (finite disp, gradients through every layer)"""
    sd = oracle.synth_weights_shape(seed, D, W, multires, multires_views, list(skips), views)
    f = np.float32(W / (400.0 * 256.0))
    if views:
        sd["alpha_linear.weight"] = (sd["alpha_linear.weight"] * f).astype(np.float32)
        sd["alpha_linear.bias"] = np.full_like(sd["alpha_linear.bias"], 0.5)
    else:
        sd["output_linear.weight"][3] *= f
        sd["output_linear.bias"][3] = np.float32(0.5)
    return sd


@functools.lru_cache(maxsize=None)
def trunk_nets(oracle, name):
    """(coarse, fine) of TRUNK_NETS[name].  acc = 1 on every ray there (the last sample is dense, its distance 1e10), so acc's
    gradient is rounding noise on these networks: signed_nets is the variant on which it is a gradient."""
    i = sorted(TRUNK_NETS).index(name)
    return tuple(scaled(oracle, s, *TRUNK_NETS[name]) for s in TRUNK_SEEDS.get(name, (300 + i, 400 + i)))


@functools.lru_cache(maxsize=None)
def heads_nets(oracle, name):
    """(coarse, fine) of HEADS_NETS[name]"""
    D, W, skips, Lv, trunk_name, seeds = HEADS_NETS[name]
    if trunk_name:
        return trunk_nets(oracle, trunk_name)
    return tuple(scaled(oracle, s, D, W, skips, True, multires_views=Lv) for s in seeds)


@functools.lru_cache(maxsize=None)
def wide_nets(oracle, name):
    """(coarse, fine) of WIDE_NETS[name]"""
    i = sorted(WIDE_NETS).index(name)
    return tuple(scaled(oracle, s + i, *WIDE_NETS[name]) for s in (500, 600))


@functools.lru_cache(maxsize=None)
def bwd_nets(oracle, name):
    """(coarse, fine) of TRUNK_NETS[name] or EXTRA[name].  Every sample's density is positive here, the last one's too, and the last
    distance is 1e10: acc = 1 on every ray and its gradient is rounding noise -- acc, acc0 and white_bkgd's 1 - acc are gradients on
    signed_nets only."""
    if name in TRUNK_NETS:
        return trunk_nets(oracle, name)
    D, W, skips, multires = EXTRA[name]
    i = sorted(EXTRA).index(name)
    return tuple(scaled(oracle, s, D, W, skips, True, multires=multires) for s in (500 + i, 600 + i))


@functools.lru_cache(maxsize=None)
def signed_nets(oracle, name):
    """bwd_nets(name) with the density rows rescaled and re-biased by SIGNED[name]: densities of either sign, of order 1, so that a ray
    whose last sample is empty behind a translucent one has 0 < acc < 1 (some rays are empty: disp = 0 / 0 there, in the reference
    as well).  The path cot_acc -> d sigma -> network backward carries a gradient on these, not a cancellation."""
    nets = []
    for sd, scale, bias, row in zip(bwd_nets(oracle, name), SIGNED[name][0::2], SIGNED[name][1::2], SIGNED_ROWS.get(name, (None, None))):
        sd = {k: v.copy() for k, v in sd.items()}
        if row is not None:
            w = sd["alpha_linear.weight"]
            w[:] = np.random.RandomState(row).standard_normal(w.shape) / np.sqrt(w.shape[1])
        if "alpha_linear.weight" in sd:
            sd["alpha_linear.weight"] *= np.float32(scale)
            sd["alpha_linear.bias"][:] = np.float32(bias)
        else:
            sd["output_linear.weight"][3] *= np.float32(scale)
            sd["output_linear.bias"][3] = np.float32(bias)
        nets.append(sd)
    return tuple(nets)


def fine_3x136(oracle):
    """the fine network of the mixed handles: padded width 160, which only the wide form takes"""
    return scaled(oracle, 411, 3, 136, [1], True)


def _with_bias(nets, key, delta=7.0e4):
    """(coarse, fine) with unit 5 of the coarse network's bias `key` raised: 7e4 on every point, out of fp16's range"""
    sd_c, sd_f = nets
    sd_c = {k: v.copy() for k, v in sd_c.items()}
    sd_c[key][5] += delta
    return sd_c, sd_f


def trunk_range_nets(oracle, layer, nets=None):
    """3 x 100 coarse network (3 x 200 with nets = the wide form's) whose pts_linears.<layer> bias sends hidden unit 5 to 7e4 on every
    point -- layer 1: the value leaves fp16's range INSIDE the trunk (split for layer 2 in LDS); layer 2: on the trunk's last layer,
    split by the heads behind it"""
    return _with_bias(nets or trunk_nets(oracle, "3x100"), "pts_linears.%d.bias" % layer)


def head_range_nets(oracle, case):
    """3 x 100 coarse network in which unit 5 reaches 7e4 on every point -- "feature": in feature_linear's output, split for
    views_linears.0; "views": in views_linears.0's output, split for rgb_linear; "trunk": on the trunk's last layer (the trunk's
    layer-2 case), split for alpha_linear and feature_linear"""
    if case == "trunk":
        return trunk_range_nets(oracle, 2)
    return _with_bias(trunk_nets(oracle, "3x100"), {"feature": "feature_linear.bias", "views": "views_linears.0.bias"}[case])


def bwd_range_nets(oracle):
    """3 x 100 (skip list [0]: layer 2 has plain K = W) whose FINE network sends one gradient out of fp16's range and no activation:
    hidden unit 5 of layer 1 is 1e-6 on every point (weights 0, bias 1e-6: alive everywhere, negligible forward), and every unit of
    layer 2 reads it with the weight 2^RANGE_LOG2 -- so dL/d(pre-activation of layer 1)[5] is 2^RANGE_LOG2 times the sum of layer
    2's gradients, which kw_composite_bwd has normalised to 2^7 .. 2^8 per point"""
    sd_c, sd_f = bwd_nets(oracle, "3x100")
    sd_f = {k: v.copy() for k, v in sd_f.items()}
    sd_f["pts_linears.1.weight"][5, :] = 0.0
    sd_f["pts_linears.1.bias"][5] = np.float32(1e-6)
    sd_f["pts_linears.2.weight"][:, 5] = np.float32(2.0 ** RANGE_LOG2)
    return sd_c, sd_f


def hostile(oracle, n=100):
    """n rays with a NaN origin (3), a zero direction (5) and an infinite one (7) among them"""
    ro, rd = (x.copy() for x in _rays(oracle, n, 24))
    ro[3] = np.nan
    rd[5] = 0.0
    rd[7] = np.inf
    return ro, rd


def models(sd_c, sd_f, ns, ni, modes, mlp="f16x2"):
    """one handle per entry of `modes`, each a dict of WideModel's on-chip keywords; the handles have what they were asked for"""
    from neural_sim_nerf_amd.wide import WideModel
    ms = tuple(WideModel(sd_c, sd_f, n_samples=ns, n_importance=ni, mlp=mlp, **kw) for kw in modes)
    assert all(getattr(m, k) == v for m, kw in zip(ms, modes) for k, v in kw.items()), modes
    return ms


@contextlib.contextmanager
def small_chunks():
    """the smallest workspace the library accepts: chunks of 64 rays"""
    os.environ["NSR_WIDE_WORKSPACE_GB"] = "0.0001"
    try:
        yield
    finally:
        del os.environ["NSR_WIDE_WORKSPACE_GB"]


def taps_equal(ra, rb, what=None, keys=TAPS):
    """every tap of two handles' render_rays(debug=True): the same bits, NaN in the same places"""
    for k in keys:
        assert _same(ra[k], rb[k]), (k, what)


def grads_equal(gs, what=None):
    """every gradient of the handles' render_rays_vjp results equals the last handle's, bit for bit"""
    for g in gs[:-1]:
        assert len(g) == len(gs[-1])
        for i in range(len(g)):
            assert _same(g[i], gs[-1][i]), (what, i)


def forward_bit_for_bit(oracle, ms, sd_c, sd_f, views, label):
    """(N_samples, N_importance) = (3, 2) handles `ms`, the last one under test, on 171 rays (513 coarse rows: one past four 128-row
    blocks) and 85 (255 rows), run_network on 1 .. 257 points of both networks: every tap, every network output, the rgb gradient and
    the gradient of all six outputs at the forward's z_fine are the same bits on every handle; equal pass counts, no re-run.  One
    run_network result of the handle under test against the oracle, with the bound of test_gpu_wide_tiles."""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
        for i, r in enumerate(rs[:-1]):
            taps_equal(r, rs[-1], (n, i))
        bad = {k: int((~np.isfinite(cpu(rs[-1][k]))).sum()) for k in OUTS if not np.isfinite(cpu(rs[-1][k])).all()}
        assert not bad, (bad, n)
        zf = cpu(rs[0]["z_fine"])
        cots = _cots(n, 31 + n)
        grads_equal([m.render_rays_vjp(ro, rd, near, far, cots["rgb_map"], z_fine=zf) for m in ms], ("rgb gradient", n))
        As = [m.render_rays_vjp(ro, rd, near, far, cotangents=cots, z_fine=zf) for m in ms]
        grads_equal(As, ("gradient of all six outputs", n))
        assert np.isfinite(cpu(As[-1][0])).all() and np.isfinite(cpu(As[-1][1])).all() and np.abs(cpu(As[-1][0])).max() > 0
    rng = np.random.RandomState(7)
    e_net = 0.0
    for P in POINTS:
        pts = (rng.rand(P, 3).astype(np.float32) - 0.5) * 0.4
        dirs = oracle.normalize_dirs(rng.standard_normal((P, 3)).astype(np.float32))
        for net_id, sd in ((0, sd_c), (1, sd_f)):
            outs = [cpu(m.run_network(pts, dirs, net_id)) for m in ms]
            for i, o in enumerate(outs[:-1]):
                assert np.array_equal(o, outs[-1], equal_nan=True), (P, net_id, i)
            assert np.isfinite(outs[-1]).all()
            if P == 257 and net_id == 0 and views:      # (the oracle's run_network takes view directions)
                want = oracle.run_network(sd, pts[:, None], dirs)[:, 0]
                e_net = np.abs(outs[-1] - want).max()
                assert_close(outs[-1], want, atol=5e-5 * max(1.0, float(np.abs(want).max())), rtol=5e-5, what="run_network on %d points" % P)
    print("%s, run_network on 257 points against the oracle: %.2e" % (label, e_net))
    st = [m.range_status() for m in ms]
    assert all(x == st[-1] for x in st) and st[-1]["passes"] > 0 and st[-1]["passes_rerun"] == 0, st
    for m in ms:
        m.close()


def range_rerun_case(oracle, sd_c, sd_f, make):
    """The range safety net through a forward form: 256 rays in 64-ray chunks on make() = (the per-layer handle, the handle under
    test); every coarse pass is re-run on bf16x3 (layer by layer), so the coarse taps are a bf16x3 handle's bits, and everything
    equals the per-layer f16x2 handle's."""
    from neural_sim_nerf_amd.wide import WideModel
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 256, 26)
    with small_chunks():
        ml, mo = make()
        b3 = WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp="bf16x3")
        rl, rc, rb = (m.render_rays(ro, rd, near, far, debug=True) for m in (ml, mo, b3))
        chunks = mo.last_kernel_ms()[1]
        st = mo.range_status()
        assert chunks == 4 and st["passes_rerun"] == chunks and st["passes"] == 2 * chunks, (chunks, st)
        assert ml.range_status() == st
        taps_equal(rc, rb, keys=COARSE_TAPS)
        taps_equal(rc, rl)
        assert np.isfinite(cpu(rc["rgb_map"])).all()
        for m in (ml, mo, b3):
            m.close()


def hostile_case(oracle, ml, mo, ro, rd):
    """hostile rays on the per-layer handle and the handle under test: every tap and the range counters equal (NaN in the same
    places), the other rays' colours finite; returns the colours"""
    rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
    taps_equal(rl, rc)
    ok = np.ones(len(ro), bool)
    ok[[3, 5, 7]] = False
    rgb = cpu(rc["rgb_map"])
    assert np.isfinite(rgb[ok]).all()
    assert ml.range_status() == mo.range_status()
    ml.close()
    mo.close()
    return rgb


def company_case(oracle, m, n=300):
    """n rays on the handle `m` at (5, 4) samples: all rays, the same rays reversed, the first 37 alone and all of them in 64-ray
    chunks give every ray the same bits -- forward taps and the rgb gradient"""
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 22)
    cot = np.random.RandomState(23).standard_normal((n, 3)).astype(np.float32)
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw", "raw0")

    def run(sel):
        o, d, c = (np.ascontiguousarray(x[sel]) for x in (ro, rd, cot))
        r = m.render_rays(o, d, near, far, debug=True)
        chunks = m.last_kernel_ms()[1]
        go, gd = m.render_rays_vjp(o, d, near, far, c)
        return [cpu(r[k]) for k in keys] + [cpu(go), cpu(gd)], chunks
    whole, chunks = run(slice(None))
    assert chunks == 1 and np.isfinite(whole[0]).all() and np.isfinite(whole[6]).all() and np.abs(whole[6]).max() > 0
    rev, _ = run(slice(None, None, -1))
    few, _ = run(slice(0, 37))
    with small_chunks():
        cut, chunks = run(slice(None))
    assert chunks == (n + 63) // 64, chunks
    for k, a, b, c, d in zip(keys + ("grad_o", "grad_d"), whole, rev, few, cut):
        assert np.array_equal(a, b[::-1], equal_nan=True), (k, "reversed")
        assert np.array_equal(a[:37], c, equal_nan=True), (k, "the first 37 alone")
        assert np.array_equal(a, d, equal_nan=True), (k, "64-ray chunks")
    assert m.range_status()["passes_rerun"] == 0
    m.close()


def replay_equals_eager(m, ro, rd, call):
    """One torch.cuda.graph capture of call(rays_o, rays_d) -- a dict or a tuple of device tensors -- on the handle `m`; the replay
    on rewritten input buffers equals the eager call, bit for bit.  Returns the eager results, {name or index: array}."""
    import torch
    host = lambda r: {k: cpu(v) for k, v in (r.items() if isinstance(r, dict) else enumerate(r))}
    dev = m.device
    eager = host(call(ro, rd))
    to, td = (torch.as_tensor(np.ascontiguousarray(x[::-1]), device=dev) for x in (ro, rd))     # other rays while capturing
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        call(to, td)                                          # this stream's workspace exists before the capture
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            r = call(to, td)
    to.copy_(torch.as_tensor(ro, device=dev))
    td.copy_(torch.as_tensor(rd, device=dev))
    torch.cuda.synchronize(dev)
    graph.replay()
    torch.cuda.synchronize(dev)
    got = host(r)
    for k in eager:
        assert np.array_equal(got[k], eager[k], equal_nan=True), k
    assert m.range_status()["passes_rerun"] == 0
    m.close()
    return eager


# ---- the bounds-checked build.  What a run records, by name: the arrays of one call on the handle
def _render(m, o, d, O):
    r = m.render_rays(o, d, O.YCBV_NEAR, O.YCBV_FAR, debug=True)
    return [r[k] for k in ("rgb_map", "raw", "raw0", "z_fine")]


def _run_network(net_id):
    return lambda m, o, d, O: [m.run_network(np.zeros((129, 3), np.float32) + 0.01, np.tile(np.float32([0, 0, 1]), (129, 1)), net_id)]


BOUNDS_CALLS = {
    "render": _render,
    "vjp_ones": lambda m, o, d, O: m.render_rays_vjp(o, d, O.YCBV_NEAR, O.YCBV_FAR, np.ones((len(o), 3), np.float32)),
    "run_network0": _run_network(0),
    "run_network1": _run_network(1),
    "vjp_rgb": lambda m, o, d, O: m.render_rays_vjp(o, d, O.YCBV_NEAR, O.YCBV_FAR, _cots(len(o), 51)["rgb_map"]),
    "vjp_cots": lambda m, o, d, O: m.render_rays_vjp(o, d, O.YCBV_NEAR, O.YCBV_FAR, cotangents=_cots(len(o), 51)),
}
BOUNDS_SCRIPT = r'''
import sys
sys.path[:0] = %r
import wide_onchip_cases
wide_onchip_cases.bounds_child(*%r, out_dir=sys.argv[1])
'''


def bounds_child(provider, kw, workspaces, calls, out_dir):
    """(in the fresh process) every run of <module>.<function> = `provider` on a handle made with the keywords `kw`, once per
    workspace size in GiB (None: as the environment has it): the arrays of `calls` into res.npz, and printed last
    {tag[_workspace]: (built_with_checks, first_bad_line, passes re-run)}"""
    import importlib
    import nerf_oracle as O
    from neural_sim_nerf_amd.wide import WideModel
    out, res = {}, []
    for tag, c, f, o, d in getattr(importlib.import_module(provider[0]), provider[1])(O):
        for gb in workspaces:
            if gb is not None:
                os.environ["NSR_WIDE_WORKSPACE_GB"] = gb
            m = WideModel(c, f, n_samples=3, n_importance=2, mlp="f16x2", **kw)
            for name in calls:
                res += [x.cpu().numpy() for x in BOUNDS_CALLS[name](m, o, d, O)]
            out[tag if gb is None else tag + "_" + gb] = m.debug_bounds_status() + (m.range_status()["passes_rerun"],)
            m.close()
    np.savez(out_dir + "/res.npz", *res)
    print(out)


def bounds_checked_build(tmp_path, provider, kw, workspaces, calls):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of the kernels of nsr_wide_trunk.inc (tag 200000 +
    line).  Runs bounds_child in a fresh process on that build and on the release build.  Returns ({build: what the child printed},
    the debug build's arrays, the release build's); None when libnsr_debug.so is not built."""
    csrc = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc")
    dbg = os.path.join(csrc, "libnsr_debug.so")
    if not os.path.exists(dbg):
        return None
    code = BOUNDS_SCRIPT % ([ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")], (provider, kw, workspaces, calls))
    res = {}
    for name, lib in (("debug", dbg), ("release", os.path.join(csrc, "libnsr.so"))):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([sys.executable, "-c", code, str(d)], env=dict(os.environ, NSR_LIB_PATH=lib), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = eval(r.stdout.strip().splitlines()[-1])
    return res, np.load(tmp_path / "debug" / "res.npz"), np.load(tmp_path / "release" / "res.npz")


def bounds_clean_and_equal(got, n_runs, n_arrays):
    """no check tripped in the debug build, the release build reports none, a pass was re-run exactly in the range cases, and every
    array of the two builds is the same"""
    res, a, b = got
    assert len(res["debug"]) == n_runs and all(v[:2] == (True, 0) for v in res["debug"].values()), res["debug"]
    assert all(v[:2] == (False, 0) for v in res["release"].values()), res["release"]
    assert all(v[2] > 0 if tag.startswith("range") else v[2] == 0 for tag, v in res["debug"].items() if not tag.startswith("hostile")), res["debug"]
    assert len(a.files) == len(b.files) == n_runs * n_arrays
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
