"""GPU tests of the layered renderer's ON-CHIP trunk (kw_trunk_h2 in csrc/nsr_wide_trunk.inc; WideModel(trunk="onchip"); run with
-m gpu on an MI355X).  The trunk kernel keeps the arithmetic of the per-layer GEMM per output element -- accumulator from 0, k16
blocks ascending, the piece products in a fixed order, one epilogue expression, the next layer's operand pieces by the same split --
and only changes where the activation lives between two layers.  So a trunk="onchip" handle must give the bits of a trunk="layers"
handle everywhere: every tap of the forward, the network outputs on ragged point counts, the gradients (whose kept passes run layer
by layer while the coarse forward runs on chip), the range safety net's counters and re-runs, hostile rays, any company of rays,
under capture, and in the bounds-checked build.  No tolerance anywhere but the one check against the oracle."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close
from test_gpu_wide_tiles import OUTS, POINTS, TAPS, _cots, _rays, _same, cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_PTS, L_VIEWS = 4, 2
COARSE_TAPS = ("rgb0", "acc0", "weights0", "raw0", "inds", "z_samples", "z_fine")

# name -> (D, W, skips, use_viewdirs): 3 x W with one skip after layer 0 or 1 in turn (NJ = 1: 24, 40; NJ = 2: 100, 128 -- a width
# below, at and off the 32-column blocks of either form), two skips, no skip at the full 128 columns, and a network without view
# directions (output_linear behind the trunk instead of the feature / alpha heads)
NETS = {"3x24": (3, 24, [0], True), "3x40": (3, 40, [1], True), "3x100": (3, 100, [0], True), "3x128": (3, 128, [1], True),
        "5x100": (5, 100, [0, 2], True), "2x128": (2, 128, [], True), "3x40-noviews": (3, 40, [0], False)}
# At W = 24 the trunk's activations are large against the fixed density bias (synth_weights_shape scales the trunk by sqrt(256 / W)) and
# most seeds give rays with an empty stretch (disp = 0 / 0 in the reference too); these two keep the density above 0.15 everywhere
# between near and far on the rays used here (checked with the oracle's run_network)
SEEDS = {"3x24": (301, 305)}


@functools.lru_cache(maxsize=None)
def _nets(oracle, name):
    """(coarse, fine) of NETS[name], with the density scaling of test_gpu_wide_tiles._nets: the density row at an eighth of its
    nn.Linear size and its bias +0.5, so that every ray is translucent at 3 + 2 samples (finite disp, gradients through every layer).
    acc = 1 on every ray there (the last sample is dense, its distance 1e10), so acc's gradient is rounding noise on these networks:
    test_gpu_wide_trunk_bwd._signed_nets is the variant on which it is a gradient."""
    D, W, skips, views = NETS[name]
    nets = []
    for s in SEEDS.get(name, (300 + sorted(NETS).index(name), 400 + sorted(NETS).index(name))):
        sd = oracle.synth_weights_shape(s, D, W, L_PTS, L_VIEWS, list(skips), views)
        f = np.float32(W / (400.0 * 256.0))
        if views:
            sd["alpha_linear.weight"] = (sd["alpha_linear.weight"] * f).astype(np.float32)
            sd["alpha_linear.bias"] = np.full_like(sd["alpha_linear.bias"], 0.5)
        else:
            sd["output_linear.weight"][3] *= f
            sd["output_linear.bias"][3] = np.float32(0.5)
        nets.append(sd)
    return tuple(nets)


def _pair(sd_c, sd_f, ns, ni, mlp="f16x2"):
    """(trunk="layers" handle, trunk="onchip" handle) of one arithmetic"""
    from neural_sim_nerf_amd.wide import WideModel
    return tuple(WideModel(sd_c, sd_f, n_samples=ns, n_importance=ni, mlp=mlp, trunk=t) for t in ("layers", "onchip"))


def _range_nets(oracle, layer):
    """3 x 100 coarse network whose pts_linears.<layer> bias sends hidden unit 5 to 7e4 on every point -- layer 1: the value leaves
    fp16's range INSIDE the trunk (split for layer 2 in LDS); layer 2: on the trunk's last layer, split by the heads behind it"""
    sd_c, sd_f = _nets(oracle, "3x100")
    sd_c = {k: v.copy() for k, v in sd_c.items()}
    sd_c["pts_linears.%d.bias" % layer][5] += 7.0e4
    return sd_c, sd_f


def _hostile(oracle, n=100):
    ro, rd = (x.copy() for x in _rays(oracle, n, 24))
    ro[3] = np.nan
    rd[5] = 0.0
    rd[7] = np.inf
    return ro, rd


@pytest.mark.parametrize("name", sorted(NETS))
def test_onchip_trunk_equals_the_per_layer_path_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past four 128-row blocks) and 85 (255 rows), run_network
    on 1 .. 257 points of both networks: every tap, every network output, the rgb gradient and the gradient of all six outputs at
    the forward's z_fine are the same bits on a trunk="layers" and a trunk="onchip" handle; equal pass counts, no re-run."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    D, W, skips, views = NETS[name]
    assert wide.trunk_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.trunk_plan(sd_c, "f16x2")["nj"] == (1 if W <= 64 else 2)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ml, mo = _pair(sd_c, sd_f, 3, 2)
    assert (ml.trunk, mo.trunk) == ("layers", "onchip")
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        rl, rc = (m.render_rays(ro, rd, near, far, debug=True) for m in (ml, mo))
        for k in TAPS:
            assert _same(rl[k], rc[k]), (k, n)
        bad = {k: int((~np.isfinite(cpu(rc[k]))).sum()) for k in OUTS if not np.isfinite(cpu(rc[k])).all()}
        assert not bad, (bad, n)
        zf = cpu(rl["z_fine"])
        cots = _cots(n, 31 + n)
        gl, gc = (m.render_rays_vjp(ro, rd, near, far, cots["rgb_map"], z_fine=zf) for m in (ml, mo))
        al, ac = (m.render_rays_vjp(ro, rd, near, far, cotangents=cots, z_fine=zf) for m in (ml, mo))
        for x, y, what in ((gl, gc, "rgb gradient"), (al, ac, "gradient of all six outputs")):
            assert _same(x[0], y[0]) and _same(x[1], y[1]), (what, n)
        assert np.isfinite(cpu(ac[0])).all() and np.isfinite(cpu(ac[1])).all() and np.abs(cpu(ac[0])).max() > 0
    rng = np.random.RandomState(7)
    e_net = 0.0
    for P in POINTS:
        pts = (rng.rand(P, 3).astype(np.float32) - 0.5) * 0.4
        dirs = oracle.normalize_dirs(rng.standard_normal((P, 3)).astype(np.float32))
        for net_id, sd in ((0, sd_c), (1, sd_f)):
            ol, oc = (cpu(m.run_network(pts, dirs, net_id)) for m in (ml, mo))
            assert np.array_equal(ol, oc, equal_nan=True), (P, net_id)
            assert np.isfinite(oc).all()
            if P == 257 and net_id == 0 and views:      # the on-chip handle against the oracle (its run_network takes view directions), with the bound of test_gpu_wide_tiles
                want = oracle.run_network(sd, pts[:, None], dirs)[:, 0]
                e_net = np.abs(oc - want).max()
                assert_close(oc, want, atol=5e-5 * max(1.0, float(np.abs(want).max())), rtol=5e-5, what="run_network on %d points" % P)
    print("%s on chip, run_network on 257 points against the oracle: %.2e" % (name, e_net))
    sl, sc = ml.range_status(), mo.range_status()
    assert sl == sc and sc["passes"] > 0 and sc["passes_rerun"] == 0, (sl, sc)
    ml.close()
    mo.close()


def test_an_ineligible_network_on_an_onchip_handle_runs_per_layer_and_other_arithmetics_are_refused(oracle):
    """Coarse 3 x 40 (on chip) with fine 3 x 136 (padded width 160: layer by layer) on one handle; trunk="onchip" exists for f16x2
    only -- WideModel says so, and nsrw_create for a caller of the C interface."""
    from neural_sim_nerf_amd import wide
    sd_c = _nets(oracle, "3x40")[0]
    sd_f = oracle.synth_weights_shape(411, 3, 136, L_PTS, L_VIEWS, [1], True)
    sd_f["alpha_linear.weight"] = (sd_f["alpha_linear.weight"] * np.float32(136 / (400.0 * 256.0))).astype(np.float32)
    sd_f["alpha_linear.bias"] = np.full_like(sd_f["alpha_linear.bias"], 0.5)
    assert wide.trunk_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.trunk_plan(sd_f, "f16x2")["mode"] == "layers"
    ml, mo = _pair(sd_c, sd_f, 3, 2)
    ro, rd = _rays(oracle, 171, 25)
    rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
    for k in TAPS:
        assert _same(rl[k], rc[k]), k
    assert np.isfinite(cpu(rc["rgb_map"])).all() and ml.range_status() == mo.range_status()
    ml.close()
    mo.close()
    for mlp in ("bf16x3", "fp32"):
        with pytest.raises(NotImplementedError, match="f16x2"):
            wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp=mlp, trunk="onchip")
    with pytest.raises(ValueError, match="trunk must be"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, trunk="lds")
    lib = wide.load()
    for flags in (wide.FLAG_TRUNK_ONCHIP, wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_BF16X3):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
        assert "NSRW_FLAG_TRUNK_ONCHIP needs NSRW_FLAG_MLP_F16X2" in lib.nsrw_last_error().decode()
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_F16X2)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    assert lib.nsrw_destroy(h) == 0


@pytest.mark.parametrize("layer", [1, 2])
def test_a_value_that_leaves_the_fp16_range_in_the_trunk_reruns_the_pass(layer, oracle):
    """The range safety net through the trunk kernel: 256 rays in 64-ray chunks; every coarse pass is re-run on bf16x3 (layer by
    layer), so the coarse taps are a bf16x3 handle's bits, and everything equals the trunk="layers" f16x2 handle's."""
    from neural_sim_nerf_amd.wide import WideModel
    sd_c, sd_f = _range_nets(oracle, layer)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 256, 26)
    os.environ["NSR_WIDE_WORKSPACE_GB"] = "0.0001"        # the smallest workspace the library accepts: chunks of 64 rays
    try:
        ml, mo = _pair(sd_c, sd_f, 3, 2)
        b3 = WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp="bf16x3")
        rl, rc, rb = (m.render_rays(ro, rd, near, far, debug=True) for m in (ml, mo, b3))
        chunks = mo.last_kernel_ms()[1]
        st = mo.range_status()
        assert chunks == 4 and st["passes_rerun"] == chunks and st["passes"] == 2 * chunks, (chunks, st)
        assert ml.range_status() == st
        for k in COARSE_TAPS:
            assert _same(rc[k], rb[k]), k
        for k in TAPS:
            assert _same(rc[k], rl[k]), k
        assert np.isfinite(cpu(rc["rgb_map"])).all()
        for m in (ml, mo, b3):
            m.close()
    finally:
        del os.environ["NSR_WIDE_WORKSPACE_GB"]


def test_hostile_rays_through_the_trunk(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 40 network: every tap and the range counters
    equal the per-layer handle's (NaN in the same places)."""
    sd_c, sd_f = _nets(oracle, "3x40")
    ro, rd = _hostile(oracle)
    ml, mo = _pair(sd_c, sd_f, 3, 2)
    rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
    for k in TAPS:
        assert _same(rl[k], rc[k]), k
    ok = np.ones(len(ro), bool)
    ok[[3, 5, 7]] = False
    assert np.isfinite(cpu(rc["rgb_map"])[ok]).all()
    assert ml.range_status() == mo.range_status()
    ml.close()
    mo.close()


def test_a_rays_result_on_chip_depends_on_nothing_but_the_ray(oracle):
    """3 x 128 at (5, 4) samples, 300 rays on the on-chip handle: all rays, the same rays reversed, the first 37 alone and all of
    them in 64-ray chunks give every ray the same bits (a ray's rows share a 128-point block with other neighbours each time)."""
    sd_c, sd_f = _nets(oracle, "3x128")
    n, near, far = 300, oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 22)
    cot = np.random.RandomState(23).standard_normal((n, 3)).astype(np.float32)
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw", "raw0")
    from neural_sim_nerf_amd.wide import WideModel
    m = WideModel(sd_c, sd_f, n_samples=5, n_importance=4, mlp="f16x2", trunk="onchip")

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
    os.environ["NSR_WIDE_WORKSPACE_GB"] = "0.0001"
    try:
        cut, chunks = run(slice(None))
    finally:
        del os.environ["NSR_WIDE_WORKSPACE_GB"]
    assert chunks == (n + 63) // 64, chunks
    for k, a, b, c, d in zip(keys + ("grad_o", "grad_d"), whole, rev, few, cut):
        assert np.array_equal(a, b[::-1], equal_nan=True), (k, "reversed")
        assert np.array_equal(a[:37], c, equal_nan=True), (k, "the first 37 alone")
        assert np.array_equal(a, d, equal_nan=True), (k, "64-ray chunks")
    assert m.range_status()["passes_rerun"] == 0
    m.close()


def test_the_trunk_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays on the on-chip handle; the replay on rewritten input buffers equals the eager call."""
    import torch
    from neural_sim_nerf_amd.wide import WideModel
    sd_c, sd_f = _nets(oracle, "3x100")
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 171, 27)
    m = WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp="f16x2", trunk="onchip")
    dev = m.device
    eager = {k: cpu(v) for k, v in m.render_rays(ro, rd, near, far).items()}
    to, td = (torch.as_tensor(np.ascontiguousarray(x[::-1]), device=dev) for x in (ro, rd))     # other rays while capturing
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        m.render_rays(to, td, near, far)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            r = m.render_rays(to, td, near, far)
    to.copy_(torch.as_tensor(ro, device=dev))
    td.copy_(torch.as_tensor(rd, device=dev))
    torch.cuda.synchronize(dev)
    graph.replay()
    torch.cuda.synchronize(dev)
    for k in eager:
        assert np.array_equal(cpu(r[k]), eager[k], equal_nan=True), k
    assert np.isfinite(eager["rgb_map"]).all() and m.range_status()["passes_rerun"] == 0
    m.close()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 24, 100, 128 on 171 rays, both
    range cases and the hostile rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x100", "3x128")]
    ro6, rd6 = _rays(oracle, 256, 26)
    runs += [("range%d" % layer,) + _range_nets(oracle, layer) + (ro6, rd6) for layer in (1, 2)]
    runs.append(("hostile",) + _nets(oracle, "3x40") + _hostile(oracle))
    return runs


def test_onchip_trunk_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_trunk_h2 (tag 200000 + line).  A fresh process
    runs the cases above on the on-chip handle with a one-chunk and a 64-ray-chunk workspace; no check may trip, and every output
    equals the release build's."""
    import subprocess
    dbg = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr_debug.so")
    if not os.path.exists(dbg):
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import nerf_oracle as O
from neural_sim_nerf_amd.wide import WideModel
from test_gpu_wide_trunk import _bounds_runs
out, res = {}, []
for tag, c, f, o, d in _bounds_runs(O):
    for gb in ("16", "0.0001"):
        os.environ["NSR_WIDE_WORKSPACE_GB"] = gb
        m = WideModel(c, f, n_samples=3, n_importance=2, mlp="f16x2", trunk="onchip")
        r = m.render_rays(o, d, O.YCBV_NEAR, O.YCBV_FAR, debug=True)
        go, gd = m.render_rays_vjp(o, d, O.YCBV_NEAR, O.YCBV_FAR, np.ones((len(o), 3), np.float32))
        rn = m.run_network(np.zeros((129, 3), np.float32) + 0.01, np.tile(np.float32([0, 0, 1]), (129, 1)), 0)
        res += [r[k].cpu().numpy() for k in ("rgb_map", "raw", "raw0", "z_fine")] + [go.cpu().numpy(), gd.cpu().numpy(), rn.cpu().numpy()]
        out[tag + "_" + gb] = m.debug_bounds_status() + (m.range_status()["passes_rerun"],)
        m.close()
np.savez(sys.argv[1] + "/res.npz", *res)
print(out)
''' % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    res = {}
    for name, lib in (("debug", dbg), ("release", os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so"))):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([sys.executable, "-c", code, str(d)], env=dict(os.environ, NSR_LIB_PATH=lib), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = eval(r.stdout.strip().splitlines()[-1])
    assert len(res["debug"]) == 12 and all(v[:2] == (True, 0) for v in res["debug"].values()), res["debug"]
    assert all(v[:2] == (False, 0) for v in res["release"].values()), res["release"]
    assert all(v[2] > 0 if tag.startswith("range") else v[2] == 0 for tag, v in res["debug"].items() if not tag.startswith("hostile")), res["debug"]
    a, b = np.load(tmp_path / "debug" / "res.npz"), np.load(tmp_path / "release" / "res.npz")
    assert len(a.files) == len(b.files) == 12 * 7
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
