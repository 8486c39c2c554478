"""GPU tests of the layered renderer's ON-CHIP heads (the heads form of kw_trunk_h2 in csrc/nsr_wide_trunk.inc;
WideModel(trunk="onchip", heads="onchip"); run with -m gpu on an MI355X).  Behind the on-chip trunk the same workgroup runs
alpha_linear, feature_linear, views_linears.0 and rgb_linear (or output_linear) on its 128 rows with the arithmetic of the per-layer
GEMM per output element, and only the raw outputs reach memory.  So a heads="onchip" handle must give the bits of a trunk="layers"
handle, and of a trunk="onchip", heads="layers" handle, everywhere: every tap of the forward, the network outputs on ragged point
counts, the gradients (whose kept passes run layer by layer), the range safety net's counters and re-runs for values that leave
fp16's range in each head, hostile rays, any company of rays, under capture, and in the bounds-checked build.  No tolerance anywhere
but the one check against the oracle."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close
from test_gpu_wide_tiles import OUTS, POINTS, TAPS, _cots, _rays, _same, cpu
from test_gpu_wide_trunk import COARSE_TAPS, L_PTS, _hostile, _range_nets
from test_gpu_wide_trunk import _nets as _trunk_nets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (D, W, skips, multires_views or None for a network without view directions, the on-chip trunk test's name of the same
# network or None, seeds).  3x66: Wp = 96 is three column blocks of the four in feature_linear's image, W2 = 33 makes views_linears.0
# two column blocks wide (W2p = 64), and Cv = 64; 2x64-v15: Cv = 96, the widest direction encoding; 3x40-noviews: output_linear.
# The seeds of the networks that are new here keep the density above 0.15 everywhere between near and far on the rays used
# (checked with the oracle's run_network, as for the trunk test's 3x24).
NETS = {"3x24": (3, 24, [0], 2, "3x24", None), "3x40-v4": (3, 40, [1], 4, None, (505, 601)), "3x66-v6": (3, 66, [0], 6, None, (502, 602)),
        "3x100": (3, 100, [0], 2, "3x100", None), "3x128-v4": (3, 128, [1], 4, None, (503, 603)),
        "2x64-v15": (2, 64, [], 15, None, (504, 604)), "2x128": (2, 128, [], 2, "2x128", None),
        "3x40-noviews": (3, 40, [0], None, "3x40-noviews", None)}
MODES = (("layers", "layers"), ("onchip", "layers"), ("onchip", "onchip"))       # (trunk, heads): the last is the one under test


@functools.lru_cache(maxsize=None)
def _nets(oracle, name):
    """(coarse, fine) of NETS[name] with the density scaling of test_gpu_wide_trunk._nets (the density row at an eighth of its
    nn.Linear size, its bias +0.5: every ray translucent at 3 + 2 samples)"""
    D, W, skips, Lv, trunk_name, seeds = NETS[name]
    if trunk_name:
        return _trunk_nets(oracle, trunk_name)
    nets = []
    for s in seeds:
        sd = oracle.synth_weights_shape(s, D, W, L_PTS, Lv, list(skips), True)
        sd["alpha_linear.weight"] = (sd["alpha_linear.weight"] * np.float32(W / (400.0 * 256.0))).astype(np.float32)
        sd["alpha_linear.bias"] = np.full_like(sd["alpha_linear.bias"], 0.5)
        nets.append(sd)
    return tuple(nets)


def _models(sd_c, sd_f, ns, ni, modes=MODES):
    from neural_sim_nerf_amd.wide import WideModel
    ms = tuple(WideModel(sd_c, sd_f, n_samples=ns, n_importance=ni, mlp="f16x2", trunk=t, heads=h) for t, h in modes)
    assert tuple((m.trunk, m.heads) for m in ms) == tuple(modes)
    return ms


def _head_range_nets(oracle, case):
    """3 x 100 coarse network in which unit 5 reaches 7e4 on every point -- "feature": in feature_linear's output, split for
    views_linears.0; "views": in views_linears.0's output, split for rgb_linear; "trunk": on the trunk's last layer (the trunk
    test's layer-2 case), split for alpha_linear and feature_linear"""
    if case == "trunk":
        return _range_nets(oracle, 2)
    sd_c, sd_f = _trunk_nets(oracle, "3x100")
    sd_c = {k: v.copy() for k, v in sd_c.items()}
    sd_c[{"feature": "feature_linear.bias", "views": "views_linears.0.bias"}[case]][5] += 7.0e4
    return sd_c, sd_f


@pytest.mark.parametrize("name", sorted(NETS))
def test_onchip_heads_equal_the_per_layer_path_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past four 128-row blocks) and 85 (255 rows), run_network
    on 1 .. 257 points of both networks: every tap, every network output, the rgb gradient and the gradient of all six outputs at
    the forward's z_fine are the same bits on the three handles; equal pass counts, no re-run."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    D, W, skips, Lv, _, _ = NETS[name]
    views = Lv is not None
    assert wide.heads_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.heads_plan(sd_f, "f16x2")["mode"] == "onchip"
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ms = _models(sd_c, sd_f, 3, 2)
    mh = ms[-1]
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms]
        for r, mode in zip(rs[:-1], MODES):
            for k in TAPS:
                assert _same(r[k], rs[-1][k]), (k, n, mode)
        bad = {k: int((~np.isfinite(cpu(rs[-1][k]))).sum()) for k in OUTS if not np.isfinite(cpu(rs[-1][k])).all()}
        assert not bad, (bad, n)
        zf = cpu(rs[0]["z_fine"])
        cots = _cots(n, 31 + n)
        gs = [m.render_rays_vjp(ro, rd, near, far, cots["rgb_map"], z_fine=zf) for m in ms]
        As = [m.render_rays_vjp(ro, rd, near, far, cotangents=cots, z_fine=zf) for m in ms]
        for xs, what in ((gs, "rgb gradient"), (As, "gradient of all six outputs")):
            for x, mode in zip(xs[:-1], MODES):
                assert _same(x[0], xs[-1][0]) and _same(x[1], xs[-1][1]), (what, n, mode)
        assert np.isfinite(cpu(As[-1][0])).all() and np.isfinite(cpu(As[-1][1])).all() and np.abs(cpu(As[-1][0])).max() > 0
    rng = np.random.RandomState(7)
    e_net = 0.0
    for P in POINTS:
        pts = (rng.rand(P, 3).astype(np.float32) - 0.5) * 0.4
        dirs = oracle.normalize_dirs(rng.standard_normal((P, 3)).astype(np.float32))
        for net_id, sd in ((0, sd_c), (1, sd_f)):
            os_ = [cpu(m.run_network(pts, dirs, net_id)) for m in ms]
            for o, mode in zip(os_[:-1], MODES):
                assert np.array_equal(o, os_[-1], equal_nan=True), (P, net_id, mode)
            assert np.isfinite(os_[-1]).all()
            if P == 257 and net_id == 0 and views:      # the on-chip handle against the oracle (its run_network takes view directions), with the bound of test_gpu_wide_trunk
                want = oracle.run_network(sd, pts[:, None], dirs)[:, 0]
                e_net = np.abs(os_[-1] - want).max()
                assert_close(os_[-1], want, atol=5e-5 * max(1.0, float(np.abs(want).max())), rtol=5e-5, what="run_network on %d points" % P)
    print("%s heads on chip, run_network on 257 points against the oracle: %.2e" % (name, e_net))
    st = [m.range_status() for m in ms]
    assert st[0] == st[1] == st[2] and st[2]["passes"] > 0 and st[2]["passes_rerun"] == 0, st
    for m in ms:
        m.close()


@pytest.mark.parametrize("case", ["feature", "views", "trunk"])
def test_a_value_that_leaves_the_fp16_range_in_the_heads_reruns_the_pass(case, oracle):
    """The range safety net through the heads: 256 rays in 64-ray chunks; every coarse pass is re-run on bf16x3 (layer by layer), so
    the coarse taps are a bf16x3 handle's bits, and everything equals the trunk="layers" f16x2 handle's."""
    from neural_sim_nerf_amd.wide import WideModel
    sd_c, sd_f = _head_range_nets(oracle, case)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 256, 26)
    os.environ["NSR_WIDE_WORKSPACE_GB"] = "0.0001"        # the smallest workspace the library accepts: chunks of 64 rays
    try:
        ml, mh = _models(sd_c, sd_f, 3, 2, (MODES[0], MODES[2]))
        b3 = WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp="bf16x3")
        rl, rh, rb = (m.render_rays(ro, rd, near, far, debug=True) for m in (ml, mh, b3))
        chunks = mh.last_kernel_ms()[1]
        st = mh.range_status()
        assert chunks == 4 and st["passes_rerun"] == chunks and st["passes"] == 2 * chunks, (chunks, st)
        assert ml.range_status() == st
        for k in COARSE_TAPS:
            assert _same(rh[k], rb[k]), k
        for k in TAPS:
            assert _same(rh[k], rl[k]), k
        assert np.isfinite(cpu(rh["rgb_map"])).all()
        for m in (ml, mh, b3):
            m.close()
    finally:
        del os.environ["NSR_WIDE_WORKSPACE_GB"]


def test_hostile_rays_through_the_heads(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 40 network: every tap and the range counters
    equal the per-layer handle's (NaN in the same places)."""
    sd_c, sd_f = _trunk_nets(oracle, "3x40")
    ro, rd = _hostile(oracle)
    ml, mh = _models(sd_c, sd_f, 3, 2, (MODES[0], MODES[2]))
    rl, rh = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mh))
    for k in TAPS:
        assert _same(rl[k], rh[k]), k
    ok = np.ones(len(ro), bool)
    ok[[3, 5, 7]] = False
    assert np.isfinite(cpu(rh["rgb_map"])[ok]).all()
    assert ml.range_status() == mh.range_status()
    ml.close()
    mh.close()


def test_a_rays_result_with_onchip_heads_depends_on_nothing_but_the_ray(oracle):
    """3 x 128 at (5, 4) samples, 300 rays on the heads="onchip" handle: all rays, the same rays reversed, the first 37 alone and all
    of them in 64-ray chunks give every ray the same bits (a ray's rows share a 128-point block with other neighbours each time)."""
    sd_c, sd_f = _trunk_nets(oracle, "3x128")
    n, near, far = 300, oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 22)
    cot = np.random.RandomState(23).standard_normal((n, 3)).astype(np.float32)
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw", "raw0")
    m, = _models(sd_c, sd_f, 5, 4, (MODES[2],))

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


def test_the_heads_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays on the heads="onchip" handle; the replay on rewritten input buffers equals the
    eager call."""
    import torch
    sd_c, sd_f = _trunk_nets(oracle, "3x100")
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 171, 27)
    m, = _models(sd_c, sd_f, 3, 2, (MODES[2],))
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


def test_heads_onchip_is_refused_without_the_onchip_trunk_and_an_ineligible_network_runs_per_layer(oracle):
    """heads="onchip" needs trunk="onchip" on an f16x2 handle -- WideModel says so, and nsrw_create for a caller of the C interface.
    Coarse 3 x 40 (on chip, heads too) with fine 3 x 136 (padded width 160: layer by layer, heads too) on one handle."""
    from neural_sim_nerf_amd import wide
    sd_c = _trunk_nets(oracle, "3x40")[0]
    with pytest.raises(NotImplementedError, match="trunk=\"onchip\""):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="layers", heads="onchip")
    for mlp in ("bf16x3", "fp32"):
        with pytest.raises(NotImplementedError):
            wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp=mlp, heads="onchip")
    with pytest.raises(ValueError, match="heads must be"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, trunk="onchip", heads="lds")
    lib = wide.load()
    for flags in (wide.FLAG_HEADS_ONCHIP | wide.FLAG_MLP_F16X2, wide.FLAG_HEADS_ONCHIP):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
        msg = lib.nsrw_last_error().decode()
        assert "NSRW_FLAG_HEADS_ONCHIP" in msg and "NSRW_FLAG_TRUNK_ONCHIP" in msg, msg
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_HEADS_ONCHIP | wide.FLAG_TRUNK_ONCHIP | wide.FLAG_MLP_F16X2)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    assert lib.nsrw_destroy(h) == 0
    # the environment's wish applies where it can
    os.environ["NSR_WIDE_HEADS"] = "onchip"
    try:
        m = wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip")
        assert m.heads == "onchip"
        m.close()
        for kw in (dict(mlp="f16x2"), dict(mlp="bf16x3"), dict(mlp="fp32")):
            m = wide.WideModel(sd_c, None, n_samples=3, n_importance=0, **kw)
            assert m.heads == "layers" and m.trunk == "layers"
            m.close()
    finally:
        del os.environ["NSR_WIDE_HEADS"]
    sd_f = oracle.synth_weights_shape(411, 3, 136, L_PTS, 2, [1], True)
    sd_f["alpha_linear.weight"] = (sd_f["alpha_linear.weight"] * np.float32(136 / (400.0 * 256.0))).astype(np.float32)
    sd_f["alpha_linear.bias"] = np.full_like(sd_f["alpha_linear.bias"], 0.5)
    assert wide.heads_plan(sd_c, "f16x2")["mode"] == "onchip" and wide.heads_plan(sd_f, "f16x2")["mode"] == "layers"
    ml, mh = _models(sd_c, sd_f, 3, 2, (MODES[0], MODES[2]))
    ro, rd = _rays(oracle, 171, 25)
    rl, rh = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mh))
    for k in TAPS:
        assert _same(rl[k], rh[k]), k
    assert np.isfinite(cpu(rh["rgb_map"])).all() and ml.range_status() == mh.range_status()
    ml.close()
    mh.close()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 24, 66, 128 on 171 rays, the
    three range cases and the hostile rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x66-v6", "3x128-v4")]
    ro6, rd6 = _rays(oracle, 256, 26)
    runs += [("range-" + case,) + _head_range_nets(oracle, case) + (ro6, rd6) for case in ("feature", "views", "trunk")]
    runs.append(("hostile",) + _trunk_nets(oracle, "3x40") + _hostile(oracle))
    return runs


def test_onchip_heads_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_trunk_h2 (tag 200000 + line).  A fresh process
    runs the cases above on the heads="onchip" handle with a one-chunk and a 64-ray-chunk workspace; no check may trip, and every
    output equals the release build's."""
    import subprocess
    dbg = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr_debug.so")
    if not os.path.exists(dbg):
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    code = r'''
import os, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import nerf_oracle as O
from neural_sim_nerf_amd.wide import WideModel
from test_gpu_wide_heads import _bounds_runs
out, res = {}, []
for tag, c, f, o, d in _bounds_runs(O):
    for gb in ("16", "0.0001"):
        os.environ["NSR_WIDE_WORKSPACE_GB"] = gb
        m = WideModel(c, f, n_samples=3, n_importance=2, mlp="f16x2", trunk="onchip", heads="onchip")
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
    assert len(res["debug"]) == 14 and all(v[:2] == (True, 0) for v in res["debug"].values()), res["debug"]
    assert all(v[:2] == (False, 0) for v in res["release"].values()), res["release"]
    assert all(v[2] > 0 if tag.startswith("range") else v[2] == 0 for tag, v in res["debug"].items() if not tag.startswith("hostile")), res["debug"]
    a, b = np.load(tmp_path / "debug" / "res.npz"), np.load(tmp_path / "release" / "res.npz")
    assert len(a.files) == len(b.files) == 14 * 7
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
