"""GPU tests of the WIDE form of the layered renderer's on-chip trunk (kw_trunk_h2<2, false, 2> in csrc/nsr_wide_trunk.inc;
WideModel(trunk="onchip", trunk_width=256); run with -m gpu on an MI355X): networks of padded width 160 .. 256 on blocks of 64 points.
Per output element the wide form keeps the arithmetic of the per-layer GEMM -- accumulator from 0, k16 blocks ascending, the piece
products in a fixed order, one epilogue expression, the next layer's operand pieces by the same split -- so such a handle must give
the bits of a trunk="layers" handle everywhere: every tap of the forward, the network outputs on ragged point counts, the gradients
(whose kept passes run layer by layer on both), the range safety net's counters and re-runs, hostile rays, any company of rays,
under capture, and in the bounds-checked build.  No tolerance anywhere but the one check against the oracle."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close
from test_gpu_wide_tiles import OUTS, TAPS, _cots, _rays, _same, cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_PTS, L_VIEWS = 4, 2
POINTS = (1, 63, 64, 65, 127, 128, 129, 257)        # around one and two blocks of either form, and past four
# name -> (D, W, skips, use_viewdirs).  Padded widths 160 (five column blocks computed, six in the weight image: the last quarter of
# the workgroup idles), 192 (six and six), 224 (seven of eight) and 256; the skip after layer 0 or 1, two skips, none; a network
# without view directions (output_linear behind the trunk)
NETS = {"3x136": (3, 136, [1], True), "3x192": (3, 192, [0], True), "3x200": (3, 200, [1], True), "3x256": (3, 256, [1], True),
        "5x256": (5, 256, [0, 2], True), "2x256": (2, 256, [], True), "3x160-noviews": (3, 160, [], False)}
NARROW = (3, 40, [1], True)                          # the coarse network of the mixed handle


def _scaled(oracle, seed, D, W, skips, views):
    """a synthetic network with the density scaling of test_gpu_wide_trunk._nets: the density row at an eighth of its nn.Linear size
    and its bias +0.5, so that every ray is translucent at 3 + 2 samples"""
    sd = oracle.synth_weights_shape(seed, D, W, L_PTS, L_VIEWS, list(skips), views)
    f = np.float32(W / (400.0 * 256.0))
    if views:
        sd["alpha_linear.weight"] = (sd["alpha_linear.weight"] * f).astype(np.float32)
        sd["alpha_linear.bias"] = np.full_like(sd["alpha_linear.bias"], 0.5)
    else:
        sd["output_linear.weight"][3] *= f
        sd["output_linear.bias"][3] = np.float32(0.5)
    return sd


@functools.lru_cache(maxsize=None)
def _nets(oracle, name):
    """(coarse, fine) of NETS[name]"""
    i = sorted(NETS).index(name)
    return tuple(_scaled(oracle, s + i, *NETS[name]) for s in (500, 600))


def _pair(sd_c, sd_f, ns=3, ni=2):
    """(trunk="layers" handle, trunk="onchip" handle that takes padded widths up to 256)"""
    from neural_sim_nerf_amd.wide import WideModel
    return (WideModel(sd_c, sd_f, n_samples=ns, n_importance=ni, mlp="f16x2", trunk="layers"),
            WideModel(sd_c, sd_f, n_samples=ns, n_importance=ni, mlp="f16x2", trunk="onchip", trunk_width=256))


def _range_nets(oracle, layer):
    """3 x 200 coarse network whose pts_linears.<layer> bias sends hidden unit 5 to 7e4 on every point -- layer 1: the value leaves
    fp16's range INSIDE the trunk (split for layer 2 in LDS); layer 2: on the trunk's last layer, split by the heads behind it"""
    sd_c, sd_f = _nets(oracle, "3x200")
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
def test_wide_onchip_trunk_equals_the_per_layer_path_bit_for_bit(name, oracle):
    """(N_samples, N_importance) = (3, 2) on 171 rays (513 coarse rows: one past a whole number of 64-row and of 128-row blocks) and
    85, run_network on 1 .. 257 points of both networks: every tap, every network output, the rgb gradient and the gradient of all six
    outputs at the forward's z_fine are the same bits on a trunk="layers" and a trunk="onchip", trunk_width=256 handle; equal pass
    counts, no re-run.  One run_network result of the on-chip handle against the oracle, with the bound of test_gpu_wide_tiles."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    D, W, skips, views = NETS[name]
    assert wide.trunk_plan(sd_c, "f16x2")["mode"] == "layers"
    assert wide.trunk_plan(sd_c, "f16x2", "onchip", trunk_width=256) == dict(mode="onchip", nj=2, tile_rows=64, lds_bytes=159744)
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ml, mo = _pair(sd_c, sd_f)
    assert (ml.trunk, ml.trunk_width, mo.trunk, mo.trunk_width) == ("layers", 128, "onchip", 256)
    ro_all, rd_all = _rays(oracle, 171 + 85, 21)
    for lo, hi in ((0, 171), (171, 256)):
        ro, rd = ro_all[lo:hi], rd_all[lo:hi]
        n = len(ro)
        rl, rc = (m.render_rays(ro, rd, near, far, debug=True) for m in (ml, mo))
        for k in TAPS:
            assert _same(rl[k], rc[k]), (k, n)
        assert np.isfinite(cpu(rc["rgb_map"])).all() and np.isfinite(cpu(rc["raw"])).all(), n
        zf = cpu(rl["z_fine"])
        cots = _cots(n, 31 + n)
        gl, gc = (m.render_rays_vjp(ro, rd, near, far, cots["rgb_map"], z_fine=zf) for m in (ml, mo))
        al, ac = (m.render_rays_vjp(ro, rd, near, far, cotangents=cots, z_fine=zf) for m in (ml, mo))
        for x, y, what in ((gl, gc, "rgb gradient"), (al, ac, "gradient of all six outputs")):
            assert _same(x[0], y[0]) and _same(x[1], y[1]), (what, n)
        assert np.abs(cpu(gc[0])).max() > 0
    rng = np.random.RandomState(7)
    e_net = 0.0
    for P in POINTS:
        pts = (rng.rand(P, 3).astype(np.float32) - 0.5) * 0.4
        dirs = oracle.normalize_dirs(rng.standard_normal((P, 3)).astype(np.float32))
        for net_id, sd in ((0, sd_c), (1, sd_f)):
            ol, oc = (cpu(m.run_network(pts, dirs, net_id)) for m in (ml, mo))
            assert np.array_equal(ol, oc, equal_nan=True), (P, net_id)
            assert np.isfinite(oc).all()
            if P == 257 and net_id == 0 and views:      # (the oracle's run_network takes view directions)
                want = oracle.run_network(sd, pts[:, None], dirs)[:, 0]
                e_net = np.abs(oc - want).max()
                print("%s on chip, run_network on 257 points against the oracle: %.2e" % (name, e_net))
                assert_close(oc, want, atol=5e-5 * max(1.0, float(np.abs(want).max())), rtol=5e-5, what="run_network on %d points" % P)
    sl, sc = ml.range_status(), mo.range_status()
    assert sl == sc and sc["passes"] > 0 and sc["passes_rerun"] == 0, (sl, sc)
    ml.close()
    mo.close()


def test_a_narrow_and_a_wide_network_on_one_handle(oracle):
    """Coarse 3 x 40 with fine 3 x 256 on a handle with all three switches: the narrow network runs in the heads form, the wide one
    as the wide trunk launch plus head launches; with trunk_width=128 the wide one runs per layer.  Both give the bits of
    trunk="layers".  $NSR_WIDE_TRUNK_WIDTH reaches WideModel where it can apply."""
    from neural_sim_nerf_amd import wide
    sd_c = _scaled(oracle, 511, *NARROW)
    sd_f = _nets(oracle, "3x256")[1]
    hp = lambda sd, tw: wide.heads_plan(sd, "f16x2", "onchip", "onchip", trunk_width=tw)
    assert hp(sd_c, 256)["mode"] == "onchip" and hp(sd_c, 128) == hp(sd_c, 256)
    assert hp(sd_f, 256)["mode"] == "layers" and "128" in hp(sd_f, 256)["reason"] and hp(sd_f, 128)["mode"] == "layers"
    assert wide.trunk_plan(sd_f, "f16x2", "onchip", trunk_width=256)["tile_rows"] == 64
    assert wide.trunk_plan(sd_c, "f16x2", "onchip", trunk_width=256)["tile_rows"] == 128
    kw = dict(n_samples=3, n_importance=2, mlp="f16x2")
    ml = wide.WideModel(sd_c, sd_f, trunk="layers", **kw)
    m256 = wide.WideModel(sd_c, sd_f, trunk="onchip", heads="onchip", trunk_width=256, **kw)
    m128 = wide.WideModel(sd_c, sd_f, trunk="onchip", heads="onchip", trunk_width=128, **kw)
    ro, rd = _rays(oracle, 171, 25)
    rl, r256, r128 = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, m256, m128))
    for k in TAPS:
        assert _same(rl[k], r256[k]) and _same(rl[k], r128[k]), k
    assert np.isfinite(cpu(r256["rgb_map"])).all()
    assert ml.range_status() == m256.range_status() == m128.range_status() and ml.range_status()["passes_rerun"] == 0
    for m in (ml, m256, m128):
        m.close()
    os.environ["NSR_WIDE_TRUNK_WIDTH"] = "256"
    try:
        for trunk, mlp, want in (("onchip", "f16x2", 256), ("layers", "f16x2", 128), (None, "bf16x3", 128)):
            m = wide.WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp=mlp, trunk=trunk)
            assert m.trunk_width == want, (trunk, mlp, m.trunk_width)
            m.close()
    finally:
        del os.environ["NSR_WIDE_TRUNK_WIDTH"]
    lib, C = wide.load(), wide.C
    h = C.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, wide.FLAG_TRUNK_WIDE | wide.FLAG_MLP_F16X2)
    assert lib.nsrw_create(C.byref(cfg), C.byref(h)) != 0 and not h.value
    err = lib.nsrw_last_error().decode()
    assert "NSRW_FLAG_TRUNK_WIDE" in err and "NSRW_FLAG_TRUNK_ONCHIP" in err


@pytest.mark.parametrize("layer", [1, 2])
def test_a_value_that_leaves_the_fp16_range_in_the_wide_trunk_reruns_the_pass(layer, oracle):
    """The range safety net through the wide form: 256 rays in small chunks; every coarse pass is re-run on bf16x3 (layer by layer),
    on both handles alike -- equal counters, re-runs counted, the same bits."""
    sd_c, sd_f = _range_nets(oracle, layer)
    ro, rd = _rays(oracle, 256, 26)
    os.environ["NSR_WIDE_WORKSPACE_GB"] = "0.0001"        # the smallest workspace the library accepts: several chunks
    try:
        ml, mo = _pair(sd_c, sd_f)
        rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
        chunks = mo.last_kernel_ms()[1]
        sl, sc = ml.range_status(), mo.range_status()
        assert chunks > 1 and sl == sc and sc["passes"] > 0 and sc["passes_rerun"] > 0, (chunks, sl, sc)
        for k in TAPS:
            assert _same(rc[k], rl[k]), k
        assert np.isfinite(cpu(rc["rgb_map"])).all()
        ml.close()
        mo.close()
    finally:
        del os.environ["NSR_WIDE_WORKSPACE_GB"]


def test_hostile_rays_through_the_wide_trunk(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 256 network: every tap and the range counters
    equal the per-layer handle's; the NaN ray stays NaN, the others' colours are finite."""
    sd_c, sd_f = _nets(oracle, "3x256")
    ro, rd = _hostile(oracle)
    ml, mo = _pair(sd_c, sd_f)
    rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
    for k in TAPS:
        assert _same(rl[k], rc[k]), k
    ok = np.ones(len(ro), bool)
    ok[[3, 5, 7]] = False
    rgb = cpu(rc["rgb_map"])
    assert np.isfinite(rgb[ok]).all() and np.isnan(rgb[3]).all()
    assert ml.range_status() == mo.range_status()
    ml.close()
    mo.close()


def test_a_rays_result_in_the_wide_trunk_depends_on_nothing_but_the_ray(oracle):
    """3 x 256 at (3, 2) samples on the on-chip handle: ray 0 alone, among 63, 64 and 200 other rays (its three coarse rows share
    a 64-point block with no, with some and with a blockful of neighbours) -- the same bits each time."""
    sd_c, sd_f = _nets(oracle, "3x256")
    ro, rd = _rays(oracle, 201, 22)
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw", "raw0")
    ml, mo = _pair(sd_c, sd_f)
    ml.close()
    alone = None
    for n in (1, 64, 65, 201):
        r = mo.render_rays(ro[:n], rd[:n], oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True)
        mine = [cpu(r[k])[0] for k in keys]
        assert np.isfinite(mine[0]).all()
        alone = alone or mine
        for k, a, b in zip(keys, alone, mine):
            assert np.array_equal(a, b, equal_nan=True), (k, n)
    assert mo.range_status()["passes_rerun"] == 0
    mo.close()


def test_the_wide_trunk_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays on the wide on-chip handle; the replay on rewritten input buffers equals the eager call."""
    import torch
    from neural_sim_nerf_amd.wide import WideModel
    sd_c, sd_f = _nets(oracle, "3x192")
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 171, 27)
    m = WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp="f16x2", trunk="onchip", trunk_width=256)
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
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the bit-for-bit case at W = 136 and 256 on 171 rays"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    return [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x136", "3x256")]


def test_wide_onchip_trunk_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_trunk_h2 (tag 200000 + line).  A fresh process
    runs the two cases above on the wide on-chip handle, render_rays and run_network on 129 points; no check may trip, and every
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
from test_gpu_wide_trunk256 import _bounds_runs
out, res = {}, []
for tag, c, f, o, d in _bounds_runs(O):
    m = WideModel(c, f, n_samples=3, n_importance=2, mlp="f16x2", trunk="onchip", trunk_width=256)
    r = m.render_rays(o, d, O.YCBV_NEAR, O.YCBV_FAR, debug=True)
    rn = m.run_network(np.zeros((129, 3), np.float32) + 0.01, np.tile(np.float32([0, 0, 1]), (129, 1)), 1)
    res += [r[k].cpu().numpy() for k in ("rgb_map", "raw", "raw0", "z_fine")] + [rn.cpu().numpy()]
    out[tag] = m.debug_bounds_status() + (m.range_status()["passes_rerun"],)
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
    assert len(res["debug"]) == 2 and all(v == (True, 0, 0) for v in res["debug"].values()), res["debug"]
    assert all(v == (False, 0, 0) for v in res["release"].values()), res["release"]
    a, b = np.load(tmp_path / "debug" / "res.npz"), np.load(tmp_path / "release" / "res.npz")
    assert len(a.files) == len(b.files) == 2 * 5
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
