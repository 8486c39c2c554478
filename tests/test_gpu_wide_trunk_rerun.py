"""GPU tests of the layered renderer's ON-CHIP bf16x3 RE-RUN of the trunk (kw_rerun_b3 in csrc/nsr_wide_trunk.inc;
WideModel(trunk="onchip", trunk_rerun="onchip"); run with -m gpu on an MI355X).  An f16x2 pass that leaves fp16's range is run again on
bf16x3 in launches that return at once unless the range word is set; on such a handle the pts_linears of that re-run are ONE launch
with the activations in LDS wherever the pass keeps nothing and the f16x2 trunk ran on chip in its 128-row form.  The kernel restates
the arithmetic of the per-layer bf16x3 GEMM per output element, so the handle must give the bits of a trunk_rerun="layers" handle, of
a trunk="layers" handle and -- where the pass is re-run -- of a bf16x3 handle: with and without a re-run, on both forms (128 rows up
to a padded width of 64, 64 rows at 96 and 128), through run_network, on a mixed handle, hostile rays, any company of rays, under
capture, and in the bounds-checked build.  rerun_status tells the path from a silent fallback.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from test_gpu_wide_tiles import _rays, cpu
from wide_onchip_cases import COARSE_TAPS
from wide_onchip_cases import TRUNK_NETS as NETS
from wide_onchip_cases import (_with_bias, bounds_checked_build, bounds_clean_and_equal, fine_3x136, forward_bit_for_bit, hostile_case,
                               models, range_rerun_case, small_chunks, taps_equal)
from wide_onchip_cases import hostile as _hostile
from wide_onchip_cases import trunk_nets as _nets
from wide_onchip_cases import trunk_range_nets as _range_nets

pytestmark = pytest.mark.gpu

ON = dict(trunk="onchip", trunk_rerun="onchip")           # the handle under test
OFF = dict(trunk="onchip", trunk_rerun="layers")          # the same handle with the re-run layer by layer
# name -> (padded width, rows of a re-run tile); the value leaves the range inside the trunk (layer 1: split for layer 2 in LDS) or on
# its last layer (layer 2: the re-run's fp32 output, which the re-run's head launches split)
RANGE = {"3x100-1": (128, 64), "3x100-2": (128, 64), "3x40-1": (64, 128)}


def _range(oracle, case):
    """(coarse, fine) of RANGE[case]: unit 5 of the coarse network's pts_linears.<layer> reaches 7e4 on every point"""
    if case.startswith("3x100"):
        return _range_nets(oracle, int(case[-1]))
    return _with_bias(_nets(oracle, "3x40"), "pts_linears.%s.bias" % case[-1])


def _counted(ms, log):
    """the handles `ms`, each of which appends its rerun_status count to `log` when it is closed (the shared bodies close them)"""
    for m in ms:
        def closing(m=m, close=m.close):
            log.append(m.rerun_status()["launches_onchip"])
            close()
        m.close = closing
    return ms


@pytest.mark.parametrize("heads", ["layers", "onchip"])
@pytest.mark.parametrize("case", sorted(RANGE))
def test_a_rerun_on_chip_gives_the_bits_of_the_per_layer_rerun(case, heads, oracle):
    """256 rays in 64-ray chunks at (3, 2) samples.  Every coarse pass is re-run on bf16x3, its pts_linears in one launch on the handle
    under test; no fine pass is, and its launch returns at once.  range_rerun_case on (trunk_rerun="layers", "onchip"): the coarse
    taps are a bf16x3 handle's bits, every tap the other handle's.  Then the same rays on a trunk="layers" handle too: every tap and
    the range counters equal; the handle under test enqueued one kw_rerun_b3 per pass and the others none.  heads="onchip": the re-run's
    heads are launches behind the on-chip re-run all the same."""
    from neural_sim_nerf_amd import wide
    from neural_sim_nerf_amd.wide import WideModel
    sd_c, sd_f = _range(oracle, case)
    Wp, rows = RANGE[case]
    plan = wide.trunk_rerun_plan(sd_c, "f16x2")
    assert plan["mode"] == "onchip" and (plan["nj"], plan["tile_rows"]) == (1, rows), plan
    log = []
    range_rerun_case(oracle, sd_c, sd_f, lambda: _counted(models(sd_c, sd_f, 3, 2, (dict(OFF, heads=heads), dict(ON, heads=heads))), log))
    assert log == [0, 8], log                 # per chunk the coarse and the fine pass
    near, far = oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, 256, 26)
    with small_chunks():
        ms = models(sd_c, sd_f, 3, 2, (dict(trunk="layers"), dict(OFF, heads=heads), dict(ON, heads=heads)))
        b3 = WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp="bf16x3")
        rs = [m.render_rays(ro, rd, near, far, debug=True) for m in ms + (b3,)]
        st = [m.range_status() for m in ms]
        assert ms[-1].last_kernel_ms()[1] == 4 and st[-1] == dict(st[-1], passes=8, passes_rerun=4), st
        assert all(s == st[-1] for s in st), st
        taps_equal(rs[2], rs[3], keys=COARSE_TAPS)
        for r in rs[:2]:
            taps_equal(r, rs[2])
        assert np.isfinite(cpu(rs[2]["rgb_map"])).all()
        assert [m.rerun_status()["launches_onchip"] for m in ms + (b3,)] == [0, 0, 8, 0]
        for m in ms + (b3,):
            m.close()


@pytest.mark.parametrize("name", sorted(NETS))
def test_without_a_rerun_the_launch_is_inert(name, oracle):
    """forward_bit_for_bit on (trunk="layers", trunk_rerun="layers", the handle under test): 171 rays (513 coarse rows) and 85 (255),
    run_network on 1 .. 257 points, the gradients -- every tap, every network output and every gradient the same bits, no pass
    re-run: every kw_rerun_b3 launch (there were some) found the range word clear and wrote nothing."""
    from neural_sim_nerf_amd import wide
    sd_c, sd_f = _nets(oracle, name)
    D, W, skips, views = NETS[name]
    for sd in (sd_c, sd_f):
        plan = wide.trunk_rerun_plan(sd, "f16x2")
        assert plan["mode"] == "onchip" and plan["tile_rows"] == (128 if W <= 64 else 64), plan
    log = []
    forward_bit_for_bit(oracle, _counted(models(sd_c, sd_f, 3, 2, (dict(trunk="layers"), OFF, ON)), log), sd_c, sd_f, views,
                        "%s, re-run on chip" % name)
    assert log[:2] == [0, 0] and log[2] > 0, log


@pytest.mark.parametrize("case", sorted(RANGE))
def test_a_rerun_through_run_network(case, oracle):
    """run_network on 1, 63, 64, 65, 127, 129 and 257 points of the range network (a ragged last tile of either form, one tile, several):
    every pass is re-run, and the result is the trunk_rerun="layers" handle's and a bf16x3 handle's"""
    from neural_sim_nerf_amd.wide import WideModel
    sd_c, sd_f = _range(oracle, case)
    ms = models(sd_c, sd_f, 3, 2, (OFF, ON)) + (WideModel(sd_c, sd_f, n_samples=3, n_importance=2, mlp="bf16x3"),)
    rng = np.random.RandomState(11)
    points = (1, 63, 64, 65, 127, 129, 257)
    for P in points:
        pts = (rng.rand(P, 3).astype(np.float32) - 0.5) * 0.4
        dirs = oracle.normalize_dirs(rng.standard_normal((P, 3)).astype(np.float32))
        outs = [cpu(m.run_network(pts, dirs, 0)) for m in ms]
        assert np.isfinite(outs[1]).all() and np.abs(outs[1]).max() > 0, P
        for i in (0, 2):
            assert np.array_equal(outs[i], outs[1], equal_nan=True), (P, i)
    st = [m.range_status() for m in ms[:2]]
    assert st[0] == st[1] and st[1]["passes"] == st[1]["passes_rerun"] >= len(points), st
    assert [m.rerun_status()["launches_onchip"] for m in ms] == [0, st[1]["passes"], 0]
    for m in ms:
        m.close()


@pytest.mark.parametrize("width", [128, 256])
def test_a_mixed_handle(width, oracle):
    """Coarse 3 x 100 whose every pass is re-run (on chip) with fine 3 x 136 (padded width 160: no re-run form, whether its trunk
    stays layer by layer or -- trunk_width = 256 -- takes the wide form; trunk_rerun_plan says why): the trunk_rerun="layers"
    handle's bits"""
    from neural_sim_nerf_amd import wide
    sd_c = _range(oracle, "3x100-1")[0]
    sd_f = fine_3x136(oracle)
    assert wide.trunk_rerun_plan(sd_c, "f16x2", trunk_width=width)["mode"] == "onchip"
    assert wide.trunk_rerun_plan(sd_f, "f16x2", trunk_width=width) == \
        dict(mode="layers", reason="the trunk is not on chip" if width == 128 else "padded width above 128: the wide trunk has no re-run form")
    ml, mo = models(sd_c, sd_f, 3, 2, (dict(OFF, trunk_width=width), dict(ON, trunk_width=width)))
    ro, rd = _rays(oracle, 171, 25)
    rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in (ml, mo))
    taps_equal(rl, rc)
    assert np.isfinite(cpu(rc["rgb_map"])).all()
    st = mo.range_status()
    assert ml.range_status() == st and (st["passes"], st["passes_rerun"]) == (2, 1), st
    assert (ml.rerun_status()["launches_onchip"], mo.rerun_status()["launches_onchip"]) == (0, 1)       # the coarse pass's, never the fine one's
    ml.close()
    mo.close()


def test_hostile_rays_through_a_rerun(oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays of the 3 x 100 range network: every tap and the range
    counters equal the trunk_rerun="layers" handle's (NaN in the same places), the other rays' colours finite"""
    sd_c, sd_f = _range(oracle, "3x100-1")
    ro, rd = _hostile(oracle)
    ml, mo = models(sd_c, sd_f, 3, 2, (OFF, ON))
    hostile_case(oracle, ml, mo, ro, rd)


@pytest.mark.parametrize("case", ["3x100-1", "3x40-1"])
def test_a_rays_result_behind_a_rerun_depends_on_nothing_but_the_ray(case, oracle):
    """(5, 4) samples, 300 rays of a range network on the handle under test: all rays, the same rays reversed, the first 37 alone and
    all of them in 64-ray chunks give every ray the same bits -- forward taps and the rgb gradient -- and in either chunking they are
    the trunk_rerun="layers" handle's.  (company_case's questions, asked of a handle whose every coarse pass is re-run: that body
    requires that none is.)  The chunk stays the unit of a re-run; here every chunk has one."""
    sd_c, sd_f = _range(oracle, case)
    n, near, far = 300, oracle.YCBV_NEAR, oracle.YCBV_FAR
    ro, rd = _rays(oracle, n, 22)
    cot = np.random.RandomState(23).standard_normal((n, 3)).astype(np.float32)
    keys = ("rgb_map", "disp_map", "acc_map", "z_std", "raw", "raw0")
    ml, mo = models(sd_c, sd_f, 5, 4, (OFF, ON))

    def run(m, sel):
        o, d, c = (np.ascontiguousarray(x[sel]) for x in (ro, rd, cot))
        r = m.render_rays(o, d, near, far, debug=True)
        chunks = m.last_kernel_ms()[1]
        go, gd = m.render_rays_vjp(o, d, near, far, c)
        return [cpu(r[k]) for k in keys] + [cpu(go), cpu(gd)], chunks
    whole, chunks = run(mo, slice(None))
    assert chunks == 1 and np.isfinite(whole[0]).all()
    rev, _ = run(mo, slice(None, None, -1))
    few, _ = run(mo, slice(0, 37))
    ref, _ = run(ml, slice(None))
    with small_chunks():
        cut, chunks = run(mo, slice(None))
        ref_cut, _ = run(ml, slice(None))
    assert chunks == (n + 63) // 64, chunks
    for k, a, b, c, d, e, f in zip(keys + ("grad_o", "grad_d"), whole, rev, few, cut, ref, ref_cut):
        assert np.array_equal(a, b[::-1], equal_nan=True), (k, "reversed")
        assert np.array_equal(a[:37], c, equal_nan=True), (k, "the first 37 alone")
        assert np.array_equal(a, d, equal_nan=True), (k, "64-ray chunks")
        assert np.array_equal(a, e, equal_nan=True), (k, "trunk_rerun=layers")
        assert np.array_equal(d, f, equal_nan=True), (k, "trunk_rerun=layers, 64-ray chunks")
    # the coarse pass of every forward was re-run: three one-chunk selections and the cut one, each as a render and inside a gradient call
    assert mo.range_status()["passes_rerun"] >= 2 * (3 + chunks), mo.range_status()
    assert mo.rerun_status()["launches_onchip"] > 0 and ml.rerun_status()["launches_onchip"] == 0
    ml.close()
    mo.close()


def test_the_rerun_launch_is_capturable(oracle):
    """One torch.cuda.graph capture of render_rays on the handle under test, on a range network, so that the re-run -- the launch
    that reads the range word and the head launches behind it -- is inside the captured graph; the replay on rewritten input buffers
    equals the eager call, which equals the trunk_rerun="layers" handle's.  (replay_equals_eager's body, asked of a handle whose
    coarse pass is re-run: that body requires that none is.)"""
    import torch
    sd_c, sd_f = _range(oracle, "3x100-1")
    ro, rd = _rays(oracle, 171, 27)
    ml, m = models(sd_c, sd_f, 3, 2, (OFF, ON))
    call = lambda o, d: m.render_rays(o, d, oracle.YCBV_NEAR, oracle.YCBV_FAR)
    host = lambda r: {k: cpu(v) for k, v in r.items()}
    dev = m.device
    eager = host(call(ro, rd))
    want = host(ml.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR))
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
    before = m.range_status()
    graph.replay()
    torch.cuda.synchronize(dev)
    got = host(r)
    for k in eager:
        assert np.array_equal(got[k], eager[k], equal_nan=True), k
        assert np.array_equal(eager[k], want[k], equal_nan=True), (k, "trunk_rerun=layers")
    assert np.isfinite(eager["rgb_map"]).all()
    after = m.range_status()
    assert (after["passes"] - before["passes"], after["passes_rerun"] - before["passes_rerun"]) == (2, 1), (before, after)
    assert m.rerun_status()["launches_onchip"] > 0
    ml.close()
    m.close()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: the inert launch at W = 24, 100, 128 on 171 rays, the three
    range cases and the hostile rays on a range network"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + _nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x100", "3x128")]
    ro6, rd6 = _rays(oracle, 256, 26)
    runs += [("range-" + case,) + _range(oracle, case) + (ro6, rd6) for case in sorted(RANGE)]
    runs.append(("hostile",) + _range(oracle, "3x100-1") + _hostile(oracle))
    return runs


def test_the_rerun_in_the_bounds_checked_build(tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of kw_rerun_b3 (tag 200000 + line).  A fresh process runs
    the cases above on the handle under test with a one-chunk and a 64-ray-chunk workspace; no check may trip, a pass is re-run
    exactly in the range cases, and every output equals the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_trunk_rerun", "_bounds_runs"), ON, ("16", "0.0001"), ("render", "run_network0"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 14, 5)
    assert {k: v[2] for k, v in got[0]["debug"].items()} == {k: v[2] for k, v in got[0]["release"].items()}


def test_refusals(oracle):
    """trunk_rerun="onchip" exists behind the on-chip trunk of an f16x2 handle only: WideModel says so, and nsrw_create for a caller
    of the C interface; with both flags it makes a handle, whose counter starts at 0."""
    from neural_sim_nerf_amd import wide
    sd_c = _nets(oracle, "3x40")[0]
    with pytest.raises(NotImplementedError, match="trunk_rerun=\"onchip\".*mlp='bf16x3'"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="bf16x3", trunk_rerun="onchip")
    with pytest.raises(NotImplementedError, match="trunk_rerun=\"onchip\".*trunk='layers'"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="layers", trunk_rerun="onchip")
    lib = wide.load()
    rr, on, f16, b3 = wide.FLAG_TRUNK_RERUN, wide.FLAG_TRUNK_ONCHIP, wide.FLAG_MLP_F16X2, wide.FLAG_MLP_BF16X3
    for flags, names in ((rr | f16, "NSRW_FLAG_TRUNK_RERUN needs NSRW_FLAG_TRUNK_ONCHIP"), (rr, "NSRW_FLAG_TRUNK_RERUN needs NSRW_FLAG_TRUNK_ONCHIP"),
                         (rr | b3, "NSRW_FLAG_TRUNK_RERUN needs NSRW_FLAG_TRUNK_ONCHIP"), (rr | on | b3, "needs NSRW_FLAG_MLP_F16X2"),
                         (rr | on, "needs NSRW_FLAG_MLP_F16X2")):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value, flags
        assert names in lib.nsrw_last_error().decode(), (flags, lib.nsrw_last_error())
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, rr | on | f16)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    n = ctypes.c_ulonglong(7)
    assert lib.nsrw_rerun_status(h, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.nsrw_destroy(h) == 0
