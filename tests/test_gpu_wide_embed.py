"""GPU tests of the layered renderer's ON-CHIP ENCODINGS (trunk_rows_encode in csrc/nsr_wide_trunk.inc; WideModel(trunk="onchip",
embed="onchip"); run with -m gpu on an MI355X).  On such a handle the one f16x2 launch of a pass -- trunk, heads form, wide form, kept
forward -- computes the position encodings of its block of points itself, by kw_embed's own functions, and in a heads form the
direction encodings too; behind a trunk-only launch kw_embed writes the direction encodings alone, and a kw_embed conditional on the
range word stands in front of the bf16x3 re-run.  The handle must give the bits of an embed="layers" handle and of a trunk="layers"
handle: on every network of the other on-chip tests, both ways of the heads and of the kept forward, through run_network (the points
form) and the gradients (the kept forms), with a re-run, on hostile rays, in any company of rays, under the options that change the
depths or the directions, under capture, and in the bounds-checked build.  embed_status tells the path from a silent fallback.  No
tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from test_gpu_wide_tiles import _rays, cpu
from wide_onchip_cases import (EXTRA, HEADS_NETS, TRUNK_NETS, WIDE_NETS, bounds_checked_build, bounds_clean_and_equal, bwd_nets, company_case,
                               forward_bit_for_bit, head_range_nets, heads_nets, hostile, hostile_case, models, range_rerun_case,
                               replay_equals_eager, taps_equal, trunk_nets, trunk_range_nets, wide_nets)

pytestmark = pytest.mark.gpu

# family -> (the networks, their provider, whether the handles take trunk_width=256)
FAMILIES = {"trunk": (TRUNK_NETS, trunk_nets, False), "heads": (HEADS_NETS, heads_nets, False), "wide": (WIDE_NETS, wide_nets, True),
            "extra": (EXTRA, bwd_nets, False)}
CASES = [(fam, name) for fam in sorted(FAMILIES) for name in sorted(FAMILIES[fam][0])]


def _views(fam, name):
    """whether the network takes view directions"""
    row = FAMILIES[fam][0][name]
    return {"trunk": lambda: row[3], "wide": lambda: row[3], "heads": lambda: row[3] is not None, "extra": lambda: True}[fam]()


def _modes(heads="onchip", keep="onchip", rerun="onchip", wide=False):
    """(the trunk="layers" handle, OFF, ON): ON has every on-chip option plus embed="onchip", OFF the same with embed="layers" """
    on = dict(trunk="onchip", heads=heads, trunk_bwd="onchip", trunk_keep=keep, trunk_rerun=rerun)
    if wide:
        on["trunk_width"] = 256
    return dict(trunk="layers"), dict(on, embed="layers"), dict(on, embed="onchip")


def _counted(ms, log):
    """the handles `ms`, each of which appends its embed_status to `log` when it is closed (the shared bodies close them)"""
    for m in ms:
        def closing(m=m, close=m.close):
            log.append(m.embed_status())
            close()
        m.close = closing
    return ms


@pytest.mark.parametrize("keep", ["layers", "onchip"])
@pytest.mark.parametrize("heads", ["layers", "onchip"])
@pytest.mark.parametrize("fam,name", CASES)
def test_the_encodings_on_chip_give_the_bits_of_kw_embed(fam, name, heads, keep, oracle):
    """One render of 100 rays on (trunk="layers", OFF, ON) first, for the counters: ON ran both passes with the encodings in the
    launch, with no unconditional kw_embed where the heads ran in it (or there are no view directions) and one -- the direction
    encodings alone -- per pass behind a trunk-only or wide launch; the other handles ran none on chip.  Then forward_bit_for_bit:
    171 rays (513 coarse rows) and 85 (255), run_network on 1 .. 257 points (the points form), the gradients (the kept forms) --
    every tap, every network output and every gradient the same bits on the three handles."""
    nets, provider, wide = FAMILIES[fam]
    sd_c, sd_f = provider(oracle, name)
    views = _views(fam, name)
    log = []
    ms = _counted(models(sd_c, sd_f, 3, 2, _modes(heads, keep, wide=wide)), log)
    ro, rd = _rays(oracle, 100, 29)
    rs = [m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True) for m in ms]
    for r in rs[:2]:
        taps_equal(r, rs[2], "the first render")
    st = [m.embed_status() for m in ms]
    heads_form = heads == "onchip" and not wide
    ed_only = 2 if views and not heads_form else 0
    assert st[2] == dict(passes_onchip=2, embed_launches=ed_only, embed_launches_conditional=2), (st, heads_form)
    assert st[0] == st[1] == dict(passes_onchip=0, embed_launches=2, embed_launches_conditional=0), st
    forward_bit_for_bit(oracle, ms, sd_c, sd_f, views, "%s %s, heads %s, kept forward %s, encodings on chip" % (fam, name, heads, keep))
    assert [s["passes_onchip"] for s in log[:2]] == [0, 0] and log[2]["passes_onchip"] > 2, log
    # every pass has one kw_embed on OFF; on ON a pass encoded on chip has none where the directions went with it (or there are none)
    assert log[2]["embed_launches_conditional"] == log[2]["passes_onchip"], log
    assert log[2]["embed_launches"] == log[1]["embed_launches"] - (log[2]["passes_onchip"] if heads_form or not views else 0), log


RANGE = {"trunk-1": lambda O: trunk_range_nets(O, 1), "trunk-2": lambda O: trunk_range_nets(O, 2),
         "head-feature": lambda O: head_range_nets(O, "feature"), "head-views": lambda O: head_range_nets(O, "views")}


@pytest.mark.parametrize("rerun", ["layers", "onchip"])
@pytest.mark.parametrize("case", sorted(RANGE))
def test_a_rerun_reads_the_encodings_the_conditional_launch_wrote(case, rerun, oracle):
    """range_rerun_case on (OFF, ON): 256 rays in 64-ray chunks of a 3 x 100 coarse network whose every pass leaves fp16's range --
    inside the trunk, on its last layer, or in a head, which reads the direction encodings.  The bf16x3 re-run reads k.E / k.ED from
    memory, where on ON nothing but the conditional kw_embed has put them: every tap equals OFF's, the coarse taps a bf16x3 handle's,
    the range counters are equal, and the conditional launches were enqueued."""
    sd_c, sd_f = RANGE[case](oracle)
    log = []
    range_rerun_case(oracle, sd_c, sd_f, lambda: _counted(models(sd_c, sd_f, 3, 2, _modes(rerun=rerun)[1:]), log))
    assert log[0] == dict(passes_onchip=0, embed_launches=8, embed_launches_conditional=0), log
    assert log[1] == dict(passes_onchip=8, embed_launches=0, embed_launches_conditional=8), log


@pytest.mark.parametrize("rerun", ["layers", "onchip"])
def test_a_rerun_behind_a_trunk_only_launch(rerun, oracle):
    """the same with the heads as launches: the unconditional kw_embed wrote k.ED, the conditional one k.E alone"""
    sd_c, sd_f = trunk_range_nets(oracle, 1)
    log = []
    range_rerun_case(oracle, sd_c, sd_f, lambda: _counted(models(sd_c, sd_f, 3, 2, _modes(heads="layers", rerun=rerun)[1:]), log))
    assert log[1] == dict(passes_onchip=8, embed_launches=8, embed_launches_conditional=8), log


@pytest.mark.parametrize("fam,name,heads", [("trunk", "3x100", "layers"), ("trunk", "3x100", "onchip"), ("wide", "3x136", "layers"),
                                            ("extra", "3x40-L15", "onchip")])
def test_hostile_rays(fam, name, heads, oracle):
    """A NaN origin, a zero direction and an infinite one among 100 rays (arguments of the fp64 library routine, NaN points and
    directions): every tap and the range counters equal OFF's, NaN in the same places, the other rays' colours finite"""
    sd_c, sd_f = FAMILIES[fam][1](oracle, name)
    ro, rd = hostile(oracle)
    ml, mo = models(sd_c, sd_f, 3, 2, _modes(heads, wide=FAMILIES[fam][2])[1:])
    hostile_case(oracle, ml, mo, ro, rd)


@pytest.mark.parametrize("name,heads", [("3x24", "layers"), ("3x100", "onchip")])
def test_a_rays_result_depends_on_nothing_but_the_ray(name, heads, oracle):
    """company_case on ON: reversed, the first 37 alone, 64-ray chunks -- the block a point falls into decides nothing"""
    sd_c, sd_f = trunk_nets(oracle, name)
    m, = models(sd_c, sd_f, 5, 4, _modes(heads)[2:])
    company_case(oracle, m)


@pytest.mark.parametrize("heads", ["layers", "onchip"])
def test_the_options_that_change_the_depths_or_the_directions(heads, oracle):
    """Per-ray near / far, perturb draws (t_rand, u) and caller-given view directions through render_rays on (OFF, ON): the launch
    reads the depths and the directions the stages in front of it wrote, whatever made them -- every tap equal."""
    sd_c, sd_f = trunk_nets(oracle, "3x100")
    n = 171
    ro, rd = _rays(oracle, n, 33)
    rng = np.random.RandomState(34)
    near = (oracle.YCBV_NEAR * (1.0 + 0.1 * rng.rand(n))).astype(np.float32)
    far = (oracle.YCBV_FAR * (1.0 - 0.1 * rng.rand(n))).astype(np.float32)
    vd = oracle.normalize_dirs(rng.standard_normal((n, 3)).astype(np.float32))
    options = {"near / far": dict(near=near, far=far),
               "perturb": dict(t_rand=rng.rand(n, 3).astype(np.float32), u=rng.rand(n, 2).astype(np.float32)),
               "viewdirs": dict(viewdirs=vd),
               "all": dict(near=near, far=far, t_rand=rng.rand(n, 3).astype(np.float32), u=rng.rand(n, 2).astype(np.float32), viewdirs=vd)}
    ml, mo = models(sd_c, sd_f, 3, 2, _modes(heads)[1:])
    plain = mo.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True)
    for what, extras in options.items():
        rl, rc = (m.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True, extras=extras) for m in (ml, mo))
        taps_equal(rl, rc, what)
        assert np.isfinite(cpu(rc["rgb_map"])).all(), what
        assert not np.array_equal(cpu(rc["raw"]), cpu(plain["raw"])), what          # the option reached the network
    assert mo.embed_status()["passes_onchip"] == 2 * (1 + len(options)) and ml.embed_status()["passes_onchip"] == 0
    assert mo.range_status() == dict(ml.range_status(), passes=ml.range_status()["passes"] + 2)
    ml.close()
    mo.close()


@pytest.mark.parametrize("heads", ["layers", "onchip"])
def test_the_launch_is_capturable(heads, oracle):
    """replay_equals_eager on ON: one capture of render_rays, replayed on rewritten input buffers"""
    sd_c, sd_f = trunk_nets(oracle, "3x100")
    ro, rd = _rays(oracle, 171, 27)
    m, = models(sd_c, sd_f, 3, 2, _modes(heads)[2:])
    eager = replay_equals_eager(m, ro, rd, lambda o, d: m.render_rays(o, d, oracle.YCBV_NEAR, oracle.YCBV_FAR))
    assert np.isfinite(eager["rgb_map"]).all()


def _bounds_runs(oracle):
    """[(tag, coarse, fine, rays_o, rays_d)] of the bounds-checked run: W = 24, 100, 128 and a network of the wide form on 171 rays,
    a range case (the conditional kw_embed writes) and the hostile rays (the called fallback)"""
    ro, rd = _rays(oracle, 171 + 85, 21)
    runs = [(name,) + trunk_nets(oracle, name) + (ro[:171], rd[:171]) for name in ("3x24", "3x100", "3x128")]
    runs.append(("3x136",) + wide_nets(oracle, "3x136") + (ro[:171], rd[:171]))
    ro6, rd6 = _rays(oracle, 256, 26)
    runs.append(("range-head-views",) + head_range_nets(oracle, "views") + (ro6, rd6))
    runs.append(("hostile",) + trunk_nets(oracle, "3x100") + hostile(oracle))
    return runs


@pytest.mark.parametrize("heads", ["layers", "onchip"])
def test_the_encodings_in_the_bounds_checked_build(heads, tmp_path):
    """libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every LDS and global index of the on-chip kernels, trunk_rows_encode's reads of the
    rays, the depths and the points included (tag 200000 + line).  A fresh process runs the cases above on ON with a one-chunk and a
    64-ray-chunk workspace -- render, run_network and the rgb gradient (the kept forms); no check may trip, and every output equals
    the release build's."""
    got = bounds_checked_build(tmp_path, ("test_gpu_wide_embed", "_bounds_runs"), _modes(heads, wide=True)[2], ("16", "0.0001"),
                               ("render", "run_network0", "vjp_rgb"))
    if got is None:
        pytest.skip("libnsr_debug.so not built (make -C neural_sim_nerf_amd/csrc debug)")
    bounds_clean_and_equal(got, 12, 7)
    assert {k: v[2] for k, v in got[0]["debug"].items()} == {k: v[2] for k, v in got[0]["release"].items()}


def test_refusals(oracle):
    """embed="onchip" exists behind the on-chip trunk of an f16x2 handle only: WideModel says so, and nsrw_create for a caller of the C
    interface; with the flags it needs it makes a handle, whose counters start at 0."""
    from neural_sim_nerf_amd import wide
    sd_c = trunk_nets(oracle, "3x40")[0]
    with pytest.raises(NotImplementedError, match="embed=\"onchip\".*mlp='bf16x3'"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="bf16x3", embed="onchip")
    with pytest.raises(NotImplementedError, match="embed=\"onchip\".*trunk='layers'"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="layers", embed="onchip")
    with pytest.raises(ValueError, match="embed must be one of"):
        wide.WideModel(sd_c, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip", embed="lds")
    lib = wide.load()
    em, on, f16, b3 = wide.FLAG_EMBED_ONCHIP, wide.FLAG_TRUNK_ONCHIP, wide.FLAG_MLP_F16X2, wide.FLAG_MLP_BF16X3
    needs = "NSRW_FLAG_EMBED_ONCHIP needs NSRW_FLAG_TRUNK_ONCHIP (the encodings are computed in the on-chip trunk's launch)"
    for flags, names in ((em | f16, needs), (em, needs), (em | b3, needs), (em | on | b3, "NSRW_FLAG_TRUNK_ONCHIP needs NSRW_FLAG_MLP_F16X2"),
                         (em | on, "NSRW_FLAG_TRUNK_ONCHIP needs NSRW_FLAG_MLP_F16X2")):
        h = ctypes.c_void_p()
        cfg = wide.NsrwConfig(0, 3, 0, flags)
        assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value, flags
        assert names in lib.nsrw_last_error().decode(), (flags, lib.nsrw_last_error())
    h = ctypes.c_void_p()
    cfg = wide.NsrwConfig(0, 3, 0, em | on | f16)
    assert lib.nsrw_create(ctypes.byref(cfg), ctypes.byref(h)) == 0 and h.value
    a, b, c = (ctypes.c_ulonglong(7) for _ in range(3))
    assert lib.nsrw_embed_status(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0 and (a.value, b.value, c.value) == (0, 0, 0)
    assert lib.nsrw_destroy(h) == 0
