"""The options of a layered handle (WideModel's nine opt-in arguments): one table, wide.KNOBS, one rule, wide.resolve_knobs, one flag
sum, wide.knob_flags -- and the library's statement of which flags go together (kFlagNeeds in csrc/nsr_wide.hip, asked through
nsrw_flags_refusal), held to the table on every combination.  No device; the library is needed for nsrw_flags_refusal only."""
import itertools
import os
import re

import pytest

from wide_onchip_rules import ROOT, wide      # (wide: the fixture -- the module with the built library, or a skip)

NAMES = ["trunk", "heads", "trunk_width", "trunk_bwd", "trunk_keep", "stages", "trunk_rerun", "embed", "rerun"]
OPT_IN_FLAGS = {"trunk": "TRUNK_ONCHIP", "heads": "HEADS_ONCHIP", "trunk_width": "TRUNK_WIDE", "trunk_bwd": "TRUNK_BWD",
                "trunk_keep": "TRUNK_KEEP", "stages": "STAGES_WAVE", "trunk_rerun": "TRUNK_RERUN", "embed": "EMBED_ONCHIP",
                "rerun": "RERUN_ROWS"}


def one(wide, name, wish, env, mlp="f16x2", trunk=None):
    """what the knob `name` resolves to on a handle of arithmetic `mlp` whose trunk is wished `trunk`"""
    return wide.resolve_knobs(mlp, {"trunk": trunk, name: wish}, env)[name]


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_the_table_has_the_nine_options_in_the_order_they_resolve():
    from neural_sim_nerf_amd import wide
    assert [k.name for k in wide.KNOBS] == NAMES
    for k in wide.KNOBS:
        assert k.on in k.values and k.on != k.values[0] and len(k.values) == 2, k
        assert k.env == "NSR_WIDE_" + k.name.upper(), k
        # a knob needs the arithmetic and knobs that resolve before it, nothing else
        assert set(k.needs) <= {"mlp"} | set(NAMES[:NAMES.index(k.name)]), k
    # every option's flag is the flag of exactly one row
    for name, flag in OPT_IN_FLAGS.items():
        assert [k.name for k in wide.KNOBS if k.flag == getattr(wide, "FLAG_" + flag)] == [name], name
    row = wide.KNOBS[NAMES.index("trunk_keep")]
    assert (row.name, row.env, row.values, row.on, row.flag) == ("trunk_keep", "NSR_WIDE_TRUNK_KEEP", ("layers", "onchip"), "onchip", 256)
    assert row.needs == dict(mlp="f16x2", trunk="onchip", trunk_bwd="onchip")
    row = wide.KNOBS[NAMES.index("embed")]
    assert (row.name, row.env, row.values, row.on, row.flag) == ("embed", "NSR_WIDE_EMBED", wide.EMBEDS, "onchip", wide.FLAG_EMBED_ONCHIP)
    assert row.needs == {"mlp": "f16x2", "trunk": "onchip"}
    assert wide.EMBEDS == ("layers", "onchip") and wide.FLAG_EMBED_ONCHIP == 1 << 11
    assert wide.RERUNS == ("pass", "rows")
    # resolve_knobs resolves all nine, the ones that used to stand beside the table too
    assert sorted(wide.resolve_knobs("f16x2", {}, {})) == sorted(NAMES)
    assert wide.resolve_knobs("f16x2", {}, {"NSR_WIDE_STAGES": "wave"})["stages"] == "wave"
    assert wide.resolve_knobs("f16x2", {"trunk": "onchip"}, {"NSR_WIDE_EMBED": "onchip"})["embed"] == "onchip"


def test_the_flags_are_thirteen_plain_globals_and_the_headers():
    from neural_sim_nerf_amd import wide
    flags = {k: v for k, v in vars(wide).items() if k.startswith("FLAG_")}
    assert len(flags) == 13 and sorted(flags.values()) == [1 << i for i in range(13)], flags
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    declared = {}
    for name, shift, value in re.findall(r"\bNSRW_FLAG_([A-Z0-9_]+)\s*=\s*\(?\s*(?:1 << (\d+)|(\d+))", hdr):
        declared[name] = 1 << int(shift) if shift else int(value)
    assert declared == {k[len("FLAG_"):]: v for k, v in flags.items()}, declared
    for name in OPT_IN_FLAGS.values():
        assert getattr(wide, "FLAG_" + name) == declared[name], name
    with pytest.raises(AttributeError):
        wide.FLAG_RERUN_ROW


def test_knob_flags_sums_the_rows_that_are_on():
    from neural_sim_nerf_amd import wide
    f = wide.knob_flags
    assert f(trunk="onchip", trunk_bwd="onchip", trunk_keep="onchip") == 16 | 128 | 256 and f(trunk="onchip", trunk_bwd="onchip") == 16 | 128
    assert f() == 0 and f(stages="wave") == 512 and f(rerun="rows") == 4096
    assert f(trunk="onchip", trunk_rerun="onchip", embed="onchip") == 16 | 1024 | 2048
    # a trunk_width of 256 says nothing without trunk="onchip"
    assert f(trunk_width=256) == 0 and f(trunk="layers", trunk_width=256, heads="onchip") == 32 and f(trunk="onchip", trunk_width=256) == 16 | 64
    for bad in (dict(trunk_width=512), dict(trunk="onchip", trunk_width=0), dict(trunk_rerun="lds"), dict(embed="lds"), dict(trunk="chip"),
                dict(stages="waves"), dict(rerun=1)):
        with pytest.raises(ValueError, match="%s must be one of" % list(bad)[-1]):
            f(**bad)
    with pytest.raises(TypeError, match="no such knob"):
        f(trunk="onchip", trunks="onchip")


# ---- the rule, option by option (each the assertions of the resolver the option used to have) ----------------------------------
def test_stages():
    from neural_sim_nerf_amd import wide
    for mlp in wide.MLPS:                                  # any arithmetic
        assert one(wide, "stages", None, {}, mlp) == "threads"
        assert one(wide, "stages", None, {"NSR_WIDE_STAGES": "wave"}, mlp) == "wave"
        assert one(wide, "stages", None, {"NSR_WIDE_STAGES": ""}, mlp) == "threads"
        assert one(wide, "stages", "threads", {"NSR_WIDE_STAGES": "wave"}, mlp) == "threads"       # the argument beats the environment
        assert one(wide, "stages", "wave", {"NSR_WIDE_STAGES": "threads"}, mlp) == "wave"
        assert one(wide, "stages", "wave", {}, mlp) == "wave"
        for wish, env in (("waves", {}), (None, {"NSR_WIDE_STAGES": "onchip"}), ("onchip", {"NSR_WIDE_STAGES": "wave"}), (1, {})):
            with pytest.raises(ValueError, match="stages must be one of"):
                one(wide, "stages", wish, env, mlp)
    # a bad wish is refused before a device is asked for (this test runs without one)
    with pytest.raises(ValueError, match="stages must be one of"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, stages="waves")


def test_trunk_keep():
    """The environment's wish is dropped where trunk_bwd is not on chip, an explicit one raises, a value that is not one of the
    knob's raises ValueError."""
    from neural_sim_nerf_amd import wide
    env = {"NSR_WIDE_TRUNK_KEEP": "onchip"}
    full = dict(trunk="onchip", heads=None, trunk_width=None, trunk_bwd="onchip", trunk_keep=None)
    assert wide.resolve_knobs("f16x2", full, env)["trunk_keep"] == "onchip"
    assert wide.resolve_knobs("f16x2", full, {})["trunk_keep"] == "layers"
    assert wide.resolve_knobs("f16x2", dict(full, trunk_keep="layers"), env)["trunk_keep"] == "layers"
    assert wide.resolve_knobs("f16x2", dict(full, trunk_keep="onchip"), {}) == \
        dict(trunk="onchip", heads="layers", trunk_width=128, trunk_bwd="onchip", trunk_keep="onchip",
             stages="threads", trunk_rerun="layers", embed="layers", rerun="pass")
    for mlp, wishes in (("f16x2", dict(full, trunk_bwd=None)), ("f16x2", dict(full, trunk_bwd="layers")),
                        ("f16x2", dict(full, trunk=None, trunk_bwd=None)), ("bf16x3", dict.fromkeys(full)), ("fp32", dict.fromkeys(full))):
        assert wide.resolve_knobs(mlp, wishes, env)["trunk_keep"] == "layers", (mlp, wishes)
        with pytest.raises(NotImplementedError, match="trunk_keep"):
            wide.resolve_knobs(mlp, dict(wishes, trunk_keep="onchip"), {})
    assert wide.resolve_knobs("f16x2", dict(full, trunk_bwd=None), dict(env, NSR_WIDE_TRUNK_BWD="onchip"))["trunk_keep"] == "onchip"
    for bad in ("bits", "on", 1):
        with pytest.raises(ValueError, match="trunk_keep must be"):
            wide.resolve_knobs("f16x2", dict(full, trunk_keep=bad), {})
    with pytest.raises(ValueError, match="trunk_keep must be"):
        wide.resolve_knobs("f16x2", full, {"NSR_WIDE_TRUNK_KEEP": "bits"})
    # (the arguments are judged before a device is asked for)
    with pytest.raises(NotImplementedError, match="trunk_keep=\"onchip\""):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip", trunk_bwd="layers", trunk_keep="onchip")


def test_trunk_rerun():
    """The environment's wish is dropped on a handle that is not f16x2 with trunk="onchip", an explicit one there raises, a value
    that is not one of the option's raises ValueError."""
    from neural_sim_nerf_amd import wide
    env = {"NSR_WIDE_TRUNK_RERUN": "onchip"}
    assert one(wide, "trunk_rerun", None, {}, "f16x2", "onchip") == "layers"
    assert one(wide, "trunk_rerun", "onchip", {}, "f16x2", "onchip") == "onchip"
    assert one(wide, "trunk_rerun", None, env, "f16x2", "onchip") == "onchip"
    assert one(wide, "trunk_rerun", "layers", env, "f16x2", "onchip") == "layers"
    assert one(wide, "trunk_rerun", "", env, "f16x2", "onchip") == "onchip"
    for mlp, trunk in (("f16x2", "layers"), ("bf16x3", "layers"), ("fp32", "layers")):
        assert one(wide, "trunk_rerun", None, env, mlp, trunk) == "layers", (mlp, trunk)
        assert one(wide, "trunk_rerun", "layers", env, mlp, trunk) == "layers", (mlp, trunk)
        with pytest.raises(NotImplementedError, match="trunk_rerun=\"onchip\".*mlp=%r, trunk=%r" % (mlp, trunk)):
            one(wide, "trunk_rerun", "onchip", {}, mlp, trunk)
    # (a bf16x3 handle with trunk="onchip" does not exist: the trunk's own row refuses it, whatever the option asks)
    for wish in (None, "layers", "onchip"):
        with pytest.raises(NotImplementedError, match="trunk=\"onchip\" exists for mlp=\"f16x2\" only"):
            one(wide, "trunk_rerun", wish, env, "bf16x3", "onchip")
    for bad in ("lds", "on", 1):
        with pytest.raises(ValueError, match="trunk_rerun must be"):
            one(wide, "trunk_rerun", bad, {}, "f16x2", "onchip")
    for mlp, trunk in (("f16x2", "onchip"), ("bf16x3", "layers")):
        with pytest.raises(ValueError, match="trunk_rerun must be"):
            one(wide, "trunk_rerun", None, {"NSR_WIDE_TRUNK_RERUN": "lds"}, mlp, trunk)
    # (the arguments are judged before a device is asked for)
    with pytest.raises(ValueError, match="trunk_rerun must be"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip", trunk_rerun="lds")
    with pytest.raises(NotImplementedError, match="trunk_rerun=\"onchip\""):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="layers", trunk_rerun="onchip")
    with pytest.raises(NotImplementedError, match="trunk_rerun=\"onchip\""):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="bf16x3", trunk_rerun="onchip")


def test_embed():
    """The environment's wish is dropped where the handle cannot honour it, an explicit one raises NotImplementedError naming what is
    missing, a value that is not one of the knob's raises ValueError."""
    from neural_sim_nerf_amd import wide
    env = {"NSR_WIDE_EMBED": "onchip"}
    assert one(wide, "embed", None, {}, "f16x2", "onchip") == "layers"
    assert one(wide, "embed", None, env, "f16x2", "onchip") == "onchip"
    assert one(wide, "embed", "layers", env, "f16x2", "onchip") == "layers"
    assert one(wide, "embed", "onchip", {}, "f16x2", "onchip") == "onchip"
    for mlp, trunk in (("bf16x3", "layers"), ("fp32", "layers"), ("f16x2", "layers")):
        assert one(wide, "embed", None, env, mlp, trunk) == "layers", (mlp, trunk)
        with pytest.raises(NotImplementedError, match="embed=\"onchip\".*mlp=%r, trunk=%r" % (mlp, trunk)):
            one(wide, "embed", "onchip", {}, mlp, trunk)
    for bad in ("lds", "on", 1):
        with pytest.raises(ValueError, match="embed must be one of"):
            one(wide, "embed", bad, {}, "f16x2", "onchip")
    with pytest.raises(ValueError, match="embed must be one of"):
        one(wide, "embed", None, {"NSR_WIDE_EMBED": "chip"}, "f16x2", "onchip")


def test_rerun():
    """The values and the default; the environment's wish is dropped on bf16x3 / fp32 handles and under trunk="onchip", an explicit
    one there raises with the resolved options in the message; an unknown value raises ValueError."""
    from neural_sim_nerf_amd import wide
    env = {"NSR_WIDE_RERUN": "rows"}
    assert one(wide, "rerun", None, {}, "f16x2", "layers") == "pass"
    assert one(wide, "rerun", "rows", {}, "f16x2", "layers") == "rows"
    assert one(wide, "rerun", None, env, "f16x2", "layers") == "rows"
    assert one(wide, "rerun", "", env, "f16x2", "layers") == "rows"
    assert one(wide, "rerun", "pass", env, "f16x2", "layers") == "pass"
    for mlp, trunk in (("bf16x3", "layers"), ("fp32", "layers"), ("f16x2", "onchip")):
        assert one(wide, "rerun", None, env, mlp, trunk) == "pass", (mlp, trunk)
        assert one(wide, "rerun", "pass", env, mlp, trunk) == "pass", (mlp, trunk)
        with pytest.raises(NotImplementedError, match="rerun=\"rows\".*mlp=%r, trunk=%r" % (mlp, trunk)):
            one(wide, "rerun", "rows", {}, mlp, trunk)
    # (a bf16x3 handle with trunk="onchip" does not exist: the trunk's own row refuses it, whatever the option asks)
    for wish in (None, "pass", "rows"):
        with pytest.raises(NotImplementedError, match="trunk=\"onchip\" exists for mlp=\"f16x2\" only"):
            one(wide, "rerun", wish, env, "bf16x3", "onchip")
    for bad in ("row", "chunk", 1):
        with pytest.raises(ValueError, match="rerun must be"):
            one(wide, "rerun", bad, {}, "f16x2", "layers")
    for mlp, trunk in (("f16x2", "layers"), ("bf16x3", "layers")):
        with pytest.raises(ValueError, match="rerun must be"):
            one(wide, "rerun", None, {"NSR_WIDE_RERUN": "row"}, mlp, trunk)
    # (the arguments are judged before a device is asked for; stages="wave" combines freely)
    with pytest.raises(ValueError, match="rerun must be"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", rerun="row")
    with pytest.raises(NotImplementedError, match="rerun=\"rows\".*mlp='f16x2', trunk='onchip'"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="f16x2", trunk="onchip", rerun="rows")
    with pytest.raises(NotImplementedError, match="rerun=\"rows\".*mlp='bf16x3', trunk='layers'"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="bf16x3", rerun="rows", stages="wave")
    with pytest.raises(NotImplementedError, match="rerun=\"rows\".*mlp='fp32'"):
        wide.WideModel(None, None, n_samples=3, n_importance=0, mlp="fp32", rerun="rows")


# ---- the rule, exhaustively -----------------------------------------------------------------------------------------------
def stated(k, got, wish, env):
    """The rule on one row, restated: the caller's wish (for a named value an empty one is none), else the environment's, else the
    default; a value that is not the row's is a ValueError; where `got` (the arithmetic and the knobs before) does not meet the row's
    needs, `on` is a NotImplementedError when the caller asked for it, and the default when the environment did."""
    asked = bool(wish) if isinstance(k.on, str) else wish is not None
    v = wish if asked else env.get(k.env) or k.values[0]
    v = int(v) if not asked and not isinstance(k.on, str) and isinstance(v, str) and v.isdigit() else v
    if v not in k.values:
        return ValueError
    met = all(got[n] == need for n, need in k.needs.items())
    return v if met or v != k.on else NotImplementedError if asked else k.values[0]


def stated_all(wide, mlp, wishes, env):
    """... over the table in its order: {knob: value}, or (the first row that raises, the exception)"""
    got = {"mlp": mlp}
    for k in wide.KNOBS:
        v = stated(k, got, wishes.get(k.name), env)
        if isinstance(v, type):
            return k, v
        got[k.name] = v
    del got["mlp"]
    return got


def outcome(wide, mlp, wishes, env):
    try:
        return wide.resolve_knobs(mlp, wishes, env)
    except (ValueError, NotImplementedError) as e:
        return type(e), str(e)


def test_every_row_follows_the_stated_rule():
    """each row x each arithmetic x each assignment of the knobs it needs x wish in {None, "", a wrong type, a wrong string, each
    value} x environment in {absent, "", wrong, each value}: the value, or the exception's type and words"""
    from neural_sim_nerf_amd import wide
    rows = {k.name: k for k in wide.KNOBS}
    count = 0
    for k in wide.KNOBS:
        named = isinstance(k.on, str)
        needed = [rows[n] for n in k.needs if n != "mlp"]
        wishes_k = (None, "", 1 if named else 1.5, "bogus") + tuple(k.values)
        envs_k = (None, "", "bogus") + tuple(str(v) for v in k.values)
        for mlp in wide.MLPS:
            for before in itertools.product(*[r.values for r in needed]):
                for wish, e in itertools.product(wishes_k, envs_k):
                    wishes = dict(zip([r.name for r in needed], before))
                    wishes[k.name] = wish
                    env = {} if e is None else {k.env: e}
                    want, got = stated_all(wide, mlp, wishes, env), outcome(wide, mlp, wishes, env)
                    case = (k.name, mlp, wishes, env, got)
                    count += 1
                    if isinstance(want, dict):
                        assert got == want, case
                        continue
                    row, exc = want
                    assert got[0] is exc, case
                    if exc is ValueError:
                        bad = wishes.get(row.name)
                        bad = bad if (bool(bad) if isinstance(row.on, str) else bad is not None) else env[row.env]
                        assert got[1] == "%s must be one of %s (got %r)" % (row.name, row.values, bad), case
                    else:
                        assert got[1].startswith("%s=%s " % (row.name, "\"%s\"" % row.on if isinstance(row.on, str) else row.on)), case
                        assert got[1].endswith("(got %s)" % ", ".join("%s=%r" % (n, mlp if n == "mlp" else wishes[n]) for n in row.needs)), case
    assert count == 3 * 6 * 5 * 18, count                  # 18: the assignments of the needed knobs, summed over the rows


# ---- the table and the library's flag table agree ---------------------------------------------------------------------------
def test_python_and_c_refuse_the_same_combinations(wide):
    """all 3 x 2^9 explicit combinations -- each arithmetic, each row at its default or `on`: resolve_knobs raises
    NotImplementedError exactly when nsrw_create would refuse the plain sum of the flags (trunk_width's not dropped), and where it
    resolves, knob_flags of the result is that sum"""
    lib = wide.load()
    before = lib.nsrw_last_error()
    refused = 0
    for mlp in wide.MLPS:
        for pick in itertools.product((False, True), repeat=len(wide.KNOBS)):
            wishes = {k.name: k.on if p else k.values[0] for k, p in zip(wide.KNOBS, pick)}
            raw = sum(k.flag for k, p in zip(wide.KNOBS, pick) if p)
            why = lib.nsrw_flags_refusal(wide._mlp_flags(mlp) | raw)
            got = outcome(wide, mlp, wishes, {})
            assert (why is not None) == (not isinstance(got, dict)), (mlp, wishes, why, got)
            if why is None:
                assert got == wishes and wide.knob_flags(**got) == raw, (mlp, wishes, got)
            else:
                assert got[0] is NotImplementedError and why.startswith(b"nsrw_create: NSRW_FLAG_"), (mlp, wishes, why, got)
                refused += 1
            # the flags that are no option's do not matter
            assert lib.nsrw_flags_refusal(wide._mlp_flags(mlp) | raw | wide.FLAG_WHITE_BKGD | wide.FLAG_LINDISP) == why
    assert 0 < refused < 3 * 2 ** len(wide.KNOBS)
    assert lib.nsrw_last_error() == before                 # a diagnostic entry: it leaves the last error alone
    f16, on = wide.FLAG_MLP_F16X2, wide.FLAG_TRUNK_ONCHIP
    assert lib.nsrw_flags_refusal(0) is None and lib.nsrw_flags_refusal(f16 | on | wide.FLAG_TRUNK_BWD | wide.FLAG_TRUNK_KEEP) is None
    assert lib.nsrw_flags_refusal(f16 | wide.FLAG_EMBED_ONCHIP) == \
        b"nsrw_create: NSRW_FLAG_EMBED_ONCHIP needs NSRW_FLAG_TRUNK_ONCHIP (the encodings are computed in the on-chip trunk's launch)"
    assert lib.nsrw_flags_refusal(f16 | on | wide.FLAG_TRUNK_KEEP) == \
        (b"nsrw_create: NSRW_FLAG_TRUNK_KEEP needs NSRW_FLAG_TRUNK_BWD (the kept on-chip forward leaves its relu masks as bits, which "
         b"only the on-chip backward trunk reads)")
    assert lib.nsrw_flags_refusal(f16 | on | wide.FLAG_RERUN_ROWS) == \
        (b"nsrw_create: NSRW_FLAG_RERUN_ROWS does not combine with NSRW_FLAG_TRUNK_ONCHIP (the on-chip forms feed one range word per "
         b"pass)")
    # the first unmet row wins: without the arithmetic it is the trunk's
    assert lib.nsrw_flags_refusal(on | wide.FLAG_RERUN_ROWS).startswith(b"nsrw_create: NSRW_FLAG_TRUNK_ONCHIP needs NSRW_FLAG_MLP_F16X2")
