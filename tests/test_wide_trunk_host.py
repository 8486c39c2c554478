"""Which networks the layered renderer's on-chip trunk (kw_trunk_h2 in csrc/nsr_wide_trunk.inc) takes, restated in plain Python and
held against nsrw_trunk_plan of the built library -- the function nsrw_upload_network itself consults.  No GPU needed."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024              # bytes of LDS one workgroup may have on gfx950


def pad32(x):
    return (x + 31) // 32 * 32


def rule(D, W, mlp, trunk):
    """None = layer by layer, else the NJ of the trunk kernel: an f16x2 handle made with trunk="onchip", at least two layers, and
    a padded width of at most 128 (one tile along N: NJ = 1 up to 64 columns, NJ = 2 for 128)"""
    if trunk != "onchip" or mlp != "f16x2" or D < 2 or pad32(W) > 128:
        return None
    return 1 if pad32(W) <= 64 else 2


def lds_bytes(nj):
    """double-buffered weight stages of two k16 blocks x 2 NJ column blocks x 2 KiB; two fp16 piece images of the activation, 128 rows
    of 64 NJ values + 16 bytes; two of the encoding, 128 rows of 96 values + 16 bytes"""
    return 2 * (2 * nj * 2 * 2048) + 2 * 128 * (2 * 64 * nj + 16) + 2 * 128 * (2 * 96 + 16)


@pytest.fixture(scope="module")
def wide():
    if not os.path.exists(os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so")):
        pytest.skip("needs the built library (python -c 'import __graft_entry__ as g; g.build()')")
    from neural_sim_nerf_amd import wide
    return wide


def _net(wide, D, W, multires=10, skips=(), viewdirs=True):
    skips = list(skips)
    return wide.NsrwNet(D, W, multires, 4 if viewdirs else 0, 1 if viewdirs else 0, 4 if viewdirs else 5, len(skips),
                        (wide.C.c_int32 * wide.MAX_SKIPS)(*(skips + [0] * (wide.MAX_SKIPS - len(skips)))))


def test_trunk_plan_is_the_rule(wide):
    assert [rule(3, W, "f16x2", "onchip") for W in (24, 40, 64, 100, 128, 129, 136, 256)] == [1, 1, 1, 2, 2, None, None, None]
    assert rule(1, 64, "f16x2", "onchip") is None and rule(8, 64, "bf16x3", "onchip") is None and rule(8, 64, "f16x2", "layers") is None
    for W in (2, 24, 32, 33, 40, 64, 65, 96, 100, 128, 129, 136, 160, 256, 1024):
        for D in (1, 2, 3, 8, 64):
            for mlp in wide.MLPS:
                for trunk in wide.TRUNKS:
                    for multires in (0, 4, 10, 15):
                        skips = [s for s in (0, 4) if s < D - 1]
                        plan = wide.trunk_plan(_net(wide, D, W, multires, skips), mlp, trunk)
                        want = rule(D, W, mlp, trunk)
                        case = (W, D, mlp, trunk, multires)
                        if want is None:
                            assert plan["mode"] == "layers" and plan["reason"], case
                        else:
                            assert plan == dict(mode="onchip", nj=want, tile_rows=128, lds_bytes=lds_bytes(want)), (case, plan)
                            assert plan["lds_bytes"] <= LDS_LIMIT == 163840, case
    # the cases the issue names, one by one
    on = lambda W, D=3, mlp="f16x2", L=10: wide.trunk_plan(_net(wide, D, W, L, [0]), mlp)
    assert [on(W)["nj"] for W in (24, 40, 64)] == [1, 1, 1] and [on(W)["nj"] for W in (100, 128)] == [2, 2]
    assert all(on(W)["mode"] == "layers" for W in (129, 136, 256))
    assert wide.trunk_plan(_net(wide, 1, 64), "f16x2")["mode"] == "layers"
    assert on(64, mlp="bf16x3")["mode"] == "layers" and on(64, mlp="fp32")["mode"] == "layers"
    assert on(128, L=15)["lds_bytes"] <= LDS_LIMIT and pad32(3 + 6 * 15) == 96        # multires = 15: the widest encoding there is
    assert wide.trunk_plan(_net(wide, 3, 64), "f16x2", trunk="layers")["mode"] == "layers"


def test_trunk_plan_reads_state_dicts_and_refuses_invalid_networks(wide, oracle):
    sd = oracle.synth_weights_shape(1, 3, 40, 4, 2, [1], True)
    assert wide.trunk_plan(sd, "f16x2") == dict(mode="onchip", nj=1, tile_rows=128, lds_bytes=lds_bytes(1))
    assert wide.trunk_plan(oracle.synth_weights_shape(1, 3, 136, 4, 2, [1], True), "f16x2")["mode"] == "layers"
    assert wide.trunk_plan(oracle.synth_weights_shape(1, 3, 40, 4, 2, [0], False), "f16x2")["nj"] == 1
    from neural_sim_nerf_amd import _lib
    with pytest.raises(_lib.NsrError, match="netwidth"):
        wide.trunk_plan(_net(wide, 3, 1), "f16x2")


def test_flag_and_signature_are_declared(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert "NSRW_FLAG_TRUNK_ONCHIP = 16" in hdr and wide.FLAG_TRUNK_ONCHIP == 16
    assert "int nsrw_trunk_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);" in hdr
    assert "200000 + the line" in hdr
