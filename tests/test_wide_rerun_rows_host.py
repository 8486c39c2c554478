"""The row-granular re-run of the layered renderer's f16x2 passes (NSRW_FLAG_RERUN_ROWS, WideModel(rerun="rows"), $NSR_WIDE_RERUN;
DESIGN.md 8 "Row-granular re-run"): the option's resolution, the flag bit, the host restatement of the list kernel
(nsrw_rerun_rows_plan) against a numpy statement of the same rule, and the drop-in API's switch by the share of rows.  No GPU
needed; tests/test_gpu_wide_rerun_rows.py holds the kernels to the contract -- a ray's bits depend on that ray only -- and has the
workspace test, since nsrw_workspace_bytes takes a handle and a handle takes a device."""
import os
import re

import numpy as np
import pytest

from wide_onchip_rules import ROOT, wide      # (wide: the fixture)

SIZES = (1, 31, 32, 33, 255, 256, 257, 771)
TILES = (128, 256)


def np_plan(words, M, tile_rows):
    """the blocks of tile_rows rows of an M-row pass with a flagged row below M, ascending"""
    bits = np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")
    rows = np.zeros(max(M, 1), bool)
    n = min(M, bits.size)
    rows[:n] = bits[:n] != 0
    rows = rows[:M]
    return sorted(set(int(r) // tile_rows for r in np.nonzero(rows)[0]))


def words_of(rows, n_words):
    w = np.zeros(n_words, np.uint32)
    for r in rows:
        w[r // 32] |= np.uint32(1) << np.uint32(r % 32)
    return w


def test_flag_and_signatures_are_declared(wide):
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert re.search(r"enum\s*\{\s*NSRW_FLAG_RERUN_ROWS\s*=\s*\(?\s*1 << 12\s*\)?\s*\}", hdr) and wide.FLAG_RERUN_ROWS == 4096 == 1 << 12
    assert "int nsrw_range_rows_status(nsrw_handle h, unsigned long long* rows, unsigned long long* rows_rerun);" in hdr
    assert "int nsrw_rerun_rows_plan(const uint32_t* words, int64_t n_words, int64_t M, int tile_rows, int32_t* list_out, int64_t max);" in hdr
    assert {"nsrw_range_rows_status", "nsrw_rerun_rows_plan"} <= set(wide.SIGNATURES)
    # the bit collides with no other flag of the module (tests/test_wide_options_host.py takes the census of all thirteen)
    flags = {k: v for k, v in vars(wide).items() if k.startswith("FLAG_") and k != "FLAG_RERUN_ROWS"}
    assert len(flags) == 12 and not any(v & 4096 for v in flags.values()), flags
    assert sorted(flags.values()) == [1 << i for i in range(12)]
    n = wide.C.c_ulonglong(7)
    lib = wide.load()
    assert lib.nsrw_range_rows_status(None, wide.C.byref(n), wide.C.byref(n)) != 0 and "null" in lib.nsrw_last_error().decode()


@pytest.mark.parametrize("tile", TILES)
def test_rows_plan_is_the_numpy_rule(wide, tile):
    """no bit, every bit, the last row's bit alone, a bit at either side of every tile edge (alone and together), random sets -- and
    bits at rows >= M, which do not count"""
    rng = np.random.RandomState(5)
    for M in SIZES:
        nw = (M + 31) // 32
        cases = [[], list(range(M)), [M - 1], [0]]
        edges = sorted(set(r for e in range(0, M + 1, tile) for r in (e - 1, e) if 0 <= r < M))
        cases += [[r] for r in edges] + [edges]
        cases += [sorted(rng.choice(M, size=min(M, k), replace=False).tolist()) for k in (1, 2, 5)]
        for rows in cases:
            w = words_of(rows, nw)
            want = sorted(set(r // tile for r in rows))
            assert np_plan(w, M, tile) == want
            assert wide.rerun_rows_plan(w, M, tile) == want, (M, tile, rows)
            # ... and the same with every bit behind row M set as well, in the last word and in words behind it
            junk = np.concatenate([w, np.full(9, 0xffffffff, np.uint32)])
            if M % 32:
                junk[nw - 1] |= np.uint32((0xffffffff << (M % 32)) & 0xffffffff)
            assert np_plan(junk, M, tile) == want
            assert wide.rerun_rows_plan(junk, M, tile) == want, (M, tile, rows, "bits behind M")
    assert wide.rerun_rows_plan(np.zeros(0, np.uint32), 0, tile) == []
    assert wide.rerun_rows_plan(words_of([700], 25), 771, tile) == [700 // tile]       # fewer words than the pass has: the rest is clear


def test_rows_plan_counts_beyond_max_and_refuses_bad_arguments(wide):
    lib, C = wide.load(), wide.C
    w = words_of(range(771), 25)
    out = (C.c_int32 * 2)(-1, -1)
    pw = w.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.nsrw_rerun_rows_plan(pw, 25, 771, 128, out, 2) == 7 and list(out) == [0, 1]
    assert lib.nsrw_rerun_rows_plan(pw, 25, 771, 256, None, 0) == 4
    for args in ((pw, 25, 771, 64, out, 2), (pw, 25, -1, 128, out, 2), (None, 25, 771, 128, out, 2), (pw, 25, 771, 128, None, 2),
                 (pw, -1, 771, 128, out, 2), (pw, 25, 771, 128, out, -1)):
        assert lib.nsrw_rerun_rows_plan(*args) == -1 and "nsrw_rerun_rows_plan" in lib.nsrw_last_error().decode(), args[1:4]
    with pytest.raises(Exception, match="tile_rows"):
        wide.rerun_rows_plan(w, 771, 100)


def test_note_range_goes_by_the_share_of_rows_on_a_rows_handle():
    """run_nerf_noscale._note_range on stand-ins for a layered f16x2 handle: with a third of the passes re-run a "pass" handle (and one
    without the attribute) pins the network to bf16x3, as before; a rows handle with the same passes pins it only when more than a
    tenth of its ROWS were re-run, and its warning counts points"""
    import warnings
    import neural_sim_nerf_amd.run_nerf_noscale as R

    class Handle:
        mlp = "layered-f16x2"

        def __init__(self, rerun, **st):
            if rerun:
                self.rerun = rerun
            self.st = dict(last_items=0, points=0, rays=0, dropped_items=0, **st)

        def range_status(self):
            return self.st
    for rerun, rows_rerun, pinned, words in ((None, 0, True, "2 of 6 network passes"), ("pass", 0, True, "2 of 6 network passes"),
                                             ("rows", 3, False, "3 of 1000 points"), ("rows", 100, False, "100 of 1000 points"),
                                             ("rows", 101, True, "101 of 1000 points")):
        net = R.NeRF(D=2, W=8, input_ch=3, output_ch=4, skips=[], input_ch_views=3, use_viewdirs=True)
        m = Handle(rerun, passes=6, passes_rerun=2, rows=1000 if rerun == "rows" else 0, rows_rerun=rows_rerun)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            R._note_range(m, net)
            R._note_range(m, net)                                    # once per handle
        assert len(w) == 1 and words in str(w[0].message), (rerun, rows_rerun, [str(x.message) for x in w])
        assert ("_nsr_force_mlp" in net.__dict__) == pinned, (rerun, rows_rerun)
        assert ("now gets the bf16x3 GEMMs outright" in str(w[0].message)) == pinned
