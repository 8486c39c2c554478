"""The N partition of the layered renderer's GEMM (gemm_plan in csrc/nsr_wide.hip) restated in plain Python, the guard that
the widths tests/test_gpu_wide_tiles.py runs reach every tile form the library compiles: kw_gemm_* <NJ, WM> with NJ column units of
64 and WM wave rows -- <4,4> <3,4> <2,4> <1,2> at the default tile height, <4,2> <2,2> <1,2> with NSRW_B3_WM=2 -- and the check that
the restatement IS what the built library launches (nsrw_gemm_plan).  No GPU needed."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# network widths of the tile tests: the padded column count u = ncb / 2 (units of 64 columns) is 1 2 3 4 5 7 9 10
WIDTHS = (40, 100, 136, 200, 264, 392, 520, 600)
L_PTS, L_VIEWS = 4, 2               # encoding frequencies of those networks: input_ch = 27, input_ch_views = 15
ALL_FORMS = {(4, 4), (3, 4), (2, 4), (1, 2), (4, 2), (2, 2)}


def pad32(x):
    return (x + 31) // 32 * 32


def units(n_padded):
    """u of a packed matrix with n_padded rows: its 32-column blocks rounded up to an even count (col_blocks), in pairs"""
    return ((n_padded + 31) // 32 + 1) // 2


def partition(n_padded, n, wm):
    """[(NJ, WM of the kernel, tiles, first column)] of the launches gemm makes for a matrix packed with n_padded rows of which the
    caller stores n columns, on a handle with tile_wm = wm.  A part whose first column is not below n is not launched."""
    u, three = units(n_padded), wm == 4
    parts, cb = [], 0

    def part(nj, tiles):
        nonlocal cb
        if n - cb * 32 > 0:
            parts.append((nj, 4 if (nj >= 2 and wm == 4) else 2, tiles, cb * 32))
        cb += tiles * nj * 2

    if u % 4 != 0 and u % 3 == 0 and three:
        part(3, u // 3)
    else:
        if u // 4:
            part(4, u // 4)
        r = u % 4
        if r == 3 and three:
            part(3, 1)
        else:
            if r >= 2:
                part(2, 1)
            if r & 1:
                part(1, 1)
    return parts


def network_matrices(W, L=L_PTS, Lv=L_VIEWS):
    """{name: (packed rows, columns the caller stores)} of every GEMM a view-direction network of width W runs, forward (trunk and
    feature: W; alpha: 1; views: W / 2; rgb: 3) and backward (the transposed side: W, W / 2, and the encodings' Ci / Cv)"""
    Wp, W2p, Ci, Cv = pad32(W), pad32(max(W // 2, 1)), pad32(3 + 6 * L), pad32(3 + 6 * Lv)
    return {"trunk / feature / b_feat / b_head / bwd_h": (Wp, Wp), "alpha": (32, 1), "views / b_rgb": (W2p, W2p), "rgb": (32, 3),
            "bwd_e": (Ci, Ci), "b_ed": (Cv, Cv)}


def forms(W, wm):
    return {(nj, kwm) for npad, n in network_matrices(W).values() for nj, kwm, _, _ in partition(npad, n, wm)}


def test_partition_rule_on_known_widths():
    """the cases DESIGN.md section 8 names: 384 = 2 x 192 in one launch, 512 = 2 x 256; and what NSRW_B3_WM=2 makes of them"""
    assert partition(384, 384, 4) == [(3, 4, 2, 0)] and partition(384, 384, 2) == [(4, 2, 1, 0), (2, 2, 1, 256)]
    assert partition(512, 512, 4) == [(4, 4, 2, 0)] and partition(512, 512, 2) == [(4, 2, 2, 0)]
    assert partition(192, 192, 4) == [(3, 4, 1, 0)] and partition(192, 192, 2) == [(2, 2, 1, 0), (1, 2, 1, 128)]
    assert partition(448, 448, 4) == [(4, 4, 1, 0), (3, 4, 1, 256)]
    assert partition(448, 448, 2) == [(4, 2, 1, 0), (2, 2, 1, 256), (1, 2, 1, 384)]
    assert partition(32, 1, 4) == partition(32, 3, 2) == [(1, 2, 1, 0)]
    # the image is padded to an even count of 32-column blocks; a part that starts behind the last stored column is not launched
    assert units(160) == 3 and partition(160, 160, 2) == [(2, 2, 1, 0), (1, 2, 1, 128)]
    assert partition(160, 100, 2) == [(2, 2, 1, 0)]
    for npad in range(32, 1025, 32):                 # every partition covers the padded columns exactly once, in order
        for wm in (4, 2):
            at = 0
            for nj, _, tiles, col in partition(npad, npad, wm):
                assert col == at
                at += 64 * nj * tiles
            assert at == 64 * units(npad) >= npad


def test_tile_test_widths_reach_every_form():
    """WIDTHS covers u = 1 2 3 4 5 7 9 10 -- every branch of the partition under both settings -- and between them all six
    (NJ, WM) forms; the default tile height alone reaches four of them, NSRW_B3_WM=2 the other two."""
    assert [units(pad32(W)) for W in WIDTHS] == [1, 2, 3, 4, 5, 7, 9, 10]
    reach4 = set().union(*(forms(W, 4) for W in WIDTHS))
    reach2 = set().union(*(forms(W, 2) for W in WIDTHS))
    assert reach4 == {(4, 4), (3, 4), (2, 4), (1, 2)}, reach4
    assert reach2 == {(4, 2), (2, 2), (1, 2)}, reach2
    assert reach4 | reach2 == ALL_FORMS
    # each branch of the rule, by the trunk's own partition
    trunk = {W: [[(nj, t) for nj, _, t, _ in partition(pad32(W), pad32(W), wm)] for wm in (4, 2)] for W in WIDTHS}
    assert trunk[136] == [[(3, 1)], [(2, 1), (1, 1)]]                          # u = 3: one 192-column tile | 128 + 64
    assert trunk[264] == [[(4, 1), (1, 1)]] * 2                                # u = 5: 256 + 64
    assert trunk[392] == [[(4, 1), (3, 1)], [(4, 1), (2, 1), (1, 1)]]          # u = 7: 256 + 192 | 256 + 128 + 64
    assert trunk[520] == [[(3, 3)], [(4, 2), (1, 1)]]                          # u = 9: 3 x 192 | 2 x 256 + 64
    assert trunk[600] == [[(4, 2), (2, 1)]] * 2                                # u = 10: 2 x 256 + 128
    for W in WIDTHS:
        print("W %3d u %2d: default %s   NSRW_B3_WM=2 %s" % (W, units(pad32(W)), sorted(forms(W, 4)), sorted(forms(W, 2))))


def test_python_partition_is_the_librarys_launch_plan():
    """partition() above against nsrw_gemm_plan of the built library -- the function gemm iterates over when it launches -- for every
    padded width up to 1024 with the stored columns at the edges of the last block, and for every matrix of the tile tests' networks."""
    if not os.path.exists(os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so")):
        pytest.skip("needs the built library (python -c 'import __graft_entry__ as g; g.build()')")
    from neural_sim_nerf_amd import wide
    cases = {(npad, max(n, 1)) for npad in range(32, 1025, 32) for n in (1, 3, npad - 31, npad)}
    cases |= {m for W in WIDTHS for m in network_matrices(W).values()}
    for npad, n in sorted(cases):
        for wm in (4, 2):
            assert wide.gemm_plan(npad, n, wm) == partition(npad, n, wm), (npad, n, wm)
