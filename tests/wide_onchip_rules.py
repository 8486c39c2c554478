"""Which networks the layered renderer's on-chip forms take (csrc/nsr_wide_trunk.inc; DESIGN.md 8 has the table), restated in plain
Python: arithmetic only, nothing read from the library.  tests/test_wide_{trunk,heads,trunk256,trunk_bwd}_host.py hold nsrw_trunk_plan,
nsrw_heads_plan and nsrw_trunk_bwd_plan of the built library -- the functions nsrw_upload_network itself consults -- to it."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024              # bytes of LDS one workgroup may have on gfx950


def pad32(x):
    return (x + 31) // 32 * 32


def trunk_nj(D, W, mlp, trunk):
    """None = layer by layer, else the NJ of the trunk kernel: an f16x2 handle made with trunk="onchip", at least two layers, and
    a padded width of at most 128 (one tile along N: NJ = 1 up to 64 columns, NJ = 2 for 128)"""
    if trunk != "onchip" or mlp != "f16x2" or D < 2 or pad32(W) > 128:
        return None
    return 1 if pad32(W) <= 64 else 2


def trunk_rule(D, W, mlp, trunk, trunk_width):
    """None = layer by layer, else (NJ, rows of a tile): the 128-row forms up to a padded width of 128 as ever; with trunk_width = 256
    the wide form -- 64 rows, two column blocks a wave -- for padded widths 160 .. 256 under the same other conditions"""
    nj = trunk_nj(D, W, mlp, trunk)
    if nj is not None:
        return nj, 128
    if trunk_width == 256 and trunk == "onchip" and mlp == "f16x2" and D >= 2 and 128 < pad32(W) <= 256:
        return 2, 64
    return None


def trunk_reason_128(D, W, mlp, trunk):
    """why trunk_width = 128 leaves a (valid) network layer by layer, in the library's words and its order of asking"""
    if trunk != "onchip":
        return "NSRW_FLAG_TRUNK_ONCHIP not set"
    if mlp != "f16x2":
        return "not an f16x2 handle"
    if D < 2:
        return "one layer: nothing to keep on chip"
    assert pad32(W) > 128
    return "padded width above 128"


def heads_rule(D, W, multires_views, viewdirs, mlp, trunk, heads):
    """None = a GEMM launch per head, else the NJ of the kernel that runs them: heads="onchip" on a handle whose trunk rule takes the
    network, and -- with view directions -- a direction encoding of at most 96 padded columns (it takes the encoding image over)"""
    if heads != "onchip":
        return None
    nj = trunk_nj(D, W, mlp, trunk)
    if nj is None or (viewdirs and pad32(3 + 6 * multires_views) > 96):
        return None
    return nj


def bwd_rule(D, W, multires, mlp, trunk, trunk_bwd, trunk_width):
    """None = a GEMM launch per product, else the NJ of the backward kernel: trunk_bwd="onchip" on a handle whose trunk rule takes the
    network in its 128-row form (so f16x2, two layers, a padded width of at most 128); NJ covers the wider of the two outputs, the
    hidden width and the encoding -- one column block a wave up to 64 columns, two up to 128 (a 96-column encoding has an image of
    four column blocks)"""
    if trunk_bwd != "onchip":
        return None
    t = trunk_rule(D, W, mlp, trunk, trunk_width)
    if t is None or t[1] != 128 or D < 2:
        return None
    return max(1 if pad32(W) <= 64 else 2, 1 if pad32(3 + 6 * multires) <= 64 else 2)


def bwd_reason(D, W, mlp, trunk, trunk_bwd, trunk_width):
    """why a (valid) network stays layer by layer, in the library's words and its order of asking"""
    if trunk_bwd != "onchip":
        return "NSRW_FLAG_TRUNK_BWD not set"
    t = trunk_rule(D, W, mlp, trunk, trunk_width)
    if t is None:
        return "the trunk is not on chip"
    assert t[1] == 64
    return "padded width above 128: the wide trunk has no backward form"


def trunk_lds(nj, rows=128):
    """128 rows: double-buffered weight stages of two k16 blocks x 2 NJ column blocks x 2 KiB; two fp16 piece images of the activation,
    128 rows of 64 NJ values + 16 bytes; two of the encoding, 128 rows of 96 values + 16 bytes.  The wide form: stages of two k16
    blocks x EIGHT column blocks x 2 KiB; the activation 64 rows of 256 values + 16 bytes; the encoding 64 rows of 96 values + 16 bytes"""
    if rows == 128:
        return 2 * (2 * nj * 2 * 2048) + 2 * 128 * (2 * 64 * nj + 16) + 2 * 128 * (2 * 96 + 16)
    assert (nj, rows) == (2, 64)
    return 2 * (2 * 8 * 2048) + 2 * 64 * (2 * 256 + 16) + 2 * 64 * (2 * 96 + 16)


def bwd_lds(nj):
    """double-buffered weight stages of two k16 blocks x 2 NJ column blocks x 2 KiB; two fp16 piece images of the gradient, 128 rows of
    64 NJ values + 16 bytes; no encoding image"""
    return 2 * (2 * nj * 2 * 2048) + 2 * 128 * (2 * 64 * nj + 16)


@pytest.fixture(scope="module")
def wide():
    if not os.path.exists(os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so")):
        pytest.skip("needs the built library (python -c 'import __graft_entry__ as g; g.build()')")
    from neural_sim_nerf_amd import wide
    return wide


def net(wide, D, W, multires=10, skips=(), viewdirs=True, multires_views=4):
    """the NsrwNet of a D x W network (without view directions: output_linear with five rows)"""
    skips = list(skips)
    return wide.NsrwNet(D, W, multires, multires_views if viewdirs else 0, 1 if viewdirs else 0, 4 if viewdirs else 5, len(skips),
                        (wide.C.c_int32 * wide.MAX_SKIPS)(*(skips + [0] * (wide.MAX_SKIPS - len(skips)))))
