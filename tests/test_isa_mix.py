"""The layer block of k_render_h2 in the compiler's output (tools/isa_mix.py): no GPU, hipcc only (about 40 s).

With one wave per SIMD, every instruction that sits before the first or after the last MFMA of a layer's 384-MFMA block is
issued with the matrix pipe idle.  The epilogue of a layer and the bias load of the next one run inside the last k16 block
of the GEMM (tail_h2, nsr_h2.inc); this test keeps them there and keeps the register allocator's copies out."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/isa_mix.py on nsr_fused_h2.hip at commit 31c3873 (the parent of the change that introduced tail_h2), block of 384
# MFMAs of k_render_h2: lead-in 1 + before 145 + after 272 instructions (of them 112 + 128 v_accvgpr_*, 80 of those
# v_accvgpr_mov_b32; profiles/r07/isa_mix_before.txt).  The bias load of that commit -- 65 more instructions in a block of
# its own elsewhere in the loop -- is NOT in this figure, so the bound below is the stricter reading of "half".
PARENT_OUTSIDE = 418


def _tool():
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def h2_blocks(tmp_path_factory):
    tool = _tool()
    if not (os.path.exists(tool.hipcc_path()) or shutil.which(tool.hipcc_path())):
        pytest.skip("hipcc not installed")
    asm = str(tmp_path_factory.mktemp("isa") / "nsr_fused_h2.s")
    tool.compile_to_asm(os.path.join(tool.CSRC, "nsr_fused_h2.hip"), asm)
    with open(asm) as f:
        res = tool.analyse(f.read(), min_mfma=24, kernel="k_render_h2")
    print(tool.report(res))
    return res["k_render_h2"]


def test_layer_block_of_k_render_h2(h2_blocks):
    layer = [b for b in h2_blocks if b["mfma"] == 384]
    assert len(layer) == 1, "one block of exactly 384 MFMAs (layers 1..8): %r" % [b["mfma"] for b in h2_blocks]
    b = layer[0]
    print("layer block %s: lead-in %d, before %d, after %d, outside %d (parent %d); accvgpr_mov %d; VALU-class in the last "
          "23 gaps %d" % (b["label"], b["n_lead"], b["n_before"], b["n_after"], b["outside"], PARENT_OUTSIDE, b["acc_mov"],
                          b["tail_valu"]))
    assert b["acc_mov"] == 0, "v_accvgpr_mov_b32 in the layer block: the allocator shuffles accumulators again"
    assert 2 * b["outside"] <= PARENT_OUTSIDE, "instructions outside the first-to-last-MFMA span: %d > %d / 2" % (
        b["outside"], PARENT_OUTSIDE)
