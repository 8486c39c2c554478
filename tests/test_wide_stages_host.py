"""The opt-in wave-per-ray stages of the layered renderer (NSRW_FLAG_STAGES_WAVE, WideModel(stages="wave"); csrc/nsr_wide_stages.inc):
the option and its plan, without a device.  stage_plan is restated here in plain Python -- the LDS one ray takes per stage and the
4 / 2 / 1 rule -- and the library's is held to it; tests/test_gpu_wide_stages.py holds the kernels to the thread-per-ray ones."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 65536
SAMPLES = (3, 64, 65, 192, 640, 1024)


def lds_bytes(stage, samples, n_importance):
    """bytes of LDS one ray takes: composite five floats per sample, sample_pdf three rows of N_samples floats and the drawn samples,
    composite_bwd an fp64 and two floats per sample"""
    return {"composite": 20 * samples, "sample_pdf": 4 * (3 * samples + n_importance), "composite_bwd": 16 * samples}[stage]


def want_plan(stage, samples, n_importance):
    need = lds_bytes(stage, samples, n_importance)
    for rays in (4, 2, 1):
        if need * rays <= LDS_MAX:
            return dict(mode="wave", rays_per_group=rays, lds_bytes=need)
    return None


def cases():
    for stage in ("composite", "composite_bwd"):
        for s in SAMPLES:
            yield stage, s, 0
    for s in SAMPLES:
        if s <= 512:                                  # N_samples of a handle: 3 .. 512
            for ni in (2, 512):
                yield "sample_pdf", s, ni


def test_header_and_module_state_the_option():
    from neural_sim_nerf_amd import wide
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    assert re.search(r"enum\s*\{\s*NSRW_FLAG_STAGES_WAVE\s*=\s*512\s*\}", hdr)
    assert "int nsrw_stage_plan(int stage, int samples, int n_importance, int flags, NsrwStagePlan* plan_out);" in hdr
    assert "int nsrw_stages_status(nsrw_handle h, unsigned long long* launches_wave);" in hdr
    assert "enum { NSRW_STAGE_COMPOSITE = 0, NSRW_STAGE_SAMPLE_PDF = 1, NSRW_STAGE_COMPOSITE_BWD = 2 };" in hdr
    assert "typedef struct { int wave; int rays_per_group; int lds_bytes; char reason[96]; } NsrwStagePlan;" in hdr
    assert wide.FLAG_STAGES_WAVE == 512 and wide.STAGES == ("threads", "wave")
    assert (wide.STAGE_COMPOSITE, wide.STAGE_SAMPLE_PDF, wide.STAGE_COMPOSITE_BWD) == (0, 1, 2)
    assert {"nsrw_stage_plan", "nsrw_stages_status"} <= set(wide.SIGNATURES)
    # the flag is free: no other flag of the header has its bit
    others = [int(v) for k, v in re.findall(r"(NSRW_FLAG_[A-Z0-9_]+)\s*=\s*(\d+)", hdr) if k != "NSRW_FLAG_STAGES_WAVE"]
    assert len(others) == 9 and not any(v & 512 for v in others), others


@pytest.mark.parametrize("stage,samples,ni", list(cases()))
def test_stage_plan_is_the_stated_rule(stage, samples, ni):
    from neural_sim_nerf_amd import wide
    want = want_plan(stage, samples, ni)
    assert want is not None                           # at the renderer's limits every stage still fits with one ray per group
    got = wide.stage_plan(stage, samples, ni)
    assert got == want, (got, want)
    assert got["lds_bytes"] * got["rays_per_group"] <= LDS_MAX and got["rays_per_group"] in (4, 2, 1)
    assert wide.stage_plan(wide.STAGE_IDS[stage], samples, ni, flags=wide.FLAG_STAGES_WAVE | wide.FLAG_MLP_F16X2 | 16 | 32) == want
    for flags in (0, wide.FLAG_MLP_F16X2 | 16 | 32 | 128 | 256, wide.FLAG_WHITE_BKGD):
        assert wide.stage_plan(stage, samples, ni, flags=flags) == dict(mode="threads", reason="NSRW_FLAG_STAGES_WAVE not set")


def test_stage_plan_at_the_timed_case_and_at_the_limits():
    from neural_sim_nerf_amd import wide
    for stage, s in (("composite", 64), ("composite", 192), ("composite_bwd", 64), ("composite_bwd", 192), ("sample_pdf", 64)):
        assert wide.stage_plan(stage, s, 128)["rays_per_group"] == 4, (stage, s)
    assert wide.stage_plan("composite", 1024) == dict(mode="wave", rays_per_group=2, lds_bytes=20480)
    assert wide.stage_plan("composite_bwd", 1024) == dict(mode="wave", rays_per_group=4, lds_bytes=16384)
    assert wide.stage_plan("sample_pdf", 512, 512) == dict(mode="wave", rays_per_group=4, lds_bytes=8192)
    # n_importance is read for sample_pdf only
    assert wide.stage_plan("composite", 640, 0) == wide.stage_plan("composite", 640, 512) == dict(mode="wave", rays_per_group=4, lds_bytes=12800)
    assert wide.stage_plan("composite", 820)["rays_per_group"] == 2 and wide.stage_plan("composite", 819)["rays_per_group"] == 4
    for bad in ((3, 64, 0), ("composite", 2, 0), ("composite", 1025, 0), ("sample_pdf", 513, 2), ("sample_pdf", 64, 0), ("sample_pdf", 64, 513)):
        with pytest.raises(Exception, match="nsrw_stage_plan"):
            wide.stage_plan(*bad)
