"""Timing of the layered renderer (include/nsr_wide.h) on one 400x400 view: ms per view forward and forward + input gradient,
algorithmic fp32 TFLOP/s of the network evaluations against the fp32-MFMA peak (157.3 TFLOP/s, MI355X_MICROARCH.md) -- the
roofline of its strict mode (kw_gemm_f32: v_mfma_f32_32x32x2_f32) and the yardstick the split arithmetics (kw_gemm_h2, kw_gemm_b3: --mlp) are
quoted against; for those the issued fraction of the fp16 / bf16 peak is reported as well.

    python tools/bench_wide.py [--hw 400] [--cases ycbv,w512,d10w384,small] [--steps 3] [--trunk layers|onchip|both]
                                  [--heads layers|onchip|both] [--trunk-width 128|256|both] [--trunk-bwd layers|onchip|both]
                                  [--trunk-keep layers|onchip|both] [--stages threads|wave|both] [--trunk-rerun layers|onchip|both]
                                  [--embed layers|onchip|both] [--rerun pass|rows|both] [--cotangents rgb|all]

One argument per row of wide.KNOBS: a value of the option, or `both` for each in turn on the same rays in one process.  The table also
says which combinations a handle takes; the others are not run.

--trunk (f16x2): the pts_linears layer by layer (the default), in the one-launch on-chip trunk (csrc/nsr_wide_trunk.inc), or both in
turn on the same rays in one process -- the comparison DESIGN.md 8 quotes.  --heads (with the on-chip trunk): the heads one launch
each behind the trunk (the default), inside the trunk's launch, or both in turn.  --trunk-width (with the on-chip trunk): the largest
padded width it takes, 128 (the default), 256 (the wide form: the 8 x 160 .. 8 x 256 cases run their trunk on chip) or both in turn.
--trunk-bwd (with the on-chip trunk): the gradient call's input-gradient chain a launch per product (the default), in the one-launch
backward trunk, or both in turn.  --trunk-keep (with the on-chip backward trunk): the gradient call's kept forward a launch per layer
with fp32 activations kept (the default), in the one kept launch that leaves the relu masks as bits, or both in turn.  --trunk-rerun
(with the on-chip trunk): the conditional bf16x3 re-run of a forward pass that keeps nothing a launch per layer (the default), its
pts_linears in the one launch of kw_rerun_b3, or both in turn (d8w128range: a network whose every coarse pass is re-run).  --embed (with the on-chip trunk): the encodings of a pass
written by the kw_embed launch and read back (the default), computed inside the pass's on-chip launch, or both in turn.  --stages (any
arithmetic): compositing, resampling and the compositing backward one thread per ray (the default), one wave per ray
(csrc/nsr_wide_stages.inc), or both in turn on the same rays in one process.  --rerun (f16x2 with the per-layer trunk): the bf16x3
re-run of a pass that left fp16's range over the whole chunk (the default), over the flagged rows alone, or both in turn.  --cotangents: the gradient call differentiates rgb_map
(the default) or all six outputs (the coarse pass's backward too).
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_sim_nerf_amd import synthetic as S  # noqa: E402
from neural_sim_nerf_amd import wide  # noqa: E402
from bench import PowerSampler  # noqa: E402  (hwmon power / clock of the GPU while the launches run)

PEAK_FP32_MFMA = 157.3

# name -> (D, W, multires, multires_views, skips, N_samples, N_importance)
CASES = {
    "ycbv": (8, 256, 10, 4, [4], 64, 128),         # the fused kernels' own network, for the price of leaving them
    "w512": (8, 512, 10, 4, [4], 64, 128),
    "d10w384": (10, 384, 10, 4, [4], 64, 128),
    "w1024": (8, 1024, 10, 4, [4], 64, 128),
    "small": (4, 128, 6, 2, [1], 48, 100),
    # networks the FUSED kernels serve by re-expression at the 8 x 256 price (108 ms per view): is the layered renderer cheaper?
    "d8w64": (8, 64, 10, 4, [4], 64, 128),
    "d8w128": (8, 128, 10, 4, [4], 64, 128),
    "d8w192": (8, 192, 10, 4, [4], 64, 128),
    "d4w256": (4, 256, 10, 4, [], 64, 128),
    # the widths the wide on-chip trunk adds (--trunk-width 256), next to ycbv (8 x 256 at 64 + 128) and d8w192
    "ycbv48": (8, 256, 10, 4, [4], 48, 100),       # sample counts without a fused kernel
    "d8w160": (8, 160, 10, 4, [4], 64, 128),
    # the per-ray stages at their largest share: a small network, three coarse samples, 512 importance samples
    "s3n512": (4, 128, 6, 2, [1], 3, 512),
    # the bf16x3 re-run at its largest share (--trunk-rerun): d8w128 with a coarse network whose every pass leaves fp16's range
    "d8w128range": (8, 128, 10, 4, [4], 64, 128),
}
RANGE_CASES = ("d8w128range",)       # the coarse network's pts_linears.1 sends hidden unit 5 to 7e4 on every point
# how an option that ran both ways names itself in a result's key, in the key's order
KEY_PARTS = (("trunk", ":%s"), ("heads", ":heads-%s"), ("trunk_width", ":width-%d"), ("trunk_bwd", ":bwd-%s"), ("trunk_keep", ":keep-%s"),
             ("trunk_rerun", ":rerun-%s"), ("embed", ":embed-%s"), ("stages", ":stages-%s"), ("rerun", ":unit-%s"))


def net_sd(D, W, L, Lv, skips, seed):
    rng = np.random.RandomState(seed)
    in_ch, in_v = 3 + 6 * L, 3 + 6 * Lv
    sd = {}

    def lin(name, o, i, scale=1.0):
        b = 1.0 / np.sqrt(i)
        sd[name + ".weight"] = (rng.uniform(-b, b, (o, i)) * scale).astype(np.float32)
        sd[name + ".bias"] = rng.uniform(-b, b, (o,)).astype(np.float32)
    g = 1.6 * np.sqrt(256.0 / W)
    lin("pts_linears.0", W, in_ch, g)
    for i in range(D - 1):
        lin("pts_linears.%d" % (i + 1), W, W + in_ch if i in skips else W, g)
    lin("feature_linear", W, W)
    lin("alpha_linear", 1, W, 50.0 * 256.0 / W)
    sd["alpha_linear.bias"][:] = -0.5
    lin("views_linears.0", W // 2, W + in_v)
    lin("rgb_linear", 3, W // 2)
    return sd


def flop_per_point(sd):
    return 2 * sum(v.size for k, v in sd.items() if k.endswith(".weight"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=400)
    ap.add_argument("--cases", default="ycbv,w512,d10w384,small")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-grad", action="store_true")
    ap.add_argument("--mlp", default=None, help="bf16x3 | fp32 | f16x2 (default: the library's)")
    for k in wide.KNOBS:              # --trunk ... --rerun: one value of the option, or both in turn
        ap.add_argument("--" + k.name.replace("_", "-"), default=str(k.values[0]), choices=tuple(str(v) for v in k.values) + ("both",))
    ap.add_argument("--cotangents", default="rgb", choices=("rgb", "all"))
    a = ap.parse_args()
    # the modes: every combination of the values asked for that a handle of this arithmetic takes (wide.KNOBS says which), in the
    # table's order -- so two modes never differ in an option the handle could not honour
    mlp = a.mlp or os.environ.get("NSR_WIDE_MLP") or wide.DEFAULT_MLP
    both = {k.name: getattr(a, k.name) == "both" for k in wide.KNOBS}
    asked = [k.values if both[k.name] else tuple(v for v in k.values if str(v) == getattr(a, k.name)) for k in wide.KNOBS]
    modes, refusal = [], None
    for values in itertools.product(*asked):
        mode = dict(zip((k.name for k in wide.KNOBS), values))
        try:
            wide.resolve_knobs(mlp, mode, {})
            modes.append(mode)
        except NotImplementedError as e:
            refusal = refusal or str(e)
    if not modes:
        ap.error(refusal)
    K = S.scaled_K(400.0 / a.hw)
    pose = S.sweep_poses(1, seed=0)[0]
    out = {}
    rows = {k.name: k for k in wide.KNOBS}
    for name, mode in [(c, mode) for c in a.cases.split(",") for mode in modes]:
        D, W, L, Lv, skips, ns, ni = CASES[name]
        sd = net_sd(D, W, L, Lv, skips, 1)
        sd_c = sd
        if name in RANGE_CASES:
            sd_c = {k: v.copy() for k, v in sd.items()}
            sd_c["pts_linears.1.bias"][5] += 7.0e4
        m = wide.WideModel(sd_c, sd, n_samples=ns, n_importance=ni, mlp=mlp, **mode)
        n = a.hw * a.hw
        evals = n * (ns + ns + ni)
        flop = evals * flop_per_point(sd)
        ro, rd = m.get_rays(a.hw, a.hw, K, torch.tensor(pose[:3, :4]))
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        torch.manual_seed(0)              # every mode and every process differentiates the same cotangent (a borderline f16x2 re-run
        cot = torch.randn(n, 3, device=m.device)      # of the backward depends on it: 8 x 64 re-ran one or two passes per call unseeded)
        cots = None
        if a.cotangents == "all":
            cots = {k: torch.randn((n, 3) if k in ("rgb_map", "rgb0") else (n,), device=m.device) for k in
                    ("disp_map", "acc_map", "rgb0", "disp0", "acc0")}
            cots["rgb_map"] = cot
        res = {"network": "%d x %d, skips %s, %d + %d samples" % (D, W, skips, ns, ni), "rays": n,
               "flop_per_point": flop_per_point(sd), "mlp": m.mlp, "trunk": m.trunk, "heads": m.heads,
               "trunk_width": m.trunk_width, "trunk_bwd": m.trunk_bwd, "trunk_keep": m.trunk_keep, "trunk_rerun": m.trunk_rerun,
               "embed": m.embed, "stages": m.stages, "rerun": m.rerun,
               "cotangents": a.cotangents}
        for what in ("forward",) + (() if a.no_grad else ("forward+input-gradient",)):
            ms = []
            ps = None
            for it in range(a.steps + 1):
                if it == 1:
                    ps = PowerSampler(m.device.index)
                    ps.start()
                if what == "forward":
                    m.render_rays(ro, rd, S.YCBV_NEAR, S.YCBV_FAR)
                elif cots:
                    m.render_rays_vjp(ro, rd, S.YCBV_NEAR, S.YCBV_FAR, cotangents=cots)
                else:
                    m.render_rays_vjp(ro, rd, S.YCBV_NEAR, S.YCBV_FAR, cot)
                t, chunks = m.last_kernel_ms()
                ms.append(t)
            power = ps.stop() if ps else None
            t = float(np.median(ms[1:]))
            f = flop if what == "forward" else flop + n * (ns + ni) * flop_per_point(sd)     # + the fine pass's transposed GEMMs
            if what != "forward" and cots:
                f += 2 * n * ns * flop_per_point(sd)                                          # + the coarse pass again, and its transposed GEMMs
            res[what] = {"ms_per_view": round(t, 2), "ms_min_max": [round(min(ms[1:]), 2), round(max(ms[1:]), 2)], "chunks": chunks, "workspace_GB": round(m.workspace_bytes / 2 ** 30, 2),
                         "algorithmic_TFLOPs": round(f / t / 1e9, 1), "frac_of_fp32_mfma_peak": round(f / t / 1e9 / PEAK_FP32_MFMA, 3)}
            if m.mlp.endswith("bf16x3"):       # six bf16 piece products per product: ceiling 2500 / 6 TFLOP/s of algorithmic work
                res[what]["issued_frac_of_bf16_peak"] = round(6 * f / t / 1e9 / 2500.0, 3)
            if m.mlp.endswith("f16x2") and what == "forward":       # three fp16 piece products per product (the gradient GEMMs are bf16x3)
                res[what]["issued_frac_of_fp16_peak"] = round(3 * f / t / 1e9 / 2500.0, 3)
            if power:
                res[what]["power_and_clock"] = {k: v for k, v in power.items() if k != "source"}
            if what == "forward":
                res[what]["Mray_samples_per_s"] = round(n * (ns + ni) / t / 1e3, 2)
        if m.mlp.endswith("f16x2"):
            res["range_status"] = m.range_status()
            res["keep_status"] = m.keep_status()
            res["rerun_status"] = m.rerun_status()
            res["embed_status"] = m.embed_status()
        # an option that ran both ways names itself in the key where the mode lets it be on (heads: in every mode)
        key = name + "".join(part % mode[n] for n, part in KEY_PARTS if both[n] and
                             (n == "heads" or all(mode[o] == need for o, need in rows[n].needs.items() if o != "mlp")))
        out[key] = res
        print(key, json.dumps(res), flush=True)
        m.close()
        del m
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
