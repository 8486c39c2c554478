"""Times the gradient of render()'s outputs through the drop-in API: one 400 x 400 view, 64 + 128 samples, the
synthetic pair on the default f16x2 handles -- rgb only (the fused VJP kernels, for comparison), rgb + rgb0 and all six outputs
(the layered twin, run_nerf_noscale._vjp_route) -- and a 64 x 64 coarse-only view (N_importance = 0: the twin).  Each figure is
the median device-synchronised wall time of forward + torch.autograd.grad over --reps runs after --warmup.

    python tools/bench_output_grads.py [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nerf_oracle as O  # noqa: E402
import neural_sim_nerf_amd.run_nerf_noscale as R  # noqa: E402


def nets(n_importance):
    sd_c = O.synth_weights(7)
    sd_f = O.synth_weights(1007, fine_of=sd_c)
    out = []
    for sd in (sd_c, sd_f)[:2 if n_importance else 1]:
        net = R.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        out.append(net.to(R.device))
    return dict(network_query_fn=None, perturb=False, N_importance=n_importance, network_fine=out[1] if n_importance else None,
                N_samples=64, network_fn=out[0], use_viewdirs=True, white_bkgd=False, raw_noise_std=0., ndc=False, lindisp=False,
                near=O.YCBV_NEAR, far=O.YCBV_FAR)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    res = {}
    for side, ni, sets in ((400, 128, {"rgb": ["rgb_map"], "rgb+rgb0": ["rgb_map", "rgb0"],
                                       "all6": ["rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0"]}),
                           (64, 0, {"coarse_only_all3": ["rgb_map", "disp_map", "acc_map"]})):
        kw = nets(ni)
        K = O.scaled_K(400.0 / side)
        c2w = torch.from_numpy(O.pose_spherical(90.0, -150.0, 1.01).astype(np.float32))
        model = R._model_for(kw["network_fn"], kw["network_fine"], ni, kw)
        ro, rd = model.get_rays(side, side, K, c2w[:3, :4].to(model.device))
        rays = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)]).contiguous()
        gen = torch.Generator(device="cpu").manual_seed(0)
        for name, keys in sets.items():
            def run():
                r = rays.detach().requires_grad_(True)
                rgb, disp, acc, ex = R.render(side, side, K, rays=r, **kw)
                outs = dict(rgb_map=rgb, disp_map=disp, acc_map=acc, **{k: ex[k] for k in ("rgb0", "disp0", "acc0") if k in ex})
                cots = [torch.randn(outs[k].shape, generator=gen).to(rgb.device) for k in keys]
                torch.autograd.grad([outs[k] for k in keys], r, grad_outputs=cots)
            ms = timed(run, a.reps, a.warmup)
            res["%dx%d_%s" % (side, side, name)] = dict(ms=round(ms, 2), route=model.last_vjp_route)
            print("%4d x %-4d %-18s %9.2f ms  route %s" % (side, side, name, ms, model.last_vjp_route), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
