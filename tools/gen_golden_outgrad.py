"""Writes tests/golden/g28_output_grads.npz: the reference's autograd of EVERY differentiable output of render_rays (RN:488-494:
rgb_map, disp_map, acc_map and the coarse rgb0 / disp0 / acc0) with respect to the rays (and to given view directions), each
output alone and all of them together, on seven cases (tests/test_gpu_output_grads.py reads it):

    A  synthetic pair (oracle/nerf_oracle.synth_weights, seed 7 -- g3's), 64 + 128 samples, view directions from the rays
    B  the trained pair of g26_trained.npz (read as tests/conftest.trained_pair reads it) on its grad_rays_in rays
    C  A with white_bkgd=True (RN:384-385)
    D  A's coarse network alone (N_importance = 0)
    E  A's networks with a density bias so negative that sigma <= 0 at every sample: acc == 0, disp = NaN (RN:381)
    F  g25's 6 x 300 two-skip network ("b") at 48 + 100 samples (only the layered renderer serves it)
    G  given view directions (another camera's, as c2w_staticcam RN:91-96 makes them), perturb=1, raw_noise_std=1 with the
       reference's own draws recorded

    python tools/gen_golden_outgrad.py          (needs the reference's source tree; CPU only)

Nothing of the reference is stored: rays, draws, seeded cotangents, its sorted fine depths (z_vals after RN:477, constants of the
gradient because z_samples is detached, RN:475), its forward outputs and its gradients."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as G  # noqa: E402  (import_reference: the reference with its CUDA calls shimmed)
import nerf_oracle as O  # noqa: E402  (weights recipe, camera constants)

OUTS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0")
SEED = 7
E_BIAS = -1000.0        # case E: alpha_linear.bias of both networks (the generator checks sigma <= 0 at every sample)
F_SHAPE = (6, 300, 6, 2, [1, 3], True, 48, 100)       # g25 "b": D, W, multires, multires_views, skips, use_viewdirs, N_samples, N_importance


def f_weights():
    """Case F's (coarse, fine) state dicts, exactly as oracle/gen_golden_r5.py makes g25's "b"."""
    D, W, L, Lv, skips, uv, _, _ = F_SHAPE
    sdc = O.synth_weights_shape(SEED + 41, D, W, L, Lv, skips, uv)
    sdf = {k: (v * (1.0 + 0.05 * np.random.RandomState(SEED + 42).standard_normal(v.shape))).astype(np.float32)
           for k, v in sdc.items()}
    return sdc, sdf


def trained_pair(g):
    sd_c = {k[2:]: np.asarray(g[k], np.float32) for k in g.files if k.startswith("c.")}
    sd_f = {k[2:]: np.asarray(g[k], np.float32) for k in g.files if k.startswith("f.")}
    return sd_c, sd_f


def main():
    RN, RH, LL = G.import_reference()
    torch.autograd.set_detect_anomaly(False)       # (the reference switches it on: it would raise on the NaN gradients E records)
    torch.manual_seed(0)
    rng = np.random.RandomState(2828)

    def nets_of(sds, D=8, W=256, L=10, Lv=4, skips=(4,), uv=True):
        ef, in_ch = RH.get_embedder(L, 0)
        edf, in_v = RH.get_embedder(Lv, 0) if uv else (None, 0)
        out = []
        for sd in sds:
            net = RH.NeRF(D=D, W=W, input_ch=in_ch, output_ch=5, skips=list(skips), input_ch_views=in_v, use_viewdirs=uv)
            net.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
            out.append(net)
        q = lambda inputs, viewdirs, fn: RN.run_network(inputs, viewdirs, fn, embed_fn=ef, embeddirs_fn=edf, netchunk=65536)
        return out, q

    z_seen = []
    orig_r2o = RN.raw2outputs

    def r2o(raw, z_vals, *a, **k):
        z_seen.append(z_vals.detach().numpy().copy())
        return orig_r2o(raw, z_vals, *a, **k)
    RN.raw2outputs = r2o

    drawn = []
    orig_rand, orig_randn = torch.rand, torch.randn

    def rec(fn):
        def w(*a, **k):
            out = fn(*a, **k)
            drawn.append(out.detach().numpy().copy())
            return out
        return w

    res = {}

    def case(tag, nets, q, ro, rd, ns=64, ni=128, white=False, vd_given=None, perturb=0.0, std=0.0):
        n = len(ro)
        ro_t = torch.from_numpy(ro).clone().requires_grad_(True)
        rd_t = torch.from_numpy(rd).clone().requires_grad_(True)
        inputs = [ro_t, rd_t]
        if vd_given is not None:
            vd = torch.from_numpy(vd_given).clone().requires_grad_(True)
            inputs.append(vd)
        else:
            vd = rd_t / torch.norm(rd_t, dim=-1, keepdim=True)               # RN:97
        near, far = O.YCBV_NEAR * torch.ones(n, 1), O.YCBV_FAR * torch.ones(n, 1)
        batch = torch.cat([ro_t, rd_t, near, far, vd.float()], -1)            # RN:109-112
        del z_seen[:], drawn[:]
        if perturb > 0 or std > 0:
            torch.rand, torch.randn = rec(orig_rand), rec(orig_randn)
        try:
            ret = RN.render_rays(batch, network_fn=nets[0], network_query_fn=q, N_samples=ns, retraw=False, lindisp=False,
                                 perturb=perturb, N_importance=ni, network_fine=nets[1] if ni > 0 else None, white_bkgd=white,
                                 raw_noise_std=std)
        finally:
            torch.rand, torch.randn = orig_rand, orig_randn
        outs = [k for k in OUTS if k in ret]
        d = {"rays_o": ro, "rays_d": rd, "shape": np.array([ns, ni, int(white)])}
        if vd_given is not None:
            d["viewdirs"] = vd_given
        if perturb > 0 or std > 0:
            names = ["t_rand", "noise0", "u", "noise1"] if ni > 0 else ["t_rand", "noise0"]
            assert len(drawn) == len(names), [x.shape for x in drawn]
            for name, x in zip(names, drawn):
                d[name] = x * np.float32(std) if name.startswith("noise") else x
        d["z_fine"] = z_seen[-1]                                              # the last pass's depths (sorted, RN:477)
        cots = {}
        for k in outs:
            sh = tuple(ret[k].shape)
            cots[k] = torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
            d["cot_" + k] = cots[k].numpy()
            d["fwd_" + k] = ret[k].detach().numpy()

        def grad(keys):
            gs = torch.autograd.grad([ret[k] for k in keys], inputs, grad_outputs=[cots[k] for k in keys], retain_graph=True)
            return [x.numpy() for x in gs]
        for k in outs + ["all"]:
            gs = grad(outs if k == "all" else [k])
            d["grad_o_" + k], d["grad_d_" + k] = gs[0], gs[1]
            if vd_given is not None:
                d["grad_v_" + k] = gs[2]
        res.update({tag + "_" + k: v for k, v in d.items()})
        print(tag, n, "rays", ns, "+", ni, {k: int(np.isnan(d["grad_d_" + k]).sum()) for k in outs + ["all"]})
        return ret

    # the YCB-V camera of g6 / g14 (LL:89-94 pose, RH:156-165 rays)
    poses = np.stack([LL.pose_spherical_nograd(t, p, 1.01).numpy() for t, p in ((90.0, 30.0 - 180.0), (94.2, 311.0 - 180.0))])
    o32, d32 = RH.get_rays(400, 400, O.YCBV_K, torch.from_numpy(poses[0])[:3, :4])
    _, d_other = RH.get_rays(400, 400, O.YCBV_K, torch.from_numpy(poses[1])[:3, :4])
    o32, d32, d_other = o32.reshape(-1, 3).numpy(), d32.reshape(-1, 3).numpy(), d_other.reshape(-1, 3).numpy()
    # half of the rays through the middle of the view (where the synthetic scene is dense), half anywhere
    mid = np.flatnonzero((np.abs(np.arange(160000) // 400 - 200) < 60) & (np.abs(np.arange(160000) % 400 - 200) < 60))
    sel = np.concatenate([rng.choice(mid, 32, replace=False), rng.choice(160000, 32, replace=False)])
    ro, rd = o32[sel].astype(np.float32), d32[sel].astype(np.float32)

    sd_c = O.synth_weights(SEED)
    sd_f = O.synth_weights(SEED + 1000, fine_of=sd_c)
    nets, q = nets_of((sd_c, sd_f))
    case("a", nets, q, ro, rd)
    g26 = np.load(os.path.join(ROOT, "tests", "golden", "g26_trained.npz"))
    nets_b, q_b = nets_of(trained_pair(g26))
    gro, grd = g26["grad_rays_in"]
    case("b", nets_b, q_b, gro[:128].astype(np.float32), grd[:128].astype(np.float32))
    case("c", nets, q, ro, rd, white=True)
    case("d", nets, q, ro, rd, ni=0)
    sd_ce = dict(sd_c, **{"alpha_linear.bias": np.array([E_BIAS], np.float32)})
    sd_fe = dict(sd_f, **{"alpha_linear.bias": np.array([E_BIAS], np.float32)})
    nets_e, q_e = nets_of((sd_ce, sd_fe))
    ret = case("e", nets_e, q_e, ro[:16], rd[:16])
    assert (ret["acc_map"] == 0).all() and (ret["acc0"] == 0).all(), "case E: sigma > 0 somewhere -- lower E_BIAS"
    D, W, L, Lv, skips, uv, ns, ni = F_SHAPE
    nets_f, q_f = nets_of(f_weights(), D, W, L, Lv, skips, uv)
    case("f", nets_f, q_f, ro, rd, ns=ns, ni=ni)
    vd = d_other[sel] / np.linalg.norm(d_other[sel], axis=-1, keepdims=True)
    case("g", nets, q, ro, rd, vd_given=vd.astype(np.float32), perturb=1.0, std=1.0)
    RN.raw2outputs = orig_r2o

    path = os.path.join(ROOT, "tests", "golden", "g28_output_grads.npz")
    np.savez_compressed(path, e_bias=np.float32(E_BIAS), seed=np.int64(SEED), **res)
    print("%s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
