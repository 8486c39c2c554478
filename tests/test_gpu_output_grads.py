"""GPU tests of the gradient of EVERY differentiable output of render() (rgb_map, disp_map, acc_map, rgb0, disp0, acc0; RN:488-494)
with respect to the rays, against the reference's own autograd (tests/golden/g28_output_grads.npz, tools/gen_golden_outgrad.py):
the layered renderer's nsrw_render_rays_vjp_cot directly, and the drop-in API's autograd, which routes every backward the
fused VJP kernels do not serve to the layered twin of the fused handle (run_nerf_noscale._vjp_route)."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden
from test_output_grads_host import CASES, case_nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

OUTS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0")
P90, NORM = 3e-4, 2e-2          # the r06 bounds of the rgb gradient on the trained pair (tests/test_gpu_r6.py)
# disp / acc: acc = sum(w) of a nearly opaque ray is 1 - (a few ulp) and its gradient a near-cancelling sum the reference itself
# rounds in fp32, and disp = depth / acc of a nearly empty ray divides by a small acc (case F's coarse pass: p90 2.2e-3 on the
# fp32-MFMA arithmetic as on the others, relative norm 8e-6): the 90th percentile bound is 3e-3 there
P90_DISP_ACC = 3e-3
# the drop-in API differentiates at its OWN resampled depths, a few ulp from the reference's (the 2^9 x frequencies of the encoding
# amplify them): the 90th percentile bound is 1e-2 there, the norm bound the same
P90_DROPIN = 1e-2
FLOOR = 1e-3                    # rows below this fraction of the largest row's norm are measured against the floor (_rel_rows)


def cpu(t):
    return t.detach().cpu().numpy()


def _rel_rows(a, b):
    """|a - b| / |b| per row, |b| floored at 1e-4 of the largest row's: a row whose reference gradient is rounding noise of a
    constant -- acc (and the acc part of disp) of an opaque ray is exactly 1.0 in fp32, its gradient ~1e-7 against ~1e2 for the
    others -- is measured against the gradient's scale, not against its own noise."""
    nb = np.linalg.norm(b, axis=1)
    floor = FLOOR * nb.max() if len(nb) else 0.0
    return np.linalg.norm(a - b, axis=1) / (np.maximum(nb, floor) + 1e-12)


def _outs(g, tag):
    return [k for k in OUTS if "%s_cot_%s" % (tag, k) in g.files]


def _extras(g, tag):
    ex = {k: g["%s_%s" % (tag, k)] for k in ("viewdirs", "t_rand", "noise0", "u", "noise1") if "%s_%s" % (tag, k) in g.files}
    return ex or None


def _check(what, a, b, rows=None, p90_bound=P90):
    """NaN exactly where the reference has NaN; on the finite rows the 90th percentile of the per-row relative error and the
    relative norm of the difference within the bounds."""
    nan_a, nan_b = np.isnan(a).any(1), np.isnan(b).any(1)
    assert np.array_equal(nan_a, nan_b), "%s: NaN rows %s vs the reference's %s" % (what, np.flatnonzero(nan_a), np.flatnonzero(nan_b))
    assert np.isfinite(a[~nan_a]).all(), what
    keep = ~nan_b if rows is None else (~nan_b & rows)
    a, b = a[keep], b[keep]
    e = _rel_rows(a, b)
    nrm = np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
    p90 = np.percentile(e, 90) if len(e) else 0.0
    nb = np.linalg.norm(b, axis=1)
    print("%-34s rows %3d floored %2d  p90 %.2e  |d|/|g| %.2e  max %.2e  (bounds: p90 < %.0e, |d|/|g| < %.0e)" % (
        what, len(e), int((nb < FLOOR * nb.max()).sum()) if len(nb) else 0, p90, nrm, e.max() if len(e) else 0.0, p90_bound, NORM))
    assert p90 < p90_bound and nrm < NORM, (what, p90, nrm)


@pytest.mark.parametrize("mlp", ["f16x2", "bf16x3", "fp32"])
@pytest.mark.parametrize("tag", CASES)
def test_layered_vjp_of_every_output_vs_reference(tag, mlp, oracle):
    """WideModel.render_rays_vjp(cotangents=..., z_fine=the reference's depths) for each output alone and all together."""
    from neural_sim_nerf_amd.wide import WideModel
    g = load_golden("g28_output_grads")
    sd_c, sd_f, white = case_nets(oracle, g, tag)
    ns, ni, _ = (int(x) for x in g[tag + "_shape"])
    m = WideModel(sd_c, sd_f, n_samples=ns, n_importance=ni, white_bkgd=white, mlp=mlp)
    ro, rd = g[tag + "_rays_o"], g[tag + "_rays_d"]
    ex = _extras(g, tag)
    zf = g[tag + "_z_fine"] if ni > 0 else None
    outs = _outs(g, tag)
    for k in outs + ["all"]:
        cot = {o: g["%s_cot_%s" % (tag, o)] for o in (outs if k == "all" else [k])}
        res = m.render_rays_vjp(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, cotangents=cot, z_fine=zf, extras=ex)
        bound = P90 if k in ("rgb_map", "rgb0") else P90_DISP_ACC
        _check("%s %s %s grad_o" % (tag, mlp, k), cpu(res[0]), g["%s_grad_o_%s" % (tag, k)], p90_bound=bound)
        _check("%s %s %s grad_d" % (tag, mlp, k), cpu(res[1]), g["%s_grad_d_%s" % (tag, k)], p90_bound=bound)
        if ex and "viewdirs" in ex:
            _check("%s %s %s grad_v" % (tag, mlp, k), cpu(res[2]), g["%s_grad_v_%s" % (tag, k)], p90_bound=bound)
    if tag == "e":
        res = m.render_rays_vjp(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, cotangents={"disp_map": g["e_cot_disp_map"]}, z_fine=zf)
        assert np.isfinite(cpu(res[0])).all() and np.isnan(cpu(res[1])).all()
    m.close()


def _dropin(oracle, g, tag, n_importance=128):
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    sd_c, sd_f, white = case_nets(oracle, g, tag)
    nets = []
    for sd in (sd_c, sd_f):
        net = R.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        nets.append(net.to(R.device))
    kw = dict(network_query_fn=None, perturb=False, N_importance=n_importance, network_fine=nets[1] if n_importance else None,
              N_samples=64, network_fn=nets[0], use_viewdirs=True, white_bkgd=white, raw_noise_std=0., ndc=False, lindisp=False,
              near=oracle.YCBV_NEAR, far=oracle.YCBV_FAR)
    return R, nets, kw


@pytest.mark.parametrize("tag", ["a", "b"])
def test_dropin_autograd_of_every_output(tag, oracle):
    """render(rays=...) + torch.autograd.grad over all six outputs on fused-routed networks: the layered twin's own call bit for
    bit, the reference within the bounds on the rays whose depths both sides resampled identically, the route _vjp_route names."""
    import torch
    g = load_golden("g28_output_grads")
    R, nets, kw = _dropin(oracle, g, tag)
    ro, rd = g[tag + "_rays_o"], g[tag + "_rays_d"]
    rays = torch.from_numpy(np.stack([ro, rd])).to(R.device).requires_grad_(True)
    rgb, disp, acc, ex = R.render(400, 400, oracle.YCBV_K, rays=rays, **kw)
    cots = {k: torch.from_numpy(g["%s_cot_%s" % (tag, k)]).to(R.device) for k in OUTS}
    outs = {"rgb_map": rgb, "disp_map": disp, "acc_map": acc, "rgb0": ex["rgb0"], "disp0": ex["disp0"], "acc0": ex["acc0"]}
    (gr,) = torch.autograd.grad([outs[k] for k in OUTS], rays, grad_outputs=[cots[k] for k in OUTS])
    model = R._model_for(nets[0], nets[1], 128, kw)
    assert not model.mlp.startswith("layered-") and model.last_vjp_route == R._vjp_route(model, OUTS) == "twin"
    twin = R._twin(model)
    go, gd = twin.render_rays_vjp(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, cotangents={k: cots[k] for k in OUTS})
    assert np.array_equal(cpu(gr[0]), cpu(go), equal_nan=True) and np.array_equal(cpu(gr[1]), cpu(gd), equal_nan=True)
    zf = cpu(twin.render_rays(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, debug=True)["z_fine"])
    zr = g[tag + "_z_fine"]
    same = (np.abs(zf - zr) <= 1e-5 * np.abs(zr)).all(1)        # the same bins: depths a few ulp apart at most
    print("%s: %d of %d rays resampled identically" % (tag, same.sum(), len(same)))
    assert same.mean() > 0.5
    _check("dropin %s all grad_o" % tag, cpu(gr[0])[same], g[tag + "_grad_o_all"][same], p90_bound=P90_DROPIN)
    _check("dropin %s all grad_d" % tag, cpu(gr[1])[same], g[tag + "_grad_d_all"][same], p90_bound=P90_DROPIN)


def test_dropin_rgb_only_stays_on_the_fused_kernels(oracle):
    """An rgb-only loss with disp / acc returned but unused: the fused VJP kernels, bit for bit what render_rays_vjp gives."""
    import torch
    g = load_golden("g28_output_grads")
    R, nets, kw = _dropin(oracle, g, "a")
    ro, rd = g["a_rays_o"], g["a_rays_d"]
    rays = torch.from_numpy(np.stack([ro, rd])).to(R.device).requires_grad_(True)
    rgb, disp, acc, ex = R.render(400, 400, oracle.YCBV_K, rays=rays, **kw)
    cot = torch.from_numpy(g["a_cot_rgb_map"]).to(R.device)
    (gr,) = torch.autograd.grad((rgb * cot).sum(), rays)
    model = R._model_for(nets[0], nets[1], 128, kw)
    assert model.last_vjp_route == "fused"
    go, gd = model.render_rays_vjp(torch.from_numpy(ro).to(R.device), torch.from_numpy(rd).to(R.device), oracle.YCBV_NEAR,
                                   oracle.YCBV_FAR, cot)
    assert np.array_equal(cpu(gr[0]), cpu(go)) and np.array_equal(cpu(gr[1]), cpu(gd))


def test_coarse_only_default_route(oracle):
    """N_importance = 0 on the default (fused) route: the render gradient through the twin against case D, and render_path_grad
    returns finite psi-gradients equal to autograd through render(c2w=...) per pose."""
    import torch
    g = load_golden("g28_output_grads")
    R, nets, kw = _dropin(oracle, g, "a", n_importance=0)
    ro, rd = g["d_rays_o"], g["d_rays_d"]
    rays = torch.from_numpy(np.stack([ro, rd])).to(R.device).requires_grad_(True)
    rgb, disp, acc, _ = R.render(400, 400, oracle.YCBV_K, rays=rays, **kw)
    outs = dict(rgb_map=rgb, disp_map=disp, acc_map=acc)
    cots = [torch.from_numpy(g["d_cot_" + k]).to(R.device) for k in outs]
    (gr,) = torch.autograd.grad(list(outs.values()), rays, grad_outputs=cots)
    model = R._model_for(nets[0], None, 0, kw)
    assert not model.mlp.startswith("layered-") and model.last_vjp_route == "twin"
    _check("coarse-only dropin grad_o", cpu(gr[0]), g["d_grad_o_all"], p90_bound=P90_DISP_ACC)
    _check("coarse-only dropin grad_d", cpu(gr[1]), g["d_grad_d_all"], p90_bound=P90_DISP_ACC)
    # render_path_grad on an 8 x 8 view: poses as a function of psi, the detector cotangent in CHW
    K = oracle.scaled_K(50.0)
    psi = torch.tensor([0.2, -0.1, 0.3], dtype=torch.float32, requires_grad=True)
    base = [torch.from_numpy(oracle.pose_spherical(90.0, p, 1.01).astype(np.float32)) for p in (-150.0, 20.0)]
    A = torch.from_numpy(np.random.RandomState(5).standard_normal((2, 12, 3)).astype(np.float32) * 0.01)
    poses = [torch.cat([base[i][:3] + (A[i] @ psi).reshape(3, 4), base[i][3:]], 0) for i in range(2)]
    gE = [{"grad_E": [torch.from_numpy(np.random.RandomState(6 + i).standard_normal((3, 8, 8)).astype(np.float32))]} for i in range(2)]
    kwp = dict(kw)
    rgbs, dpsi = R.render_path_grad(psi, poses, (8, 8, K[0][0]), K, 64, gE, kwp)
    assert len(dpsi) == 2 and all(np.isfinite(d.numpy()).all() for d in dpsi)
    for i in range(2):
        c2w = poses[i][:3, :4]
        rgb, _, _, _ = R.render(8, 8, K, c2w=c2w, **kw)
        (gp,) = torch.autograd.grad(rgb, psi, grad_outputs=gE[i]["grad_E"][0].permute(1, 2, 0).to(rgb.device), retain_graph=True)
        assert np.allclose(dpsi[i].numpy(), gp.cpu().numpy(), rtol=1e-4, atol=1e-6), (dpsi[i], gp)


def test_acc_loss_reaches_c2w(oracle):
    """A loss on acc through render(c2w=c2w.requires_grad_()): a finite gradient of c2w, equal to nsr_pose_grad of the rays'
    gradient."""
    import torch
    g = load_golden("g28_output_grads")
    R, nets, kw = _dropin(oracle, g, "a")
    K = oracle.scaled_K(25.0)
    c2w0 = torch.from_numpy(oracle.pose_spherical(90.0, -150.0, 1.01).astype(np.float32))
    c2w = c2w0.clone().to(R.device).requires_grad_(True)
    _, _, acc, _ = R.render(16, 16, K, c2w=c2w[:3, :4], **kw)
    cot = torch.from_numpy(np.random.RandomState(3).standard_normal((16, 16)).astype(np.float32)).to(R.device)
    (gc,) = torch.autograd.grad(acc, c2w, grad_outputs=cot)
    assert np.isfinite(cpu(gc)).all() and np.abs(cpu(gc)).max() > 0
    model = R._model_for(nets[0], nets[1], 128, kw)
    ro, rd = model.get_rays(16, 16, K, c2w0[:3, :4].to(R.device))
    rays = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)]).requires_grad_(True)
    _, _, acc2, _ = R.render(16, 16, K, rays=rays, **kw)
    (gr,) = torch.autograd.grad(acc2, rays, grad_outputs=cot.reshape(-1))
    gp = model.pose_grad(gr[0].contiguous(), gr[1].contiguous(), 16, 16, K, 256)[0]
    assert np.allclose(cpu(gc)[:3, :4], cpu(gp), rtol=1e-5, atol=1e-7), (cpu(gc), cpu(gp))


def test_f16x2_counts_the_coarse_backward_passes(oracle):
    """f16x2: a call with coarse cotangents runs two more network passes per chunk (the coarse forward again, its backward), both
    in the range safety net's count."""
    from neural_sim_nerf_amd.wide import WideModel
    g = load_golden("g28_output_grads")
    sd_c, sd_f, _ = case_nets(oracle, g, "a")
    m = WideModel(sd_c, sd_f, mlp="f16x2")
    ro, rd = g["a_rays_o"], g["a_rays_d"]
    p0 = m.range_status()["passes"]
    m.render_rays_vjp(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, g["a_cot_rgb_map"])
    p1 = m.range_status()["passes"]
    chunks = m.last_kernel_ms()[1]
    m.render_rays_vjp(ro, rd, oracle.YCBV_NEAR, oracle.YCBV_FAR, cotangents={"rgb_map": g["a_cot_rgb_map"], "rgb0": g["a_cot_rgb0"]})
    p2 = m.range_status()["passes"]
    assert chunks >= 1 and p1 - p0 == 3 * chunks and p2 - p1 == 5 * m.last_kernel_ms()[1], (p0, p1, p2, chunks)
    m.close()


def test_output_grads_debug_bounds_build_is_clean(tmp_path):
    """libnsr_debug.so (every index of nsr_wide.hip checked) runs cases A, D and F through nsrw_render_rays_vjp_cot, all outputs,
    on the three arithmetics: no check trips, and the results equal the release build's."""
    import subprocess
    dbg = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr_debug.so")
    assert os.path.exists(dbg), "libnsr_debug.so not built"
    code = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import nerf_oracle as O
from neural_sim_nerf_amd.wide import WideModel
from test_output_grads_host import case_nets
g = np.load(%r)
out, res = {}, []
for mlp in ("bf16x3", "fp32", "f16x2"):
    for tag in "adf":
        c, f, white = case_nets(O, g, tag)
        ns, ni, _ = (int(x) for x in g[tag + "_shape"])
        m = WideModel(c, f, n_samples=ns, n_importance=ni, white_bkgd=white, mlp=mlp)
        cot = {k: g[tag + "_cot_" + k] for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0") if tag + "_cot_" + k in g.files}
        go, gd = m.render_rays_vjp(g[tag + "_rays_o"], g[tag + "_rays_d"], O.YCBV_NEAR, O.YCBV_FAR, cotangents=cot)
        res += [go.cpu().numpy(), gd.cpu().numpy()]
        out["%%s_%%s" %% (mlp, tag)] = m.debug_bounds_status()
        m.close()
np.savez(sys.argv[1] + "/res.npz", *res)
print(out)
''' % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "g28_output_grads.npz"))
    res = {}
    for name, lib in (("debug", dbg), ("release", os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so"))):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([sys.executable, "-c", code, str(d)], env=dict(os.environ, NSR_LIB_PATH=lib), capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[name] = eval(r.stdout.strip().splitlines()[-1])
    assert len(res["debug"]) == 9 and all(v == (True, 0) for v in res["debug"].values()), res["debug"]
    assert all(v == (False, 0) for v in res["release"].values()), res["release"]
    a, b = np.load(tmp_path / "debug" / "res.npz"), np.load(tmp_path / "release" / "res.npz")
    for k in a.files:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
