"""Autograd oracle of the layered renderer's input-gradient call.  TEST INFRASTRUCTURE ONLY.

A torch restatement of what nsrw_render_rays_vjp / _vjp_cot differentiate -- the encoder (RH:18-48), the network (RH:99-122) and the
compositing (RN:343-387) of both passes at GIVEN depths (the coarse depths are constants of near / far, z_fine is detached: RN:475)
-- written from oracle/nerf_oracle.py and differentiated by torch.autograd instead of by hand.  The dtype is a parameter: float64 is
the oracle, float32 the yardstick (what one more fp32-grade evaluation of the same graph costs: tests/test_grad_oracle_host.py).

Besides the gradients it returns what decides whether a ray's gradient is a fair thing to hold a kernel to:
  * relu_margin [N]: the smallest |pre| / (|x| |w| + |b|) over every relu'd unit (all pts_linears, views_linears.0) of every coarse
    and fine point of the ray -- below vjp_census.MARGIN another fp32-grade forward may see the unit on the other side of its relu;
  * sigma_margin [N]: the smallest |sigma| / max |sigma| over the ray's samples of a pass (of both, the smaller), the density relu of RN:356 being a kink too.

`mutate` evaluates a deliberately WRONG backward (MUTATIONS) with the forward untouched: the host test uses them to prove that the
fixtures exercise each path and that the bound of the GPU test would notice its loss."""
import numpy as np
import torch

import nerf_oracle as O
from vjp_census import MARGIN

OUTS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0")
# name -> the term of the backward that is wrong
MUTATIONS = {
    "no_dists_norm": "the dists * |rays_d| path (RN:361) dropped",
    "no_dir_jacobian": "the Jacobian of d / |d| (RN:97) dropped: dL/d viewdirs reaches rays_d as G / |d|, unprojected",
    "no_skip_grad": "the skip layers' encoding gradient (RH:105-106) dropped",
    "views_relu_all_on": "the relu mask of views_linears.0 taken as all-on",
    "sigma_relu_all_on": "the density relu's mask (RN:356) taken as all-on",
    "white_no_sum": "white_bkgd's -sum(g) term (RN:384-385) dropped",
    "untransposed": "one square pts_linears weight matrix not transposed in the backward",
}


class _Untransposed(torch.autograd.Function):
    """h @ w.T whose backward multiplies by w.T again (right: by w)"""
    @staticmethod
    def forward(ctx, h, w):
        ctx.save_for_backward(w)
        return h @ w.T

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return g @ w.T, None


def _relu_all_on(x):
    """relu(x) forward, identity backward"""
    return torch.relu(x).detach() + x - x.detach()


def _embed(x, n_freqs):
    out = [x]
    for l in range(n_freqs):
        out += [torch.sin(x * 2.0 ** l), torch.cos(x * 2.0 ** l)]
    return torch.cat(out, -1)


def _network(sd, pts, dirs, dtype, mutate):
    """RH:99-122 on points [P,3] and directions [P,3] -> rgb logits [P,3], sigma [P], relu margin [P], the density's own
    |sigma| / (|h| |w| + |b|) [P]"""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)
    D, W, input_ch, input_ch_views, skips, use_viewdirs = O.net_shape(sd)
    margin = torch.full((pts.shape[0],), float("inf"), dtype=torch.float64)
    head = None

    def lin(name, x, relu=False, untransposed=False, row=None):
        nonlocal margin, head
        w, b = t(name + ".weight"), t(name + ".bias")
        pre = (_Untransposed.apply(x, w) if untransposed else x @ w.T) + b
        with torch.no_grad():
            scale = x.norm(dim=1)[:, None] * w.norm(dim=1)[None, :] + b.abs()[None, :]
            if relu:
                margin = torch.minimum(margin, (pre.abs() / scale).min(1).values.double())
            if row is not None:
                head = (pre.abs() / scale)[:, row].double()
        return pre

    square = [i for i in range(1, D) if sd["pts_linears.%d.weight" % i].shape[1] == W]
    e_p = _embed(pts, (input_ch - 3) // 6)
    h = e_p
    for i in range(D):
        h = torch.relu(lin("pts_linears.%d" % i, h, True, mutate == "untransposed" and square[:1] == [i]))
        if i in skips:
            h = torch.cat([e_p.detach() if mutate == "no_skip_grad" else e_p, h], -1)
    if not use_viewdirs:
        out = lin("output_linear", h, row=3)
        return out[:, :3], out[:, 3], margin, head
    e_d = _embed(dirs, (input_ch_views - 3) // 6)
    sigma = lin("alpha_linear", h, row=0)[:, 0]
    av = lin("views_linears.0", torch.cat([lin("feature_linear", h), e_d], -1), True)
    hv = _relu_all_on(av) if mutate == "views_relu_all_on" else torch.relu(av)
    return lin("rgb_linear", hv), sigma, margin, head


def _composite(rgb_raw, sigma, z, nrm, white_bkgd, mutate):
    """RN:343-387: rgb logits [N,S,3], sigma [N,S], z [N,S], |rays_d| [N] -> rgb_map, disp_map, acc_map"""
    N = z.shape[0]
    if mutate == "no_dists_norm":
        nrm = nrm.detach()
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), 1e10, dtype=z.dtype)], -1) * nrm[:, None]
    rgb = torch.sigmoid(rgb_raw)
    sig = _relu_all_on(sigma) if mutate == "sigma_relu_all_on" else torch.relu(sigma)
    alpha = 1.0 - torch.exp(-sig * dists)
    T = torch.cumprod(torch.cat([torch.ones((N, 1), dtype=z.dtype), 1.0 - alpha + 1e-10], -1), -1)[:, :-1]
    weights = alpha * T
    rgb_map = (weights[..., None] * rgb).sum(-2)
    depth = (weights * z).sum(-1)
    acc = weights.sum(-1)
    disp = 1.0 / torch.max(1e-10 * torch.ones_like(depth), depth / acc)
    if white_bkgd:
        rgb_map = rgb_map + (1.0 - (acc.detach() if mutate == "white_no_sum" else acc))[:, None]
    return rgb_map, disp, acc, weights


def coarse_depths(n_rays, near, far, n_samples, lindisp=False):
    """the constants of RN:439-443 as the kernels take them: fp32, from the host's linspace table"""
    return O.coarse_z(np.full(n_rays, near, np.float32), np.full(n_rays, far, np.float32), n=n_samples, lindisp=lindisp)


def render_rays_grad(sd_coarse, sd_fine, rays_o, rays_d, z_coarse, z_fine, cotangents, viewdirs=None, white_bkgd=False,
                     dtype=torch.float64, mutate=None):
    """d(sum_k <cotangents[k], output k>) / d(rays_o, rays_d[, viewdirs]) by autograd in `dtype`.
    sd_coarse / sd_fine: state dicts of any net_shape (with `output_linear`: the network without view directions); z_coarse [N,S]
    (coarse_depths: `lindisp` lives there) and z_fine [N,S+I], both constants; z_fine None: a coarse-only handle, whose rgb_map /
    disp_map / acc_map are the coarse pass's.  viewdirs [N,3]: view directions that are an input of their own -- grad_d then holds
    no direction term and grad_viewdirs is returned.  cotangents: {name in OUTS: [N,3] or [N]}.
    Returns dict(grad_o, grad_d [N,3] float64 numpy, grad_viewdirs or None -- none of them without cotangents --, the outputs (OUTS
    the handle has), the compositing weights (weights0 [N,S], weights [N,S+I]; a coarse-only handle: weights), relu_margin [N],
    sigma_margin [N])."""
    assert mutate is None or mutate in MUTATIONS, mutate
    tt = lambda a: torch.tensor(np.asarray(a, np.float32)).to(dtype)
    o, d = tt(rays_o).requires_grad_(True), tt(rays_d).requires_grad_(True)
    N = o.shape[0]
    nrm = d.norm(dim=1)
    if viewdirs is None:
        v_in = None
        v = d / (nrm.detach() if mutate == "no_dir_jacobian" else nrm)[:, None]
    else:
        v = v_in = tt(viewdirs).requires_grad_(True)
    passes = [("0" if z_fine is not None else "_map", sd_coarse, tt(z_coarse))]
    if z_fine is not None:
        passes.append(("_map", sd_fine if sd_fine is not None else sd_coarse, tt(z_fine)))
    outs, taps = {}, {}
    relu_margin = torch.full((N,), float("inf"), dtype=torch.float64)
    sigma_margin = torch.full((N,), float("inf"), dtype=torch.float64)
    density_margin = torch.full((N,), float("inf"), dtype=torch.float64)
    for suffix, sd, z in passes:
        S = z.shape[1]
        pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
        dirs = v[:, None, :].expand(N, S, 3).reshape(-1, 3)
        rgb_raw, sigma, margin, head = _network(sd, pts, dirs, dtype, mutate)
        sigma = sigma.reshape(N, S)
        head = torch.where(sigma.detach() > 0, head.reshape(N, S), torch.full((N, S), float("inf"), dtype=torch.float64))
        density_margin = torch.minimum(density_margin, head.min(1).values)
        relu_margin = torch.minimum(relu_margin, margin.reshape(N, S).min(1).values)
        with torch.no_grad():
            s = sigma.abs().double()
            sigma_margin = torch.minimum(sigma_margin, (s / s.max(1, keepdim=True).values).min(1).values)
        rgb_map, disp, acc, weights = _composite(rgb_raw.reshape(N, S, 3), sigma, z, nrm, white_bkgd, mutate)
        outs.update({"rgb" + suffix: rgb_map, "disp" + suffix: disp, "acc" + suffix: acc})
        taps["weights" + suffix.replace("_map", "")] = weights.detach().double().numpy()
    unknown = set(cotangents) - set(outs)
    assert not unknown, "cotangents of outputs this handle does not have: %s" % sorted(unknown)
    res = dict(relu_margin=relu_margin.numpy(), sigma_margin=sigma_margin.numpy(),
               density_margin=density_margin.numpy(), **taps)
    if cotangents:
        loss = sum((outs[k] * tt(c)).sum() for k, c in cotangents.items())
        wrt = [o, d] + ([v_in] if v_in is not None else [])
        grads = torch.autograd.grad(loss, wrt, allow_unused=True)
        g = [np.zeros((N, 3)) if x is None else x.detach().double().numpy() for x in grads]
        res.update(grad_o=g[0], grad_d=g[1], grad_viewdirs=g[2] if v_in is not None else None)
    res.update({k: x.detach().double().numpy() for k, x in outs.items()})
    return res


def stacked(res):
    """[grad_o | grad_d | grad_viewdirs] rows of a result (or of a kernel's tuple of tensors / arrays)"""
    if isinstance(res, dict):
        parts = [res["grad_o"], res["grad_d"]] + ([res["grad_viewdirs"]] if res.get("grad_viewdirs") is not None else [])
    else:
        parts = [x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x) for x in res]
    return np.concatenate([np.asarray(p, np.float64) for p in parts], 1)
