"""The item pipeline of the x32-structured forward kernels (render32_body): an item's fine composite, output stores and range
report run AFTER the next item's coarse pass, next to that item's coarse chain, and each per-ray chain lives in one wave.

What can go wrong is one item's state being overwritten by, or mixed with, its neighbour's -- which shows at a handful of rays
on one workgroup.  The reference of every test here is the SAME build rendering the same rays one per launch (a one-ray
launch has one item and no partner); the oracle tests of the rest of the suite hold the absolute values.  Everything is
compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 3, 7, 8]          # 3 and 7 end in a one-ray item; 7 on one workgroup: prologue, steady state, epilogue


def cpu(t):
    return t.detach().cpu().numpy()


def _same(a, b, what):
    for k in b:
        x, y = cpu(a[k]), cpu(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert x.tobytes() == y.tobytes(), "%s: %s differs in %d of %d values" % (
            what, k, int((x.view(np.uint8).reshape(x.shape[0], -1) != y.view(np.uint8).reshape(y.shape[0], -1)).any(1).sum()), x.shape[0])


def _cat(outs):
    import torch
    return {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}


@pytest.fixture(scope="module")
def rays(oracle):
    """the 16 rays of a 4x4 view"""
    from neural_sim_nerf_amd import synthetic as S
    c2w = S.sweep_poses(1, seed=3)[0]
    ro, rd = oracle.get_rays(4, 4, S.scaled_K(100.0), c2w[:3, :4])
    return (np.ascontiguousarray(ro.reshape(-1, 3), np.float32), np.ascontiguousarray(rd.reshape(-1, 3), np.float32),
            float(S.YCBV_NEAR), float(S.YCBV_FAR))


def _model(nets, max_workgroups, **kw):
    from neural_sim_nerf_amd.engine import NsrModel
    return NsrModel(nets[0], nets[1], max_workgroups=max_workgroups, **kw)


def _neighbour_invariance(nets, rays, kw, counts=COUNTS, workgroups=(1, 2)):
    ro, rd, near, far = rays
    for wg in workgroups:
        m = _model(nets, wg, **kw)
        single = [m.render_rays(ro[i:i + 1], rd[i:i + 1], near, far, debug=True) for i in range(max(counts))]
        for n in counts:
            got = m.render_rays(ro[:n], rd[:n], near, far, debug=True)
            want = _cat(single[:n])
            assert len(want) >= (5 if kw.get("n_importance", 128) == 0 else 13)      # 3 / 7 outputs and every debug tap
            _same(got, want, "%r, %d workgroup(s), %d rays" % (kw, wg, n))
        m.close()


@pytest.mark.parametrize("kw", [dict(mlp="f16x2"), dict(mlp="bf16x3"), dict(mlp="fp32", variant=32)],
                         ids=["f16x2", "bf16x3", "fp32"])
def test_rays_do_not_depend_on_their_neighbours(synth_nets, rays, kw):
    _neighbour_invariance(synth_nets, rays, kw)


@pytest.mark.parametrize("ns,ni", [(64, 128), (64, 96), (64, 64), (64, 32), (32, 64), (128, 128)])
def test_every_sample_count_form(synth_nets, rays, ns, ni):
    _neighbour_invariance(synth_nets, rays, dict(mlp="f16x2", n_samples=ns, n_importance=ni))


@pytest.mark.parametrize("mlp", ["f16x2", "bf16x3"])
def test_coarse_only_handle(synth_nets, rays, mlp):
    _neighbour_invariance(synth_nets, rays, dict(mlp=mlp, n_importance=0))


@pytest.mark.parametrize("kw", [dict(mlp="f16x2"), dict(mlp="fp32", variant=32)], ids=["f16x2", "fp32"])
def test_per_ray_inputs_follow_their_ray(synth_nets, rays, kw):
    """7 rays on one workgroup with every per-ray input different: jitter, uniforms (sorted for the even rays only, so the odd
    rays' importance samples come out unsorted and take the merge's full rank count -- the path is chosen per ray), both
    noises, per-ray bounds, given view directions; white background."""
    ro, rd, near, far = rays
    n = 7
    rs = np.random.RandomState(11)
    u = rs.uniform(0.0, 1.0, (n, 128)).astype(np.float32)
    u[::2] = np.sort(u[::2], axis=1)
    vd = rs.standard_normal((n, 3)).astype(np.float32)
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    ex = dict(t_rand=rs.uniform(0.0, 1.0, (n, 64)).astype(np.float32), u=u,
              noise0=rs.standard_normal((n, 64)).astype(np.float32), noise1=rs.standard_normal((n, 192)).astype(np.float32),
              near=(near * (1.0 + 0.05 * np.arange(n))).astype(np.float32), far=(far * (1.0 - 0.03 * np.arange(n))).astype(np.float32),
              viewdirs=vd)
    m = _model(synth_nets, 1, white_bkgd=True, **kw)
    got = m.render_rays(ro[:n], rd[:n], near, far, debug=True, extras=ex)
    want = _cat([m.render_rays(ro[i:i + 1], rd[i:i + 1], near, far, debug=True, extras={k: v[i:i + 1] for k, v in ex.items()})
                 for i in range(n)])
    _same(got, want, "extras, %r" % (kw,))
    zf = cpu(got["z_fine"])
    assert (np.diff(zf, axis=1) >= 0).all(), "z_fine is sorted whichever path merged it"
    assert (np.diff(cpu(got["z_samples"])[1::2], axis=1) < 0).any(), "the odd rays' importance samples are unsorted"
    m.close()


def test_range_safety_net_across_the_deferral(oracle, synth_nets, rays):
    """A network of range_stress_workload's kind: the coarse layer-0 bias[7] just under the f16x2 ceiling, here with row 7 of
    that layer's weights scaled by 1024 so that the rays' largest pre-activations of unit 7 lie tens apart.  The oracle's
    encoding (float64 dot product) says which rays exceed 65504 there; the bias is placed in the widest gap that leaves four
    rays on either side, so that four rays end above 65504 and four below the kernels' own ceiling 65504 (1 - 2^-12) = 65488,
    both by at least 8 (fp16 values are 32 apart at the ceiling).  The four items hold in|out, out|out, in|in and out|in.  The report of an
    item is deferred past the next item's coarse pass, which counts into the other copy of the counters."""
    ro, rd, near, far = rays
    edge = [{k: np.array(v, copy=True) for k, v in sd.items()} for sd in synth_nets]
    edge[0]["pts_linears.0.weight"][7] *= np.float32(1024.0)
    z = oracle.coarse_z(np.full(len(ro), near, np.float32), np.full(len(ro), far, np.float32))
    pts = (ro[:, None] + rd[:, None] * z[..., None]).astype(np.float32)
    w7 = edge[0]["pts_linears.0.weight"][7].astype(np.float64)
    pre = oracle.embed(pts.reshape(-1, 3), 10).astype(np.float64)[:, :w7.shape[0]] @ w7
    peak = pre.reshape(len(ro), -1).max(1)                     # per ray: the largest pre-activation of unit 7 without its bias
    order = np.argsort(peak)
    gaps = np.diff(peak[order])
    cut = 3 + int(np.argmax(gaps[3:len(gaps) - 3]))            # order[:cut + 1] stay inside, order[cut + 1:] leave; >= 4 of each
    assert gaps[cut] >= 16.0 + 2 * 8.0, gaps
    bias = np.float32(65496.0 - 0.5 * (peak[order[cut]] + peak[order[cut + 1]]))      # the middle of the gap on 65496
    edge[0]["pts_linears.0.bias"][7] = bias
    inside, outside = order[cut - 3:cut + 1], order[cut + 1:cut + 5]
    act = peak + np.float64(bias)
    assert (act[outside] > 65504.0 + 8.0).all() and (act[inside] < 65488.0 - 8.0).all(), (act[inside], act[outside])
    i_, o_ = inside, outside
    pick = np.array([i_[0], o_[0], o_[1], o_[2], i_[1], i_[2], o_[3], i_[3]])      # items: in|out, out|out, in|in, out|in
    o, d = ro[pick], rd[pick]
    m = _model(edge, 1, mlp="f16x2")
    before = m.range_status()
    single = [m.render_rays(o[i:i + 1], d[i:i + 1], near, far, debug=True) for i in range(8)]
    mid = m.range_status()
    assert mid["rays"] - before["rays"] == 4, "the single launches re-render exactly the rays the oracle names: %r %r" % (before, mid)
    got = m.render_rays(o, d, near, far, debug=True)
    after = m.range_status()
    print("range status: before %r, after 8 single launches %r, after the 8-ray launch %r" % (before, mid, after))
    _same(got, _cat(single), "edge network, 8 rays")
    for k in ("points", "rays"):
        assert after[k] - mid[k] == mid[k] - before[k], (k, before, mid, after)
    assert after["last_items"] == 3 and after["dropped_items"] == 0, after
    # a ray in range keeps its f16x2 bits: alone on a fresh handle each of the four is rendered by the f16x2 kernel only, and
    # every output of the 8-ray launch -- whose fallback launch re-rendered three of the four items -- equals it
    plain = _model(edge, 1, mlp="f16x2")
    for i in (0, 4, 5, 7):
        alone = plain.render_rays(o[i:i + 1], d[i:i + 1], near, far)
        assert len(alone) == 7
        for k, v in alone.items():
            assert cpu(v).tobytes() == cpu(got[k])[i:i + 1].tobytes(), (i, k)
    assert plain.range_status()["rays"] == 0, plain.range_status()
    m.close(); plain.close()


def test_captured_launch_replays(synth_nets, rays):
    """7 rays on one workgroup captured in a graph; the input rays are rewritten and the graph replayed twice"""
    import torch
    ro, rd, near, far = rays
    m = _model(synth_nets, 1, mlp="f16x2")
    sets = [(ro[s:s + 7], rd[s:s + 7]) for s in (0, 4, 9)]
    eager = [{k: cpu(v) for k, v in m.render_rays(a, b, near, far).items()} for a, b in sets]
    o_t = torch.as_tensor(sets[0][0], device=m.device).clone()
    d_t = torch.as_tensor(sets[0][1], device=m.device).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        m.render_rays(o_t, d_t, near, far)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = m.render_rays(o_t, d_t, near, far)
    for i in (1, 2):
        o_t.copy_(torch.as_tensor(sets[i][0])); d_t.copy_(torch.as_tensor(sets[i][1]))
        for v in out.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager[i]:
            assert cpu(out[k]).tobytes() == eager[i][k].tobytes(), (i, k)
    m.close()
