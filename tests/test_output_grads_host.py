"""CPU checks of the all-outputs gradient (tests/golden/g28_output_grads.npz, tools/gen_golden_outgrad.py): the fixture's forward
outputs against the oracle's numpy restatement at the reference's own depths, and the routing of a backward of render()
(run_nerf_noscale._vjp_route) between the fused VJP kernels, the layered twin of a fused handle and a layered handle."""
import types

import numpy as np
import pytest

from conftest import assert_close, load_golden, trained_pair


def case_nets(O, g, tag):
    """(coarse, fine or None, white_bkgd) state dicts of a g28 case, made the way tools/gen_golden_outgrad.py makes them."""
    sd_c = O.synth_weights(7)
    sd_f = O.synth_weights(7 + 1000, fine_of=sd_c)
    if tag == "b":
        sd_c, sd_f = trained_pair(load_golden("g26_trained"))
    elif tag == "e":
        bias = np.array([g["e_bias"]], np.float32)
        sd_c, sd_f = dict(sd_c, **{"alpha_linear.bias": bias}), dict(sd_f, **{"alpha_linear.bias": bias})
    elif tag == "f":          # g25's "b": 6 x 300, skips after layers 1 and 3, multires 6 / 2
        sd_c = O.synth_weights_shape(48, 6, 300, 6, 2, [1, 3], True)
        sd_f = {k: (v * (1.0 + 0.05 * np.random.RandomState(49).standard_normal(v.shape))).astype(np.float32) for k, v in sd_c.items()}
    ns, ni, white = (int(x) for x in g[tag + "_shape"])
    return sd_c, (sd_f if ni > 0 else None), bool(white)


CASES = "abcdefg"


@pytest.mark.parametrize("tag", CASES)
def test_fixture_forward_matches_the_oracle(tag, oracle):
    """The last pass's rgb / disp / acc of the reference (g28) = the oracle's network + raw2outputs at the reference's sorted depths
    (and its recorded density noise in G): the fixture is the function the GPU tests differentiate."""
    g = load_golden("g28_output_grads")
    sd_c, sd_f, white = case_nets(oracle, g, tag)
    ro, rd, zf = g[tag + "_rays_o"], g[tag + "_rays_d"], g[tag + "_z_fine"]
    vd = g[tag + "_viewdirs"] if tag + "_viewdirs" in g.files else oracle.normalize_dirs(rd)
    noise = g[tag + ("_noise1" if sd_f is not None else "_noise0")] if tag + "_noise0" in g.files else None
    raw = oracle.run_network(sd_f if sd_f is not None else sd_c, (ro[:, None] + rd[:, None] * zf[..., None]).astype(np.float32), vd)
    rgb, disp, acc, _, _ = oracle.raw2outputs(raw, zf, rd, white_bkgd=white, noise=noise)
    assert_close(rgb, g[tag + "_fwd_rgb_map"], atol=3e-6, what="rgb")
    assert_close(acc, g[tag + "_fwd_acc_map"], atol=3e-6, what="acc")
    assert np.array_equal(np.isnan(disp), np.isnan(g[tag + "_fwd_disp_map"]))
    assert_close(disp, g[tag + "_fwd_disp_map"], rtol=1e-4, atol=1e-6, what="disp")
    if tag == "e":            # the NaN case: nothing is opaque, disp = 0 / 0 (RN:381) on every ray, the gradient of disp NaN in d only
        assert (g["e_fwd_acc_map"] == 0).all() and np.isnan(g["e_fwd_disp_map"]).all()
        assert np.isfinite(g["e_grad_o_disp_map"]).all() and np.isnan(g["e_grad_d_disp_map"]).all()
        assert np.isfinite(g["e_grad_d_rgb_map"]).all() and np.isfinite(g["e_grad_d_acc_map"]).all()


def test_vjp_route():
    """rgb_map alone on a coarse+fine fused handle: the fused VJP kernels; any other cotangent -- or a coarse-only fused handle,
    whose fused VJP kernels do not exist -- the layered twin; a layered handle differentiates everything itself."""
    from neural_sim_nerf_amd.run_nerf_noscale import _vjp_route, DIFFERENTIABLE
    fused = types.SimpleNamespace(mlp="f16x2", n_importance=128)
    coarse_only = types.SimpleNamespace(mlp="bf16x3", n_importance=0)
    layered = types.SimpleNamespace(mlp="layered-f16x2", n_importance=128)
    assert _vjp_route(fused, ["rgb_map"]) == "fused"
    assert _vjp_route(fused, {"rgb_map": 1}) == "fused"
    for k in DIFFERENTIABLE[1:]:
        assert _vjp_route(fused, [k]) == "twin"
        assert _vjp_route(fused, ["rgb_map", k]) == "twin"
        assert _vjp_route(layered, [k]) == "layered"
    assert _vjp_route(fused, DIFFERENTIABLE) == "twin"
    for keys in (["rgb_map"], ["disp_map"], ["rgb_map", "acc_map"]):
        assert _vjp_route(coarse_only, keys) == "twin"
    assert _vjp_route(layered, ["rgb_map"]) == "layered"
    assert _vjp_route(fused, []) is None
    assert set(DIFFERENTIABLE) == {"rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0"}       # not z_std, not raw (RN:475)


def test_cotangent_abi_layout():
    """wide.NsrwCotangents mirrors include/nsr_wide.h (six pointers in render()'s output order) and the symbol is bound."""
    from neural_sim_nerf_amd import wide
    assert [f for f, _ in wide.NsrwCotangents._fields_] == ["d_rgb", "d_disp", "d_acc", "d_rgb0", "d_disp0", "d_acc0"]
    assert [wide.COTANGENTS[k][0] for k in wide.COTANGENTS] == [f for f, _ in wide.NsrwCotangents._fields_]
    assert "nsrw_render_rays_vjp_cot" in wide.SIGNATURES
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nsr_wide.h")).read()
    assert "typedef struct NsrwCotangents" in hdr and "int nsrw_render_rays_vjp_cot(" in hdr
