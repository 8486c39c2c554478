"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol include/nsr.h declares, the packers
agree with the oracle through a lane-level emulation of the kernel's MFMA data flow, the host API rejects
unsupported configurations loudly, PNG side effects, synthetic-input recipes."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_exports_every_declared_symbol():
    from neural_sim_nerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "nsr.h")).read()
    declared = set(re.findall(r"\b(nsr_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"nsr_handle_s"}
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), (declared ^ set(_lib.SIGNATURES))
    lib = _lib.load()                                   # dlopen; binds every symbol or raises
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.nsr_abi_version() == _lib.ABI_VERSION


def test_layered_renderer_abi_is_exported_and_bound():
    """include/nsr_wide.h <-> libnsr.so (and its bounds-checked twin) <-> wide.SIGNATURES; nsrw_network_floats (host arithmetic)
    agrees with the parameter block wide.describe() builds from a state dict, for networks with and without view directions."""
    import ctypes as C
    from neural_sim_nerf_amd import wide
    import nerf_oracle as O
    hdr = open(os.path.join(ROOT, "include", "nsr_wide.h")).read()
    declared = set(re.findall(r"\b(nsrw_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(wide.SIGNATURES), declared ^ set(wide.SIGNATURES)
    lib = wide.load()
    dbg = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr_debug.so")
    if os.path.exists(dbg):
        d = C.CDLL(dbg)
        for name in declared:
            assert hasattr(d, name), name
    for D, W, L, Lv, skips, uv in ((10, 384, 10, 4, [4], True), (6, 300, 6, 2, [1, 3], True), (9, 272, 10, 4, [5], False),
                                   (1, 2, 0, 0, [], True)):
        sd = O.synth_weights_shape(3, D, W, L, Lv, skips, uv)
        net, flat = wide.describe(sd)
        assert (net.D, net.W, net.multires, net.use_viewdirs, list(net.skips[:net.n_skips])) == (D, W, L, int(uv), skips)
        assert lib.nsrw_network_floats(C.byref(net)) == flat.size == sum(v.size for k, v in sd.items()
                                                                           if uv or not k.startswith("views_linears"))
        assert np.array_equal(flat[:W * (3 + 6 * L)].reshape(W, -1), sd["pts_linears.0.weight"])
    bad = wide.NsrwNet(8, 256, 10, 4, 1, 4, 1, (C.c_int32 * 16)(7))           # a skip behind the last layer (RH:109 fails there)
    assert lib.nsrw_network_floats(C.byref(bad)) == 0 and b"skip" in lib.nsrw_last_error()


def test_probe_and_debug_libraries_export_their_headers():
    """include/nsr_probe.h <-> libnsr_probe.so; libnsr_debug.so exports the same ABI as libnsr.so (dlopen only: no
    compute without a GPU)."""
    import ctypes as C
    import torch                                                  # one HIP runtime per process (see _lib.py)
    hip = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)
    csrc = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc")
    hdr = open(os.path.join(ROOT, "include", "nsr_probe.h")).read()
    declared = set(re.findall(r"\b(nsr_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"nsr_probe", "nsr_probe_last_error"}
    for so, names in (("libnsr_probe.so", declared),
                      ("libnsr_debug.so", set(re.findall(r"\b(nsr_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "nsr.h")).read()))
                       - {"nsr_handle_s"})):
        path = os.path.join(csrc, so)
        if not os.path.exists(path):
            pytest.skip("%s not built (python -c 'import __graft_entry__ as g; g.build()')" % so)
        lib = C.CDLL(path)
        for name in names:
            assert hasattr(lib, name), (so, name)


def test_shipped_kernels_target_gfx950_only_and_do_not_spill():
    """The library as built (no compiler run, no GPU): its only offload target is gfx950, and the fused render kernels --
    forward and input-gradient, all three arithmetics, both structures -- keep every value in registers (no VGPR spill, no
    scratch).  The one exception is stated, not hidden: the x32 fp32 input-gradient kernel k_render_vjp (not a default;
    it serves the per-ray extras of fp32 handles) spills 4 registers.  Figures from the code object's metadata
    (tools/kernel_resources.py)."""
    import sys
    lib = os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "libnsr.so")
    if not os.path.exists(lib) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    res, targets = kernel_resources(lib)
    assert targets == ["hipv4-amdgcn-amd-amdhsa--gfx950"], targets
    fused = ["k_render_h2", "k_render_vjp_h2", "k_render_b3", "k_render_vjp_b3", "k_render16p", "k_render16", "k_render",
             "k_render_vjp16p", "k_render_vjp16", "k_run_network",
             "k_render_h2_n64", "k_render_h2_n32", "k_render_vjp_h2_n64", "k_render_vjp_h2_n32",       # N_importance 64 / 32 (r04)
             "k_render_b3_n64", "k_render_b3_n32",     # ... and the bf16x3 kernels their range safety net falls back to (r05)
             "k_render_vjp_b3_n64", "k_render_vjp_b3_n32"]
    for k in fused:
        assert res[k]["vgpr_spill_count"] == 0 and res[k]["private_segment_fixed_size"] == 0, (k, res[k])
    assert res["k_render_vjp"]["vgpr_spill_count"] <= 4 and res["k_render_vjp"]["private_segment_fixed_size"] <= 20, res["k_render_vjp"]
    # the register allocation of the default forward kernel is part of its performance contract (r04: a control-flow change
    # that moved it from 412 to 449 registers cost 16 % on MI355X); a change here wants an A/B on hardware
    assert res["k_render_h2"]["vgpr_count"] + 0 <= 420, res["k_render_h2"]
    # the x32-structured kernels own a whole SIMD's register file (one workgroup per CU); the x16 ones share it two ways
    assert res["k_render_h2"]["vgpr_count"] > 256 and res["k_render16p"]["vgpr_count"] <= 256
    # the layered renderer (csrc/nsr_wide.hip, a translation unit of its own in the same library): nothing spills
    layered = [k for k in res if k.startswith("kw_")]
    assert "kw_composite" in layered and "kw_sort" in layered and "kw_embed" in layered
    for k in layered:
        assert res[k]["vgpr_spill_count"] == 0 and res[k]["private_segment_fixed_size"] == 0, (k, res[k])
    # r06: ONE GEMM body for the three arithmetics (csrc/nsr_wide_gemm.inc) -- r05's separate fp32 kernel kw_gemm<...> is gone; the
    # strict fp32 mode is the same body on fp32 MFMAs with the f16x2 form's LDS footprint
    assert not [k for k in layered if k.startswith("kw_gemm<")]
    f32 = [k for k in layered if k.startswith("kw_gemm_f32<")]
    assert {"kw_gemm_f32<%d, %d, %d>" % (nj, e, wm) for nj, wm in ((4, 4), (3, 4), (2, 4), (4, 2), (2, 2), (1, 2)) for e in (0, 1, 2, 4)} <= set(f32), f32
    for e in (0, 1, 2, 4):
        r = res["kw_gemm_f32<4, %d, 4>" % e]
        assert r["vgpr_count"] <= 256 and r["group_segment_fixed_size"] == 65536, r
    # r06: the bf16x3 GEMM (csrc/nsr_wide_gemm.inc).  Its 256 x 256 tile (512 threads, two waves per SIMD) lives on <= 256 registers
    # and 96 KiB of LDS -- one workgroup per CU; the 128-row form on 72 KiB, two per CU
    b3 = [k for k in layered if k.startswith("kw_gemm_b3<")]
    assert {"kw_gemm_b3<%d, %d, %d>" % (nj, e, wm) for nj, wm in ((4, 4), (3, 4), (2, 4), (4, 2), (2, 2), (1, 2)) for e in (0, 1, 2, 4)} <= set(b3), b3
    for e in (0, 1, 2, 4):
        r = res["kw_gemm_b3<4, %d, 4>" % e]
        assert r["vgpr_count"] <= 256 and r["group_segment_fixed_size"] == 98304, r
        r = res["kw_gemm_b3<4, %d, 2>" % e]
        assert r["vgpr_count"] <= 256 and r["group_segment_fixed_size"] == 73728, r
    # r06: the same kernel body on two fp16 pieces (kw_gemm_h2, the layered default): two thirds of the LDS, the same occupancy
    h2 = [k for k in layered if k.startswith("kw_gemm_h2<")]
    assert {"kw_gemm_h2<%d, %d, %d>" % (nj, e, wm) for nj, wm in ((4, 4), (3, 4), (2, 4), (4, 2), (2, 2), (1, 2)) for e in (0, 1, 2, 4)} <= set(h2), h2
    for e in (0, 1, 2, 4):
        r = res["kw_gemm_h2<4, %d, 4>" % e]
        assert r["vgpr_count"] <= 256 and r["group_segment_fixed_size"] == 65536, r


def test_header_constants_match_packer():
    from neural_sim_nerf_amd import pack
    hdr = open(os.path.join(ROOT, "include", "nsr.h")).read()
    val = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, hdr).group(1))
    assert val("NSR_SLAB_FLOATS") == pack.SLAB_FLOATS
    assert val("NSR_STREAM_SLABS") == pack.STREAM_SLABS
    assert val("NSR_AUX_FLOATS") == pack.AUX_FLOATS
    assert pack.PACKED_FLOATS == pack.STREAM_SLABS * pack.SLAB_FLOATS + pack.AUX_FLOATS


def test_no_gpu_means_loud_failure(synth_nets):
    """The product has no CPU path: without a HIP device the engine refuses to construct."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from neural_sim_nerf_amd import _lib
    from neural_sim_nerf_amd.engine import NsrModel
    with pytest.raises(_lib.NsrError):
        NsrModel(synth_nets[0], synth_nets[1])


def test_packer16_backward_through_kernel_emulation(oracle, synth_nets):
    """The x16 forward stream with relu capture and the x16 transposed stream (pack_network_backward16), one wave of 16
    points emulated lane by lane, against the oracle's network and its input-side VJP."""
    from neural_sim_nerf_amd import pack
    import kernel_emulator as E
    sd = synth_nets[1]
    p16, b16 = pack.pack_network16(sd), pack.pack_network_backward16(sd)
    assert b16.shape == (pack.STREAM_SLABS * pack.SLAB_FLOATS,)
    rng = np.random.RandomState(1)
    pts = rng.uniform(-1.5, 1.5, (16, 3)).astype(np.float32)
    d = rng.standard_normal((16, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    masks = {}
    raw = E.mlp_pass16(p16, pts, d, masks)
    want = oracle.mlp(sd, np.concatenate([oracle.embed(pts, 10), oracle.embed(d, 4)], -1))
    assert np.abs(raw - want).max() < 2e-5
    g = rng.standard_normal((16, 4)).astype(np.float32)
    dp, dv = E.mlp_bwd_pass16(p16, b16, masks, pts, d, g)
    rp, rv = oracle.network_vjp(sd, pts, d, g)
    assert np.abs(dp - rp).max() < 1e-5 * np.abs(rp).max(), np.abs(dp - rp).max() / np.abs(rp).max()
    assert np.abs(dv - rv).max() < 1e-5 * np.abs(rv).max(), np.abs(dv - rv).max() / np.abs(rv).max()


def test_kappa_is_a_permutation():
    from neural_sim_nerf_amd.pack import kappa, eps
    t = np.arange(128)
    k = np.concatenate([kappa(t, 0), kappa(t, 1)])
    assert sorted(k.tolist()) == list(range(256))
    cols = [eps(tt, h, 10) for tt in range(32) for h in (0, 1)]
    assert sorted(c for c in cols if c >= 0) == list(range(63)) and cols.count(-1) == 1
    cols = [eps(tt, h, 4) for tt in range(16) for h in (0, 1)]
    assert sorted(c for c in cols if c >= 0) == list(range(27))


def test_eps16_covers_every_embedding_column_once():
    from neural_sim_nerf_amd.pack import eps16
    for n_freq, regs in ((10, 16), (4, 8)):
        cols = [eps16(t, g, n_freq) for t in range(regs) for g in range(4)]
        used = sorted(c for c in cols if c >= 0)
        assert used == list(range(3 + 6 * n_freq)), (n_freq, used)


def test_packer_through_kernel_emulation(oracle, synth_nets):
    """Lane-level numpy emulation of one wave of the kernel's forward and backward network pass, fed with the
    packed streams, against the oracle: pins pack.py and the kernel's fragment indexing on the CPU."""
    from neural_sim_nerf_amd import pack
    import kernel_emulator as E
    sd = synth_nets[1]
    p, b = pack.pack_network(sd), pack.pack_network_backward(sd)
    assert p.shape == (pack.PACKED_FLOATS,) and p.dtype == np.float32
    rng = np.random.RandomState(0)
    pts = rng.uniform(-1.5, 1.5, (32, 3)).astype(np.float32)
    d = rng.standard_normal((32, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    masks = {}
    raw = E.mlp_pass(p, pts, d, masks)
    want = oracle.mlp(sd, np.concatenate([oracle.embed(pts, 10), oracle.embed(d, 4)], -1))
    assert np.abs(raw - want).max() < 2e-5
    g = rng.standard_normal((32, 4)).astype(np.float32)
    dp, dv = E.mlp_bwd_pass(p, b, masks, pts, d, g)
    rp, rv = oracle.network_vjp(sd, pts, d, g)
    assert np.abs(dp - rp).max() < 1e-5 * np.abs(rp).max()
    assert np.abs(dv - rv).max() < 1e-5 * np.abs(rv).max()


def test_packer_b3_through_kernel_emulation(oracle, synth_nets):
    """The bf16x3 forward pass (csrc/nsr_b3.inc): lane-level emulation of one wave, chunk by chunk in the kernel's
    group / step / round order, fed with pack_network_b3's stream, against the oracle AND against the fp32 emulation:
    pins the packer's chunk tables, the slot <-> k-step map and the six-product scheme on the CPU."""
    from neural_sim_nerf_amd import pack
    import kernel_emulator as E
    sd = synth_nets[1]
    p3 = pack.pack_network_b3(sd)
    assert p3.shape == (pack.PACKED_B3_FLOATS,) and p3.dtype == np.float32
    assert np.array_equal(p3[pack.STREAM_SLABS_B3 * pack.SLAB_FLOATS:], pack.pack_network(sd)[pack.STREAM_SLABS * pack.SLAB_FLOATS:])
    rng = np.random.RandomState(0)
    pts = rng.uniform(-1.5, 1.5, (32, 3)).astype(np.float32)
    d = rng.standard_normal((32, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    masks = {}
    raw3 = E.mlp_pass_b3(p3, pts, d, masks)
    raw32 = E.mlp_pass(pack.pack_network(sd), pts, d)
    want = oracle.mlp(sd, np.concatenate([oracle.embed(pts, 10), oracle.embed(d, 4)], -1))
    assert np.abs(raw3 - want).max() < 2e-5                       # the same bound as the fp32 kernel's emulation
    assert np.abs(raw3 - raw32).max() < 2e-5
    assert np.abs(raw3 - raw32).max() > 0                         # it IS a different arithmetic (not the same code path)
    # backward: the transposed stream (4-block encoding GEMMs ahead of the 8-block ones) against the oracle's VJP
    b3 = pack.pack_network_backward_b3(sd)
    assert b3.shape == (pack.STREAM_SLABS_B3_BWD * pack.SLAB_FLOATS,)
    g = rng.standard_normal((32, 4)).astype(np.float32)
    dp, dv = E.mlp_bwd_pass_b3(p3, b3, masks, pts, d, g)
    rp, rv = oracle.network_vjp(sd, pts, d, g)
    assert np.abs(dp - rp).max() < 1e-5 * np.abs(rp).max()
    assert np.abs(dv - rv).max() < 1e-5 * np.abs(rv).max()


def test_packer_h2_through_kernel_emulation(oracle, synth_nets):
    """The f16x2 forward pass (csrc/nsr_h2.inc): lane-level emulation of one wave, chunk by chunk in the kernel's step
    order, fed with pack_network_h2's stream and scaled aux block, against the oracle and the fp32 emulation: pins the
    chunk order, the slot <-> k-step map, the three-product scheme and the scale bookkeeping (weights x 2^sw, biases x
    2^(sw+ca), lazy multipliers, head weights x 2^-P) on the CPU -- also with non-trivial activation scales."""
    from neural_sim_nerf_amd import pack
    import kernel_emulator as E
    sd = synth_nets[1]
    rng = np.random.RandomState(0)
    pts = rng.uniform(-1.5, 1.5, (32, 3)).astype(np.float32)
    d = rng.standard_normal((32, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    want = oracle.mlp(sd, np.concatenate([oracle.embed(pts, 10), oracle.embed(d, 4)], -1))
    raw32 = E.mlp_pass(pack.pack_network(sd), pts, d)
    for ca in (None, [3, -2, 5, 0, 1, 4, -1, 2, 6, 3]):
        p2 = pack.pack_network_h2(sd, ca)
        assert p2.shape == (pack.PACKED_FLOATS,) and p2.dtype == np.float32
        sw, _ = pack.h2_scales(sd, ca)
        for l, name in enumerate(["pts_linears.%d.weight" % i for i in range(8)] + ["feature_linear.weight", "views_linears.0.weight"]):
            top = np.abs(sd[name]).max() * 2.0 ** sw[l]
            assert 2 ** 14 <= top < 2 ** 15, (name, top)
        masks = {}
        raw2 = E.mlp_pass_h2(p2, pts, d, masks)
        assert np.abs(raw2 - want).max() < 2e-5, (ca, np.abs(raw2 - want).max())     # the fp32 kernel emulation's bound
        assert 0 < np.abs(raw2 - raw32).max() < 2e-5
        m32 = {}
        E.mlp_pass(pack.pack_network(sd), pts, d, m32)
        assert all((masks[k] == m32[k]).mean() > 0.9999 for k in masks)               # same relu patterns (up to rounding at 0)
        if ca is None:
            # backward: the transposed stream (2-block encoding GEMMs ahead of the 8-block ones, per-point normalised
            # gradients) against the oracle's VJP -- with cotangents spread over twelve orders of magnitude
            b2 = pack.pack_network_backward_h2(sd)
            assert b2.shape == (pack.STREAM_SLABS_H2_BWD * pack.SLAB_FLOATS,)
            g = (rng.standard_normal((32, 4)) * np.exp(rng.uniform(-14, 14, (32, 1)))).astype(np.float32)
            g[5] = 0.0
            dp, dv = E.mlp_bwd_pass_h2(p2, b2, masks, pts, d, g)
            rp, rv = oracle.network_vjp(sd, pts, d, g)
            scale = np.abs(g).max(1, keepdims=True) + 1e-30
            assert np.abs(dp - rp).max() / np.abs(rp).max() < 1e-5 and np.abs((dp - rp) / scale).max() < 2e-5 * np.abs(rp / scale).max()
            assert np.abs(dv - rv).max() / np.abs(rv).max() < 1e-5 and np.abs((dv - rv) / scale).max() < 2e-5 * np.abs(rv / scale).max()
            assert (dp[5] == 0).all() and (dv[5] == 0).all()
    # domain: a hidden activation whose scaled value leaves the fp16 range poisons that point, and only that point
    big = {k: v.copy() for k, v in sd.items()}
    big["pts_linears.0.bias"][7] = 7.0e4
    raw = E.mlp_pass_h2(pack.pack_network_h2(big), pts, d)
    assert np.isnan(raw).all()
    big["pts_linears.0.bias"][7] = 6.0e4
    raw = E.mlp_pass_h2(pack.pack_network_h2(big), pts, d)
    want_big = oracle.mlp(big, np.concatenate([oracle.embed(pts, 10), oracle.embed(d, 4)], -1))
    assert np.isfinite(raw).all() and np.abs(raw - want_big).max() < 2e-5 * max(1.0, np.abs(want_big).max())


def test_f16x2_split_is_fp32_grade(oracle, synth_nets):
    """The claim in csrc/nsr_h2.inc: with the weights scaled to the top of the fp16 range, the two-piece split with three
    piece products leaves a chain of 256x256 layers as close to an fp64 evaluation as an fp32 GEMM chain is -- on
    ordinary activations, on tiny ones (1e-2: low pieces in the fp16 subnormal range), on large ones, on a wide dynamic
    range within one vector and on cancelling sums.  Gate: <= 2x the error of numpy's fp32 GEMM chain."""
    from neural_sim_nerf_amd import pack
    rng = np.random.RandomState(3)
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-8, 10, 100000))).astype(np.float32)
    x = x[np.abs(x) < 6e4]
    hi, lo = pack.split_f16x2(x)
    rel = np.abs(hi.astype(np.float64) + lo - x) / np.abs(x)
    assert rel[np.abs(x) >= 0.25].max() <= 2.0 ** -23            # both pieces normal: 22+ significand bits
    assert np.abs(hi.astype(np.float64) + lo - x)[np.abs(x) < 0.25].max() <= 2.0 ** -25    # subnormal low piece: absolute
    sd = synth_nets[1]
    W = [np.asarray(sd["pts_linears.%d.weight" % i], np.float32) for i in range(1, 5)]
    B = [np.asarray(sd["pts_linears.%d.bias" % i], np.float32) for i in range(1, 5)]

    def chain(mm, dt, h0):
        h = h0.astype(dt)
        for w, b in zip(W, B):
            h = np.maximum(mm(w.astype(dt), h) + b.astype(dt)[:, None], 0).astype(dt)
        return h

    def mm_h2(w, h):
        sw = np.float32(2.0 ** pack.h2_weight_scale_log2(w))
        w0, w1 = pack.split_f16x2(w * sw)
        h0_, h1 = pack.split_f16x2(h)
        acc = np.zeros((w.shape[0], h.shape[1]), np.float32)
        for k in range(0, w.shape[1], 16):
            for a, b in ((w1, h0_), (w0, h1), (w0, h0_)):
                acc = (acc + a[:, k:k + 16].astype(np.float64) @ b[k:k + 16].astype(np.float64)).astype(np.float32)
        return (acc / sw).astype(np.float32)
    cases = {"ordinary": np.abs(rng.standard_normal((256, 256))),
             "tiny": np.abs(rng.standard_normal((256, 256))) * 1e-2,
             "large": np.abs(rng.standard_normal((256, 256))) * 300.0,
             "wide range": np.abs(rng.standard_normal((256, 256))) * np.exp(rng.uniform(-9, 6, (256, 256))),
             "near-denormal low pieces": np.abs(rng.standard_normal((256, 256))) * 2.0 ** -10}
    for name, h0 in cases.items():
        h0 = h0.astype(np.float32)
        ref = chain(lambda w, h: w @ h, np.float64, h0)
        e32 = np.abs(chain(lambda w, h: (w @ h).astype(np.float32), np.float32, h0) - ref).max()
        e2 = np.abs(chain(mm_h2, np.float32, h0) - ref).max()
        assert e2 <= 2 * e32 + 1e-9 * np.abs(ref).max(), (name, e2, e32)
    # cancellation: rows whose products cancel to 1e-6 of their magnitude
    w = rng.standard_normal((64, 256)).astype(np.float32)
    h = np.abs(rng.standard_normal((256, 64))).astype(np.float32)
    w[:, 128:] = -w[:, :128] * (1 + 1e-6 * rng.standard_normal((64, 128))).astype(np.float32)
    h[128:] = h[:128]
    ref = w.astype(np.float64) @ h.astype(np.float64)
    e32 = np.abs((w @ h).astype(np.float32) - ref).max()
    assert np.abs(mm_h2(w, h) - ref).max() <= 2 * e32 + 1e-9


def test_bf16x3_chunk_tables_match_the_kernel_source():
    """pack.B3_STEPS8 / B3_STEPS4 (and the emulator's copies) mirror B3Sched<8> / B3Sched<4> in csrc/nsr_b3.inc by hand:
    parse the constexpr tables out of the source and compare, and check the properties the schedule relies on (every
    step 8 MFMAs, four different output blocks per step, every (piece, block) pair exactly once per k16 block)."""
    import re
    from neural_sim_nerf_amd import pack
    import kernel_emulator as E
    src = open(os.path.join(ROOT, "neural_sim_nerf_amd", "csrc", "nsr_b3.inc")).read()

    def table(struct, fn):
        body = src[src.index("template <> struct B3Sched<%d>" % struct):]
        m = re.search(r"static constexpr int %s\(int s, int c\) \{ constexpr int t\[\d\]\[4\] = \{(.*?)\}; return" % fn, body)
        return [[int(x) for x in row.split(",")] for row in re.findall(r"\{([\d, ]+)\}", m.group(1))]
    for nmo, steps, ep, eb in ((8, pack.B3_STEPS8, E.B3_PIECE8, E.B3_BLOCK8), (4, pack.B3_STEPS4, E.B3_PIECE4, E.B3_BLOCK4)):
        piece, block = table(nmo, "piece"), table(nmo, "block")
        assert piece == ep and block == eb
        assert [[(p, b) for p, b in zip(pr, br)] for pr, br in zip(piece, block)] == [list(s) for s in steps]
        seen = set()
        for pr, br in zip(piece, block):
            assert sum(3 - p for p in pr) == 8 and len(set(br)) == 4
            seen |= set(zip(pr, br))
        assert seen == {(p, b) for p in range(3) for b in range(nmo)} and len(piece) * 4 == 3 * nmo
    assert int(re.search(r"kStreamSlabsB3 = (\d+)", src).group(1)) == pack.STREAM_SLABS_B3
    assert int(re.search(r"kStreamSlabsB3Bwd = (\d+)", src).group(1)) == pack.STREAM_SLABS_B3_BWD


def test_bf16x3_split_is_fp32_grade(oracle, synth_nets):
    """The claim in csrc/nsr_b3.inc: the three-piece split is exact, and the six kept piece products leave the whole
    MLP as close to an fp64 evaluation as an fp32 GEMM chain is (2048 points, both networks' layer shapes)."""
    from neural_sim_nerf_amd import pack
    rng = np.random.RandomState(3)
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 20, 100000))).astype(np.float32)
    p0, p1, p2 = pack.split_bf16x3(x)
    assert np.array_equal(p0.astype(np.float64) + p1 + p2, x.astype(np.float64))
    for p in (p0, p1, p2):
        assert not (p.view(np.uint32) & 0xffff).any()             # every piece is a bf16
    import kernel_emulator as E
    t0, t1, t2 = E.split_trunc(x)                                 # the kernel's activation split (truncation)
    assert np.array_equal(t0.astype(np.float64) + t1 + t2, x.astype(np.float64))

    sd = synth_nets[1]
    W = [np.asarray(sd["pts_linears.%d.weight" % i], np.float32) for i in range(1, 5)]
    B = [np.asarray(sd["pts_linears.%d.bias" % i], np.float32) for i in range(1, 5)]
    h0 = np.abs(rng.standard_normal((256, 512))).astype(np.float32)

    def chain(mm, dt):
        h = h0.astype(dt)
        for w, b in zip(W, B):
            h = np.maximum(mm(w.astype(dt), h) + b.astype(dt)[:, None], 0).astype(dt)
        return h

    def mm_b3(w, h):
        ws, hs = pack.split_bf16x3(w), E.split_trunc(h)
        acc = np.zeros((w.shape[0], h.shape[1]), np.float32)
        for k in range(0, w.shape[1], 16):
            for i, j in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):
                acc = (acc + ws[i][:, k:k + 16].astype(np.float64) @ hs[j][k:k + 16].astype(np.float64)).astype(np.float32)
        return acc
    ref = chain(lambda w, h: w @ h, np.float64)
    e32 = np.abs(chain(lambda w, h: (w @ h).astype(np.float32), np.float32) - ref).max()
    e3 = np.abs(chain(mm_b3, np.float32) - ref).max()
    assert e3 < 2 * e32 + 1e-7, (e3, e32)


def test_packer_rejects_other_architectures(synth_nets):
    from neural_sim_nerf_amd.pack import pack_network
    sd = dict(synth_nets[0])
    sd["pts_linears.3.weight"] = np.zeros((128, 256), np.float32)
    with pytest.raises(ValueError, match="pts_linears.3.weight"):
        pack_network(sd)


def test_oracle_vjp_matches_reference_autograd(golden, oracle, synth_nets):
    g = golden("g8_backward")
    n = g["rays"].shape[1]
    z = oracle.coarse_z(np.full(n, oracle.YCBV_NEAR, np.float32), np.full(n, oracle.YCBV_FAR, np.float32))
    zf = np.sort(np.concatenate([z, g["z_samples"]], -1), -1)
    go, gd, rgb = oracle.render_rays_vjp(synth_nets[0], synth_nets[1], g["rays"][0], g["rays"][1],
                                         oracle.YCBV_NEAR, oracle.YCBV_FAR, g["cot"], z_fine=zf)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert rel(go, g["grad_rays"][0]) < 5e-5 and rel(gd, g["grad_rays"][1]) < 5e-5
    assert np.abs(rgb - g["rgb"]).max() < 1e-5


def test_synthetic_recipe_is_the_oracles(oracle):
    from neural_sim_nerf_amd import synthetic as S
    a, b = S.synth_weights(5), oracle.synth_weights(5)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    fa, fb = S.synth_weights(1005, fine_of=a), oracle.synth_weights(1005, fine_of=b)
    assert all(np.array_equal(fa[k], fb[k]) for k in fa)
    assert np.array_equal(S.sweep_poses(3, 1), oracle.sweep_poses(3, 1))
    assert S.FLOP_PER_POINT == 2 * oracle.MACS_PER_POINT == 1186816
    assert (S.YCBV_NEAR, S.YCBV_FAR) == (oracle.YCBV_NEAR, oracle.YCBV_FAR)


def test_png_roundtrip_and_to8b(tmp_path):
    from neural_sim_nerf_amd import png
    from neural_sim_nerf_amd.run_nerf_helpers import to8b
    img = to8b(np.random.RandomState(0).uniform(-0.2, 1.2, (13, 7, 3)).astype(np.float32))
    assert img.dtype == np.uint8 and img.min() == 0 and img.max() == 255
    f = str(tmp_path / "a.png")
    png.imwrite(f, img)
    assert np.array_equal(png.imread(f), img)
    with pytest.raises(TypeError):
        png.imwrite(f, img.astype(np.float32))


def test_api_rejects_unsupported_configurations():
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    K = [[100., 0, 4], [0, 100., 4], [0, 0, 1]]
    base = dict(H=8, W=8, K=K, c2w=np.eye(4, dtype=np.float32)[:3], ndc=False, use_viewdirs=True,
                network_fn=None, N_samples=64, N_importance=128)
    # (ndc, c2w_staticcam, perturb, raw_noise_std, per-ray near / far and use_viewdirs=False NETWORKS are served since
    # round 3: tests/test_gpu_parity.py, g14, g15)
    net = R.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    base["network_fn"] = net
    for bad, pat in ((dict(use_viewdirs=False), "use_viewdirs"), (dict(N_samples=2), "N_samples"),
                     (dict(N_samples=1000), "N_samples"), (dict(N_importance=600), "N_importance")):
        kw = dict(base)
        kw.update(bad)
        with pytest.raises(NotImplementedError, match=pat):
            R.render(**kw)
    # sample counts no fused kernel is built for, and networks that are not an 8 x 256 in disguise, go to the layered renderer
    # (wide.WideModel, include/nsr_wide.h) since r05 instead of being refused -- which renderer takes a call, and why:
    assert R._layered_why(net, net, 64, 128) is None and R._layered_why(net, None, 64, 0) is None
    assert R._layered_why(net, net, 32, 64) is None and R._layered_why(net, net, 32, 64, "fp32") is not None
    assert R._layered_why(net, net, 64, 96) is None and "N_importance" in R._layered_why(net, net, 64, 96, "bf16x3")
    assert "N_samples=32" in R._layered_why(net, net, 32, 128) and "N_importance=100" in R._layered_why(net, net, 64, 100)
    deep = R.NeRF(D=9, W=256, input_ch=63, input_ch_views=27, use_viewdirs=True)
    assert "netdepth" in deep.fused_why_not and "netdepth" in R._layered_why(net, deep, 64, 128)
    with pytest.raises(NotImplementedError, match="layered"):
        deep.native_state_dict()
    # retraw on a fused handle whose fine pass carries duplicated samples (decided on the handle that will run)
    class Fused:
        mlp, ni_kernel = "f16x2", 128
    with pytest.raises(NotImplementedError, match="retraw"):
        R._check_retraw(dict(base, N_importance=16, retraw=True), Fused)
    R._check_retraw(dict(base, N_importance=128, retraw=True), Fused)
    # ... which the drop-in API no longer reaches (r06): a retraw call the fused kernels cannot answer in the reference's shape goes to
    # the layered renderer
    assert "retraw" in R._layered_why(net, net, 64, 16, retraw=True) and R._layered_why(net, net, 64, 16) is None
    assert R._layered_why(net, net, 64, 64, retraw=True) is None and R._layered_why(net, net, 64, 128, retraw=True) is None
    assert "retraw" in R._layered_why(net, net, 64, 64, "bf16x3", retraw=True)
    nv = R.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=0, use_viewdirs=False)
    assert "output_linear.weight" in nv.state_dict() and "alpha_linear.weight" not in nv.state_dict()
    assert set(nv.native_state_dict()) == set(net.state_dict())
    for bad in (dict(D=65), dict(W=5000), dict(input_ch=64), dict(input_ch=3 + 6 * 16), dict(input_ch_views=4)):
        with pytest.raises(NotImplementedError, match="neither"):
            R.NeRF(**dict(dict(D=8, W=256, input_ch=63, input_ch_views=27, use_viewdirs=True), **bad))
    small = R.NeRF(D=4, W=128, input_ch=39, input_ch_views=15, use_viewdirs=True)       # fits: served as an 8 x 256 network
    assert {k: tuple(v.shape) for k, v in small.native_state_dict().items()} == {k: tuple(v.shape) for k, v in net.state_dict().items()}
    with pytest.raises(NotImplementedError):
        R.get_embedder(10, 1)
    assert R.get_embedder(10, 0)[1] == 63 and R.get_embedder(4, 0)[1] == 27
    # i_embed = -1 (RH:52-53): no encoding -- (Identity, 3), and a NeRF on 3 + 3 raw channels is the L = 0 case of the mapping
    ident, ch = R.get_embedder(10, -1)
    assert ch == 3 and torch.equal(ident(torch.arange(6.).reshape(2, 3)), torch.arange(6.).reshape(2, 3))
    raw_in = R.NeRF(D=8, W=256, input_ch=3, output_ch=5, skips=[4], input_ch_views=3, use_viewdirs=True)
    assert {k: tuple(v.shape) for k, v in raw_in.native_state_dict().items()} == {k: tuple(v.shape) for k, v in net.state_dict().items()}


def test_random_draws_follow_the_references_order():
    """run_nerf_noscale._draws: what is drawn for which option, in the order the reference draws inside one chunk
    (t_rand RN:451, coarse noise RN:368, u RH:211, fine noise) -- and nothing for the deterministic path."""
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    cpu = torch.device("cpu")
    assert R._draws(dict(perturb=False, raw_noise_std=0.), 5, 128, cpu) == {}
    assert not R._stochastic(dict(perturb=0., raw_noise_std=0.)) and R._stochastic(dict(perturb=1.)) and R._stochastic(dict(raw_noise_std=.1))
    d = R._draws(dict(perturb=1.0, raw_noise_std=2.0), 5, 128, cpu)
    assert list(d) == ["t_rand", "noise0", "u", "noise1"]
    assert [tuple(v.shape) for v in d.values()] == [(5, 64), (5, 64), (5, 128), (5, 192)]
    assert 0 <= float(d["t_rand"].min()) and float(d["t_rand"].max()) < 1 and 0 <= float(d["u"].min()) and float(d["u"].max()) < 1
    assert list(R._draws(dict(perturb=1.0), 3, 0, cpu)) == ["t_rand"]                      # coarse only: no resampling
    assert list(R._draws(dict(raw_noise_std=0.5), 3, 128, cpu)) == ["noise0", "noise1"]   # det resampling stays (RN:474)
    torch.manual_seed(4)
    a = R._draws(dict(perturb=1.0, raw_noise_std=2.0), 7, 128, cpu)
    torch.manual_seed(4)
    t = torch.rand(7, 64); n0 = torch.randn(7, 64) * 2.0; u = torch.rand(7, 128); n1 = torch.randn(7, 192) * 2.0
    assert all(torch.equal(x, y) for x, y in zip(a.values(), (t, n0, u, n1)))
    # more rays than `chunk`: the reference draws inside render_rays, once per chunk (batchify_rays RN:43-55) -- the same
    # calls, chunk by chunk (7 rays, chunk 3 -> 3 + 3 + 1), so a seeded generator gives every ray the reference's numbers
    torch.manual_seed(9)
    a = R._draws(dict(perturb=1.0, raw_noise_std=2.0), 7, 128, cpu, chunk=3)
    torch.manual_seed(9)
    want = {k: [] for k in ("t_rand", "noise0", "u", "noise1")}
    for m in (3, 3, 1):
        want["t_rand"].append(torch.rand(m, 64)); want["noise0"].append(torch.randn(m, 64) * 2.0)
        want["u"].append(torch.rand(m, 128)); want["noise1"].append(torch.randn(m, 192) * 2.0)
    assert list(a) == list(want) and all(torch.equal(a[k], torch.cat(want[k])) for k in want)


def test_pytest_hook_draws_are_the_references(oracle, synth_nets):
    """pytest=True (RN:454-457, RH:214-222): numpy's global generator reseeded with 0 at every draw site and once per chunk
    of rays; the deterministic resampling takes NUMPY's linspace.  run_nerf_noscale._draws against what the reference's
    sample_pdf saw (g18: 80 rays in chunks of 32), and the oracle's render with these draws against the reference's."""
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_pytest_hook.npz"))
    cpu = torch.device("cpu")
    chunk = int(g["chunk"])
    p = R._draws(dict(perturb=1.0, pytest=True), 80, 128, cpu, chunk)
    d = R._draws(dict(perturb=0.0, pytest=True), 80, 128, cpu, chunk)
    assert list(p) == ["t_rand", "u"] and list(d) == ["u"]
    assert np.array_equal(p["u"].numpy(), g["p_u"]) and np.array_equal(d["u"].numpy(), g["d_u"])
    assert np.array_equal(p["u"].numpy()[:32], p["u"].numpy()[32:64]) and np.array_equal(p["u"].numpy()[:16], p["u"].numpy()[64:])
    assert not np.array_equal(d["u"].numpy()[0], oracle.torch_linspace01(128))            # numpy's linspace, not torch's
    assert R._stochastic(dict(pytest=True))
    with pytest.raises(NotImplementedError, match="reference itself fails"):
        R._draws(dict(raw_noise_std=1.0, pytest=True), 8, 128, cpu, 8)
    sd_c, sd_f = synth_nets
    vd = oracle.normalize_dirs(g["rays_d"])
    for tag, dr in (("p", p), ("d", d)):
        rnd = {k: v.numpy() for k, v in dr.items()}
        r = oracle.render_rays(sd_c, sd_f, g["rays_o"], g["rays_d"], vd, oracle.YCBV_NEAR, oracle.YCBV_FAR, extras=True, **rnd)
        assert np.abs(r["rgb0"] - g[tag + "_rgb0"]).max() < 1e-5
        dd = np.abs(r["rgb_map"] - g[tag + "_rgb"]).max(-1)
        assert (dd > 1e-4).mean() <= 0.08 and dd.mean() < 2e-4, (tag, (dd > 1e-4).mean())
        assert (np.abs(r["z_samples"] - g[tag + "_z_samples"]) > 1e-4).mean() < 0.03


def test_nerf_module_has_reference_parameter_names(synth_nets):
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    n = R.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
    assert set(n.state_dict()) == set(synth_nets[0])
    n.load_state_dict({k: torch.from_numpy(v) for k, v in synth_nets[0].items()})
    v0 = n.weights_version()
    with torch.no_grad():
        n.rgb_linear.bias.add_(1.0)
    assert n.weights_version() != v0                     # in-place edits re-trigger packing
    v1 = n.weights_version()
    n.pts_linears[3].weight.data[17, 5] += 0.25          # through .data: neither data_ptr nor _version changes ...
    assert n.weights_version()[0] == v1[0]
    assert n.weights_version() != v1                     # ... the content fingerprint does
    n.invalidate()                                       # explicit hook: no native handle yet, must be a no-op


def test_dropin_import_shadows_only_the_render_modules(tmp_path):
    """`from utils.run_nerf_noscale import *` as neural_sim_main.py:35 does, with the drop-in directory ahead of
    the reference's optimization/ on sys.path: render symbols come from this package, pose sampling
    (utils.load_LINEMOD_noscale, NM:36) still comes from the reference.  The reference's side is a stand-in with its
    layout: `utils` a namespace package (no __init__.py) holding run_nerf_noscale / run_nerf_helpers (which fail if they
    are ever imported), gumble and load_LINEMOD_noscale (which star-imports utils.gumble and imports imageio / cv2)."""
    import subprocess
    import sys
    ref = tmp_path / "optimization"
    (ref / "utils").mkdir(parents=True)
    for name in ("run_nerf_noscale", "run_nerf_helpers"):
        (ref / "utils" / (name + ".py")).write_text("raise ImportError('the reference\\'s utils.%s was imported')\n" % name)
    (ref / "utils" / "gumble.py").write_text("def gumbel_softmax(logits, tau):\n    return logits\n")
    (ref / "utils" / "load_LINEMOD_noscale.py").write_text(
        "import imageio\nimport cv2\nfrom utils.gumble import *\n\n\ndef sample_pose_nograd(prob, n, std):\n    return None\n")
    code = r'''
import sys, types
for m in ("imageio", "cv2"):
    sys.modules[m] = types.ModuleType(m)
sys.path[:0] = [%r, %r, %r]
ns = {}
exec("from utils.run_nerf_noscale import *\nfrom utils.load_LINEMOD_noscale import *", ns)
assert ns["render_path"].__module__ == "neural_sim_nerf_amd.run_nerf_noscale", ns["render_path"].__module__
assert ns["create_nerf"].__module__ == "neural_sim_nerf_amd.run_nerf_noscale"
for name in ("render", "render_path_grad", "to8b", "device"):
    assert name in ns, name
assert ns["sample_pose_nograd"].__module__ == "utils.load_LINEMOD_noscale"
assert ns["gumbel_softmax"].__module__ == "utils.gumble"
import utils.load_LINEMOD_noscale as LL
import utils.run_nerf_helpers as RH
assert LL.__file__.startswith(%r)
assert RH.__file__.startswith(%r)
print("ok")
''' % (ROOT, os.path.join(ROOT, "neural_sim_nerf_amd", "dropin"), str(ref), str(ref), os.path.join(ROOT, "neural_sim_nerf_amd", "dropin"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_pose_module_matches_reference(golden):
    """psi -> poses (LL:202-301) against what the reference produced for the same noise: exact."""
    import torch
    from neural_sim_nerf_amd import pose as P
    g = golden("g10_path_grad")
    poses, log = P.sample_pose_nograd(g["prob16"], 2, 0.1, seed=5)          # the reference seeded numpy with 5
    assert np.array_equal(poses.numpy(), g["poses_nograd"])
    assert np.allclose(log["gumbel_noises"], g["gumbel"]) and np.allclose(log["thetas"], g["thetas"])
    prob = torch.softmax(torch.tensor(g["psi"]) / 0.25, 0).requires_grad_()
    pg = P.sample_pose(prob, 2, 0.1, log)
    assert np.array_equal(pg.detach().numpy(), g["poses_grad"])
    assert np.abs(g["poses_grad"] - g["poses_nograd"]).max() < 1e-5          # fp64-trig vs fp32-trig construction
    (gr,) = torch.autograd.grad(pg.sum(), prob)
    assert gr.shape == (8,) and torch.isfinite(gr).all()


def test_load_data_param(oracle):
    """LL:166-199 on the reference's own nerf_traindata_info.json (committed as a data fixture)."""
    from neural_sim_nerf_amd.data import load_data_param
    d = os.path.join(ROOT, "tests", "golden")
    hwf, K, near, far = load_data_param(d, half_res=False)
    assert hwf == [400, 400, 1333.3333740234375] and K == oracle.YCBV_K
    assert (near, far) == (oracle.YCBV_NEAR, oracle.YCBV_FAR)
    hwf, K, near, far = load_data_param(d, half_res=True)                   # the config default (CF:24)
    assert hwf == [100, 100, 1333.3333740234375 / 4] and K[:2] == oracle.scaled_K(4.0)[:2] and K[2] == [0.0, 0.0, 1.0]


def _args(tmp_path, ckpt):
    import argparse
    return argparse.Namespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=128,
                              netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, netchunk=65536,
                              lrate=5e-4, basedir=str(tmp_path), expname="exp", ft_path=ckpt, no_reload=False,
                              perturb=1.0, N_samples=64, white_bkgd=False, raw_noise_std=0.0,
                              dataset_type="LINEMOD", no_ndc=False, lindisp=False)


def test_create_nerf_loads_reference_checkpoints(tmp_path, synth_nets):
    """RN:258-340: a checkpoint with the reference's keys (RN:296-314) loads; the returned dicts carry the
    reference's keys and the test kwargs are deterministic (perturb False, raw_noise_std 0)."""
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    mk = lambda sd: {k: torch.from_numpy(v) for k, v in sd.items()}
    nets = [R.NeRF(D=8, W=256, input_ch=63, output_ch=5, skips=[4], input_ch_views=27, use_viewdirs=True)
            for _ in range(2)]
    opt = torch.optim.Adam([p for n in nets for p in n.parameters()], lr=5e-4, betas=(0.9, 0.999))
    ckpt = str(tmp_path / "ycbvid2.tar")
    torch.save({"global_step": 1234, "optimizer_state_dict": opt.state_dict(),
                "network_fn_state_dict": mk(synth_nets[0]), "network_fine_state_dict": mk(synth_nets[1])}, ckpt)
    train, test, start, grad_vars, optimizer = R.create_nerf(_args(tmp_path, ckpt))
    assert start == 1234 and len(grad_vars) == 2 * 24
    assert set(train) == {"network_query_fn", "perturb", "N_importance", "network_fine", "N_samples", "network_fn",
                          "use_viewdirs", "white_bkgd", "raw_noise_std", "ndc", "lindisp"}
    assert test["perturb"] is False and test["raw_noise_std"] == 0. and train["perturb"] == 1.0
    for net, sd in zip((test["network_fn"], test["network_fine"]), synth_nets):
        got = net.state_dict()
        assert all(np.array_equal(got[k].cpu().numpy(), sd[k]) for k in sd)


def test_create_nerf_builds_whatever_the_arguments_say(tmp_path, oracle):
    """RN:260-278: netdepth / netwidth / multires / multires_views / use_viewdirs decide the networks.  Shapes that can be
    written as the kernels' 8 x 256 network are built with the reference's parameter names and shapes (so its checkpoints
    load) and re-express themselves for the kernels; the others are refused with the reason."""
    import torch
    import neural_sim_nerf_amd.run_nerf_noscale as R
    a = _args(tmp_path, None)
    a.netdepth, a.netwidth, a.netdepth_fine, a.netwidth_fine, a.multires, a.multires_views = 6, 128, 4, 64, 6, 2
    train, test, start, grad_vars, _ = R.create_nerf(a)
    c, f = test["network_fn"], test["network_fine"]
    assert c.pts_linears[0].weight.shape == (128, 39) and c.views_linears[0].weight.shape == (64, 128 + 15)
    assert f.pts_linears[0].weight.shape == (64, 39) and len(f.pts_linears) == 4 and start == 0
    sd = {k: v.detach().numpy() for k, v in c.state_dict().items()}
    assert oracle.net_shape(sd) == (6, 128, 39, 15, [4], True)
    assert oracle.net_shape({k: v.numpy() for k, v in c.native_state_dict().items()}) == (8, 256, 63, 27, [4], True)
    a.use_viewdirs = False
    _, test, _, _, _ = R.create_nerf(a)
    n = test["network_fn"]
    assert not n.use_viewdirs and n.output_linear.weight.shape == (5, 128) and test["use_viewdirs"] is False
    assert n.views_linears[0].weight.shape == (64, 128) and not hasattr(n, "alpha_linear")            # RH:86, RH:95-96
    a.netwidth = 512                 # wider than the fused kernels: built all the same, served by the layered renderer (r05)
    _, test, _, _, _ = R.create_nerf(a)
    n = test["network_fn"]
    assert n.pts_linears[0].weight.shape == (512, 39) and "netwidth 512" in n.fused_why_not
    assert "netwidth 512" in R._layered_why(n, test["network_fine"], 64, 128)


def test_bench_self_launch_fails_only_on_device_count():
    """`python bench.py --gpus N` outside a launcher re-execs itself under torch.distributed.run; with fewer than N
    devices the ONLY failure is the device count, stated as such (no 'use torchrun' error)."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a node with fewer than 2 devices")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--gpus 2: only %d HIP device(s) visible" % torch.cuda.device_count() in (r.stderr + r.stdout)


def test_adopting_a_module_with_the_references_layout():
    """NeRF.adopt (r06): a module of a FOREIGN class with the reference's attribute and layer names (RH:70-97) is wrapped by a
    drop-in NeRF that holds the same nn.Linear modules -- shared Parameters, so the weight fingerprint and the packer read what
    the caller's optimizer writes; anything else is refused by name."""
    import torch
    import torch.nn as nn
    import neural_sim_nerf_amd.run_nerf_noscale as R

    class Foreign(nn.Module):
        def __init__(self, use_viewdirs):
            super().__init__()
            self.D, self.W, self.input_ch, self.input_ch_views, self.skips, self.use_viewdirs = 3, 40, 15, 9, [1], use_viewdirs
            self.pts_linears = nn.ModuleList([nn.Linear(15, 40), nn.Linear(40, 40), nn.Linear(55, 40)])
            self.views_linears = nn.ModuleList([nn.Linear(49, 20)])
            if use_viewdirs:
                self.feature_linear, self.alpha_linear, self.rgb_linear = nn.Linear(40, 40), nn.Linear(40, 1), nn.Linear(20, 3)
            else:
                self.output_linear = nn.Linear(40, 5)

    for uv in (True, False):
        f = Foreign(uv)
        a = R.NeRF.adopt(f)
        assert isinstance(a, R.NeRF) and a is R.NeRF.adopt(f) and R.NeRF.adopt(a) is a and R.NeRF.adopt(None) is None
        assert (a.D, a.W, a.input_ch, a.input_ch_views, list(a.skips), a.use_viewdirs, a.output_ch) == (3, 40, 15, 9, [1], uv, 4 if uv else 5)
        assert set(a.state_dict()) == set(f.state_dict())
        for k, v in f.state_dict().items():
            assert a.state_dict()[k].data_ptr() == v.data_ptr(), k                 # the SAME storage
        with torch.no_grad():
            f.pts_linears[1].bias.add_(1.0)
        assert torch.equal(a.pts_linears[1].bias, f.pts_linears[1].bias)
        assert "_nsr_adopted" not in dict(f.named_modules()) and len(list(f.parameters())) == len(list(a.parameters()))
    f = Foreign(True)
    a1 = R.NeRF.adopt(f)
    f.rgb_linear = nn.Linear(20, 3)                                                # a layer REPLACED on the foreign module ...
    a2 = R.NeRF.adopt(f)
    assert a2 is not a1 and a2.rgb_linear is f.rgb_linear and a2 is R.NeRF.adopt(f)   # ... is not served from the stale wrapper
    with pytest.raises(NotImplementedError, match="reference's NeRF layout"):
        R.NeRF.adopt(nn.Linear(3, 4))
    bad = Foreign(True)
    bad.alpha_linear = nn.Linear(40, 2)
    with pytest.raises(NotImplementedError, match="alpha_linear"):
        R.NeRF.adopt(bad)

