"""WideModel: a handle of the LAYERED renderer in libnsr.so (C ABI: include/nsr_wide.h) -- render_rays (RN:390-501) and its
input-side VJP (RN:168-178) for what the fused kernels are not built for: a NeRF (RH:70-122) of any depth / width / skip
list, any N_samples / N_importance (RN:439, RN:474).  Same interface as engine.NsrModel where the drop-in API
(run_nerf_noscale.py) touches it, so `_model_for` can hand out either.

One MFMA GEMM kernel per layer over a chunk of rays (f16x2, bf16x3 or fp32 MFMAs: `mlp`), activations resident in HBM between the layers; torch owns the
buffers (including the workspace) and the stream, nothing else.  No fallback: without the library or a GPU every call raises."""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

MAX_SKIPS = 16
MAX_SAMPLES = 512


class NsrwConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_samples", C.c_int32), ("n_importance", C.c_int32), ("flags", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class NsrwNet(C.Structure):
    _fields_ = [("D", C.c_int32), ("W", C.c_int32), ("multires", C.c_int32), ("multires_views", C.c_int32),
                ("use_viewdirs", C.c_int32), ("output_ch", C.c_int32), ("n_skips", C.c_int32), ("skips", C.c_int32 * MAX_SKIPS)]


class NsrwExtras(C.Structure):
    _fields_ = [("d_viewdirs", C.c_void_p), ("d_near", C.c_void_p), ("d_far", C.c_void_p), ("d_t_rand", C.c_void_p),
                ("d_u", C.c_void_p), ("d_noise0", C.c_void_p), ("d_noise1", C.c_void_p), ("d_z_fine", C.c_void_p)]


class NsrwOut(C.Structure):
    _fields_ = [("d_rgb", C.c_void_p), ("d_disp", C.c_void_p), ("d_acc", C.c_void_p), ("d_rgb0", C.c_void_p),
                ("d_disp0", C.c_void_p), ("d_acc0", C.c_void_p), ("d_z_std", C.c_void_p), ("d_raw", C.c_void_p),
                ("d_z_vals", C.c_void_p), ("d_weights0", C.c_void_p), ("d_z_samples", C.c_void_p), ("d_inds", C.c_void_p),
                ("d_raw0", C.c_void_p)]


class NsrwCotangents(C.Structure):
    _fields_ = [("d_rgb", C.c_void_p), ("d_disp", C.c_void_p), ("d_acc", C.c_void_p), ("d_rgb0", C.c_void_p),
                ("d_disp0", C.c_void_p), ("d_acc0", C.c_void_p)]


class NsrwGemmPart(C.Structure):
    _fields_ = [("nj", C.c_int32), ("wm", C.c_int32), ("tiles", C.c_int32), ("col_block", C.c_int32)]


class NsrwTrunkPlan(C.Structure):
    _fields_ = [("onchip", C.c_int32), ("nj", C.c_int32), ("tile_rows", C.c_int32), ("lds_bytes", C.c_int32), ("reason", C.c_char * 64)]


class NsrwHeadsPlan(C.Structure):
    _fields_ = [("onchip", C.c_int32), ("lds_bytes", C.c_int32), ("reason", C.c_char * 64)]


class NsrwEmbedPlan(C.Structure):
    _fields_ = [("positions_onchip", C.c_int32), ("directions_onchip", C.c_int32), ("positions_reason", C.c_char * 64),
                ("directions_reason", C.c_char * 64)]


class NsrwStagePlan(C.Structure):
    _fields_ = [("wave", C.c_int), ("rays_per_group", C.c_int), ("lds_bytes", C.c_int), ("reason", C.c_char * 96)]


# render()'s differentiable outputs (RN:488-494) -> the field of NsrwCotangents and the shape of one ray's cotangent
COTANGENTS = {"rgb_map": ("d_rgb", 3), "disp_map": ("d_disp", 1), "acc_map": ("d_acc", 1),
              "rgb0": ("d_rgb0", 3), "disp0": ("d_disp0", 1), "acc0": ("d_acc0", 1)}
COARSE_COTANGENTS = ("rgb0", "disp0", "acc0")


# name -> (restype, argtypes); every symbol include/nsr_wide.h declares
SIGNATURES = {
    "nsrw_last_error": (C.c_char_p, []),
    "nsrw_create": (C.c_int, [C.POINTER(NsrwConfig), C.POINTER(C.c_void_p)]),
    "nsrw_destroy": (C.c_int, [C.c_void_p]),
    "nsrw_upload_network": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(NsrwNet), C.POINTER(C.c_float), C.c_size_t]),
    "nsrw_network_floats": (C.c_size_t, [C.POINTER(NsrwNet)]),
    "nsrw_upload_tables": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float), C.c_int]),
    "nsrw_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_size_t)]),
    "nsrw_render_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.POINTER(NsrwExtras),
                                   C.POINTER(NsrwOut), C.c_void_p, C.c_size_t, C.c_void_p]),
    "nsrw_render_rays_vjp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                       C.POINTER(NsrwExtras), C.c_void_p, C.POINTER(NsrwOut), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "nsrw_render_rays_vjp_cot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                           C.POINTER(NsrwExtras), C.POINTER(NsrwCotangents), C.POINTER(NsrwOut), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "nsrw_run_network": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "nsrw_last_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "nsrw_gemm_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(NsrwGemmPart), C.c_int]),
    "nsrw_flags_refusal": (C.c_char_p, [C.c_int]),
    "nsrw_trunk_plan": (C.c_int, [C.POINTER(NsrwNet), C.c_int, C.POINTER(NsrwTrunkPlan)]),
    "nsrw_heads_plan": (C.c_int, [C.POINTER(NsrwNet), C.c_int, C.POINTER(NsrwHeadsPlan)]),
    "nsrw_trunk_bwd_plan": (C.c_int, [C.POINTER(NsrwNet), C.c_int, C.POINTER(NsrwTrunkPlan)]),
    "nsrw_trunk_keep_plan": (C.c_int, [C.POINTER(NsrwNet), C.c_int, C.POINTER(NsrwTrunkPlan)]),
    "nsrw_keep_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "nsrw_trunk_rerun_plan": (C.c_int, [C.POINTER(NsrwNet), C.c_int, C.POINTER(NsrwTrunkPlan)]),
    "nsrw_rerun_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "nsrw_embed_plan": (C.c_int, [C.POINTER(NsrwNet), C.c_int, C.c_int, C.POINTER(NsrwEmbedPlan)]),
    "nsrw_embed_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "nsrw_stage_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(NsrwStagePlan)]),
    "nsrw_stages_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "nsrw_debug_bounds_status": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_uint)]),
    "nsrw_range_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "nsrw_range_rows_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "nsrw_rerun_rows_list": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "nsrw_rerun_rows_plan": (C.c_int, [C.POINTER(C.c_uint32), C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_int32), C.c_int64]),
    "nsrw_sample_pdf": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "nsrw_embed_vjp": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
}

FLAG_WHITE_BKGD, FLAG_LINDISP, FLAG_MLP_BF16X3, FLAG_MLP_F16X2, FLAG_TRUNK_ONCHIP, FLAG_HEADS_ONCHIP = 1, 2, 4, 8, 16, 32
FLAG_TRUNK_WIDE = 64
FLAG_TRUNK_BWD = 128
FLAG_TRUNK_KEEP = 256
FLAG_STAGES_WAVE = 512
FLAG_TRUNK_RERUN = 1024
FLAG_EMBED_ONCHIP = 1 << 11
FLAG_RERUN_ROWS = 1 << 12
MLPS = ("bf16x3", "fp32", "f16x2")
TRUNKS = ("layers", "onchip")
HEADS = ("layers", "onchip")
TRUNK_BWDS = ("layers", "onchip")
TRUNK_KEEPS = ("layers", "onchip")
TRUNK_RERUNS = ("layers", "onchip")     # the bf16x3 re-run of a pass whose trunk ran on chip: a launch per layer, or one (FLAG_TRUNK_RERUN)
EMBEDS = ("layers", "onchip")           # the encodings of a pass whose f16x2 launch is on chip: the kw_embed launch, or in that launch (FLAG_EMBED_ONCHIP)
RERUNS = ("pass", "rows")               # the unit of an f16x2 handle's bf16x3 re-run: the pass over a chunk, or the point (FLAG_RERUN_ROWS)
STAGES = ("threads", "wave")    # the per-ray stages between the network passes: one thread per ray, or one wave (FLAG_STAGES_WAVE)
STAGE_COMPOSITE, STAGE_SAMPLE_PDF, STAGE_COMPOSITE_BWD = 0, 1, 2
STAGE_IDS = {"composite": STAGE_COMPOSITE, "sample_pdf": STAGE_SAMPLE_PDF, "composite_bwd": STAGE_COMPOSITE_BWD}
TRUNK_WIDTHS = (128, 256)       # the largest padded width trunk="onchip" takes: 256 adds the wide form (FLAG_TRUNK_WIDE)

DEFAULT_MLP = "f16x2"           # r06: the fused default kernel's arithmetic; same parity bounds as the fp32 MFMAs and bf16x3 (tests/test_gpu_wide.py
                                # runs every case on all three), 2.6x / 1.5x their speed; a pass that leaves fp16's range is re-run on
                                # bf16x3, so the bits are chunk-dependent once a pass re-runs, unless rerun="rows" (workspace_cap_env)

_bound = None


def load():
    """The nsrw_* entry points of libnsr.so, bound; raises NsrError when the library is missing or stale."""
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                raise _lib.NsrError("libnsr.so does not export %s -- rebuild it (python -c 'import __graft_entry__ as g; g.build()')"
                                    % name)
            fn.restype, fn.argtypes = res, args
        _bound = lib
    return _bound


def check(rc):
    if rc != 0:
        raise _lib.NsrError(load().nsrw_last_error().decode("utf-8", "replace"))


def gemm_plan(n_packed_rows, n_stored_columns, tile_wm=4):
    """nsrw_gemm_plan (diagnostic; no device, no handle): the launches of one layer GEMM along N, as
    [(NJ, WM of the kernel form, tiles, first column)]; tile_wm = 2 is what NSRW_B3_WM=2 selects."""
    lib = load()
    parts = (NsrwGemmPart * 8)()
    count = lib.nsrw_gemm_plan(int(n_packed_rows), int(n_stored_columns), int(tile_wm), parts, len(parts))
    if not 0 <= count <= len(parts):
        raise _lib.NsrError(lib.nsrw_last_error().decode("utf-8", "replace"))
    return [(p.nj, p.wm, p.tiles, 32 * p.col_block) for p in parts[:count]]


def _mlp_flags(mlp):
    return (FLAG_MLP_BF16X3 if mlp == "bf16x3" else 0) | (FLAG_MLP_F16X2 if mlp == "f16x2" else 0)


# The opt-in knobs of a handle, in the order they are resolved -- a knob may need the ones before it.  name: WideModel's argument and
# attribute; env: where the wish comes from when the argument is not given; values: what it may be, values[0] the default; on: the
# value that asks for something; flag: what `on` sets in NsrwConfig.flags; needs: what `on` takes of mlp and of the knobs before it;
# refusal: NotImplementedError's words for an explicit `on` that cannot be honoured (% the resolved options).  The library states the
# same dependencies for the flags (kFlagNeeds in csrc/nsr_wide.hip); tests/test_wide_options_host.py holds the two to each other.
_Knob = collections.namedtuple("_Knob", "name env values on flag needs refusal")
_ONCHIP = {"mlp": "f16x2", "trunk": "onchip"}
KNOBS = (
    _Knob("trunk", "NSR_WIDE_TRUNK", TRUNKS, "onchip", FLAG_TRUNK_ONCHIP, {"mlp": "f16x2"},
          "trunk=\"onchip\" exists for mlp=\"f16x2\" only (got mlp=%(mlp)r)"),
    _Knob("heads", "NSR_WIDE_HEADS", HEADS, "onchip", FLAG_HEADS_ONCHIP, _ONCHIP,
          "heads=\"onchip\" runs behind the on-chip trunk: it needs mlp=\"f16x2\" and trunk=\"onchip\" (got mlp=%(mlp)r, trunk=%(trunk)r)"),
    _Knob("trunk_width", "NSR_WIDE_TRUNK_WIDTH", TRUNK_WIDTHS, 256, FLAG_TRUNK_WIDE, _ONCHIP,
          "trunk_width=256 widens the on-chip trunk: it needs mlp=\"f16x2\" and trunk=\"onchip\" (got mlp=%(mlp)r, trunk=%(trunk)r)"),
    _Knob("trunk_bwd", "NSR_WIDE_TRUNK_BWD", TRUNK_BWDS, "onchip", FLAG_TRUNK_BWD, _ONCHIP,
          "trunk_bwd=\"onchip\" serves the networks the on-chip trunk serves: it needs mlp=\"f16x2\" and "
          "trunk=\"onchip\" (got mlp=%(mlp)r, trunk=%(trunk)r)"),
    _Knob("trunk_keep", "NSR_WIDE_TRUNK_KEEP", TRUNK_KEEPS, "onchip", FLAG_TRUNK_KEEP, dict(_ONCHIP, trunk_bwd="onchip"),
          "trunk_keep=\"onchip\" leaves the relu masks as bits for the on-chip backward trunk: it needs mlp=\"f16x2\", "
          "trunk=\"onchip\" and trunk_bwd=\"onchip\" (got mlp=%(mlp)r, trunk=%(trunk)r, trunk_bwd=%(trunk_bwd)r)"),
    _Knob("stages", "NSR_WIDE_STAGES", STAGES, "wave", FLAG_STAGES_WAVE, {}, ""),       # any arithmetic, any other knob: never refused
    _Knob("trunk_rerun", "NSR_WIDE_TRUNK_RERUN", TRUNK_RERUNS, "onchip", FLAG_TRUNK_RERUN, _ONCHIP,
          "trunk_rerun=\"onchip\" re-runs a pass of the on-chip trunk: it needs mlp=\"f16x2\" and "
          "trunk=\"onchip\" (got mlp=%(mlp)r, trunk=%(trunk)r)"),
    _Knob("embed", "NSR_WIDE_EMBED", EMBEDS, "onchip", FLAG_EMBED_ONCHIP, _ONCHIP,
          "embed=\"onchip\" computes the encodings in the on-chip trunk's launch: it needs mlp=\"f16x2\" and trunk=\"onchip\" "
          "(got mlp=%(mlp)r, trunk=%(trunk)r)"),
    _Knob("rerun", "NSR_WIDE_RERUN", RERUNS, "rows", FLAG_RERUN_ROWS, {"mlp": "f16x2", "trunk": "layers"},
          "rerun=\"rows\" re-runs the flagged rows of a per-layer f16x2 pass: it needs mlp=\"f16x2\" and "
          "trunk=\"layers\" (got mlp=%(mlp)r, trunk=%(trunk)r)"),
)


def resolve_knobs(mlp, wishes, environ):
    """{knob: value} for a handle of arithmetic `mlp`: the caller's wish (`wishes`: {knob: argument or None}), else the
    environment's, else the default.  A value that is not one of the knob's raises ValueError.  The environment's wish is dropped where
    the handle cannot honour it (the drop-in API also builds bf16x3 / fp32 handles); an explicit one raises NotImplementedError.  Pure:
    no device, no library."""
    got = {"mlp": mlp}
    for k in KNOBS:
        v = wishes.get(k.name)
        number = not isinstance(k.on, str)
        from_env = v is None if number else not v               # (trunk_width=0 is a wish, and a bad one)
        if from_env:
            v = environ.get(k.env) or k.values[0]
            if number and isinstance(v, str) and v.isdigit():
                v = int(v)
        if v not in k.values:
            raise ValueError("%s must be one of %s (got %r)" % (k.name, k.values, v))
        v = k.values[k.values.index(v)]
        can = all(got[n] == need for n, need in k.needs.items())
        if from_env and not can:
            v = k.values[0]
        if v == k.on and not can:
            raise NotImplementedError(k.refusal % got)
        got[k.name] = v
    del got["mlp"]
    return got


def knob_flags(**values):
    """the NsrwConfig.flags of the knobs `values` ({knob: value}; a knob not named is at its default): the flags of the rows whose
    value is `on` (a trunk_width of 256 says nothing without trunk="onchip").  A value that is not one of its knob's raises
    ValueError.  What goes together is resolve_knobs' to say, not this sum's."""
    got = {k.name: values.pop(k.name, k.values[0]) for k in KNOBS}
    if values:
        raise TypeError("knob_flags: no such knob: %s" % ", ".join(sorted(values)))
    for k in KNOBS:
        if got[k.name] not in k.values:
            raise ValueError("%s must be one of %s (got %r)" % (k.name, k.values, got[k.name]))
    if got["trunk"] != "onchip":
        got["trunk_width"] = TRUNK_WIDTHS[0]
    return sum(k.flag for k in KNOBS if got[k.name] == k.on)


def rerun_rows_plan(words, M, tile_rows=256):
    """nsrw_rerun_rows_plan (diagnostic; no device, no handle): the ascending tile blocks of `tile_rows` (128 or 256) rows of an M-row
    pass that hold a flagged row, from the row bits `words` (uint32; bit r % 32 of word r // 32 = row r; rows >= M do not count) -- the
    host restatement of the list kernel of rerun="rows"."""
    lib = load()
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(max(1, (int(M) + int(tile_rows) - 1) // max(int(tile_rows), 1)), dtype=np.int32)
    count = lib.nsrw_rerun_rows_plan(w.ctypes.data_as(C.POINTER(C.c_uint32)), w.size, int(M), int(tile_rows),
                                     out.ctypes.data_as(C.POINTER(C.c_int32)), out.size)
    if count < 0:
        raise _lib.NsrError(lib.nsrw_last_error().decode("utf-8", "replace"))
    return [int(x) for x in out[:count]]


def rerun_rows_list(words, M, tile_rows=256, device=None):
    """nsrw_rerun_rows_list (diagnostic stage entry; no handle): the list kernel of rerun="rows" on the row bits `words` -> (the
    listed blocks in the order the kernel wrote them, rows seen, rows flagged, the range word)."""
    lib = load()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    w = torch.as_tensor(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32), device=dev)
    blocks = (int(M) + int(tile_rows) - 1) // int(tile_rows)
    lst = torch.zeros(1 + max(blocks, 1), dtype=torch.int32, device=dev)
    rng = torch.zeros(8, dtype=torch.int32, device=dev)
    check(lib.nsrw_rerun_rows_list(dev.index, _dev(w), int(M), int(tile_rows), _dev(lst), blocks, _dev(rng), _stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    l, r = lst.cpu().numpy(), rng.cpu().numpy().view(np.uint32)
    counts = r[4:8].view(np.uint64)
    return [int(x) for x in l[1:1 + int(l[0])]], int(counts[0]), int(counts[1]), int(r[0])


def stage_plan(stage, samples, n_importance=0, flags=FLAG_STAGES_WAVE):
    """nsrw_stage_plan (diagnostic; no device, no handle): how a handle created with `flags` runs the per-ray stage `stage`
    (STAGE_COMPOSITE / STAGE_SAMPLE_PDF / STAGE_COMPOSITE_BWD, or its name in STAGE_IDS) of a pass with `samples` samples per ray
    (sample_pdf: N_samples, drawing n_importance) -- dict(mode="wave", rays_per_group, lds_bytes: per ray) for the wave-per-ray
    kernel of csrc/nsr_wide_stages.inc, or dict(mode="threads", reason=...) for the thread-per-ray kernel."""
    lib = load()
    plan = NsrwStagePlan()
    if lib.nsrw_stage_plan(int(STAGE_IDS.get(stage, stage)), int(samples), int(n_importance), int(flags), C.byref(plan)) != 0:
        raise _lib.NsrError(lib.nsrw_last_error().decode("utf-8", "replace"))
    if plan.wave:
        return dict(mode="wave", rays_per_group=int(plan.rays_per_group), lds_bytes=int(plan.lds_bytes))
    return dict(mode="threads", reason=plan.reason.decode("utf-8", "replace"))


def _plan(entry, struct, fields, net_or_sd, flags):
    """one of the library's four plan entries (diagnostic; no device, no handle) on a network -- an NsrwNet or a state dict"""
    lib = load()
    net = net_or_sd if isinstance(net_or_sd, NsrwNet) else describe(net_or_sd)[0]
    plan = struct()
    if getattr(lib, entry)(C.byref(net), flags, C.byref(plan)) != 0:
        raise _lib.NsrError(lib.nsrw_last_error().decode("utf-8", "replace"))
    if plan.onchip:
        return dict(mode="onchip", **{f: int(getattr(plan, f)) for f in fields})
    return dict(mode="layers", reason=plan.reason.decode("utf-8", "replace"))


def trunk_plan(net_or_sd, mlp=DEFAULT_MLP, trunk="onchip", trunk_width=128):
    """nsrw_trunk_plan (diagnostic; no device, no handle): how a handle of arithmetic `mlp` created with trunk=`trunk`,
    trunk_width=`trunk_width` runs the pts_linears of a network (an NsrwNet or a state dict) -- dict(mode="onchip", nj, tile_rows,
    lds_bytes) for the one-launch trunk of csrc/nsr_wide_trunk.inc (tile_rows = 64: its wide form), or dict(mode="layers",
    reason=...) for a GEMM launch per layer."""
    return _plan("nsrw_trunk_plan", NsrwTrunkPlan, ("nj", "tile_rows", "lds_bytes"), net_or_sd,
                 _mlp_flags(mlp) | knob_flags(trunk=trunk, trunk_width=trunk_width))


def heads_plan(net_or_sd, mlp=DEFAULT_MLP, trunk="onchip", heads="onchip", trunk_width=128):
    """nsrw_heads_plan (diagnostic; no device, no handle): how a handle of arithmetic `mlp` created with trunk=`trunk`,
    heads=`heads`, trunk_width=`trunk_width` runs the heads of a network (an NsrwNet or a state dict) behind its pts_linears -- dict(mode="onchip",
    lds_bytes) for the heads form of the one-launch trunk, or dict(mode="layers", reason=...) for a GEMM launch per head."""
    return _plan("nsrw_heads_plan", NsrwHeadsPlan, ("lds_bytes",), net_or_sd,
                 _mlp_flags(mlp) | knob_flags(trunk=trunk, trunk_width=trunk_width, heads=heads))


def trunk_bwd_plan(net_or_sd, mlp=DEFAULT_MLP, trunk="onchip", trunk_bwd="onchip", trunk_width=128):
    """nsrw_trunk_bwd_plan (diagnostic; no device, no handle): how a handle of arithmetic `mlp` created with trunk=`trunk`,
    trunk_bwd=`trunk_bwd`, trunk_width=`trunk_width` runs the input-gradient chain of a network (an NsrwNet or a state dict) in its
    gradient calls -- dict(mode="onchip", nj, tile_rows, lds_bytes) for the one-launch backward trunk of csrc/nsr_wide_trunk.inc, or
    dict(mode="layers", reason=...) for a GEMM launch per product."""
    return _plan("nsrw_trunk_bwd_plan", NsrwTrunkPlan, ("nj", "tile_rows", "lds_bytes"), net_or_sd,
                 _mlp_flags(mlp) | knob_flags(trunk=trunk, trunk_width=trunk_width, trunk_bwd=trunk_bwd))


def trunk_keep_plan(net_or_sd, mlp=DEFAULT_MLP, trunk="onchip", trunk_bwd="onchip", trunk_keep="onchip", heads="layers", trunk_width=128):
    """nsrw_trunk_keep_plan (diagnostic; no device, no handle): how a handle of arithmetic `mlp` created with these knobs runs the
    f16x2 pass of a forward that keeps its activations for a backward, on a network (an NsrwNet or a state dict) --
    dict(mode="onchip", nj, tile_rows, lds_bytes) for the one kept launch of csrc/nsr_wide_trunk.inc (the relu masks as bits, read by
    the bit-reading backward launch), or dict(mode="layers", reason=...) for a GEMM launch per layer with fp32 activations kept."""
    return _plan("nsrw_trunk_keep_plan", NsrwTrunkPlan, ("nj", "tile_rows", "lds_bytes"), net_or_sd,
                 _mlp_flags(mlp) | knob_flags(trunk=trunk, trunk_width=trunk_width, heads=heads, trunk_bwd=trunk_bwd,
                                              trunk_keep=trunk_keep))


def trunk_rerun_plan(net_or_sd, mlp=DEFAULT_MLP, trunk="onchip", trunk_rerun="onchip", trunk_width=128):
    """nsrw_trunk_rerun_plan (diagnostic; no device, no handle): how a handle of arithmetic `mlp` created with trunk=`trunk`,
    trunk_rerun=`trunk_rerun`, trunk_width=`trunk_width` runs the pts_linears of the conditional bf16x3 re-run of a forward pass that
    keeps no activations, on a network (an NsrwNet or a state dict) -- dict(mode="onchip", nj, tile_rows, lds_bytes) for the one
    launch of kw_rerun_b3 (csrc/nsr_wide_trunk.inc; tile_rows = 128 up to a padded width of 64, 64 for 96 and 128), or
    dict(mode="layers", reason=...) for a conditional GEMM launch per layer."""
    return _plan("nsrw_trunk_rerun_plan", NsrwTrunkPlan, ("nj", "tile_rows", "lds_bytes"), net_or_sd,
                 _mlp_flags(mlp) | knob_flags(trunk=trunk, trunk_width=trunk_width, trunk_rerun=trunk_rerun))


def embed_plan(net_or_sd, mlp=DEFAULT_MLP, trunk="onchip", heads="layers", trunk_width=128, trunk_bwd="layers", trunk_keep="layers",
               embed="onchip", kept=False):
    """nsrw_embed_plan (diagnostic; no device, no handle): where a handle of arithmetic `mlp` created with these knobs computes the
    encodings of a pass of a network (an NsrwNet or a state dict) -- kept: a pass that keeps its activations for a backward -- as
    dict(positions=..., directions=...), each dict(mode="onchip") for "in the pass's one f16x2 launch" or dict(mode="layers",
    reason=...) for the kw_embed launch."""
    flags = _mlp_flags(mlp) | knob_flags(trunk=trunk, trunk_width=trunk_width, heads=heads, trunk_bwd=trunk_bwd, trunk_keep=trunk_keep,
                                         embed=embed)
    lib = load()
    net = net_or_sd if isinstance(net_or_sd, NsrwNet) else describe(net_or_sd)[0]
    plan = NsrwEmbedPlan()
    if lib.nsrw_embed_plan(C.byref(net), flags, 1 if kept else 0, C.byref(plan)) != 0:
        raise _lib.NsrError(lib.nsrw_last_error().decode("utf-8", "replace"))
    one = lambda on, why: dict(mode="onchip") if on else dict(mode="layers", reason=why.decode("utf-8", "replace"))
    return dict(positions=one(plan.positions_onchip, plan.positions_reason), directions=one(plan.directions_onchip, plan.directions_reason))


def _np(v):
    return (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float32)


def describe(sd):
    """State dict with the reference's parameter names (RH:82-97) -> (NsrwNet, flat fp32 parameter block in the order
    include/nsr_wide.h: nsrw_upload_network names).  The shape is read off the weights (layer i + 1 takes W + input_ch inputs
    exactly when i is a skip, RH:82-83; `output_linear` present = use_viewdirs=False, RH:95-96)."""
    a = {k: _np(v) for k, v in sd.items()}
    D = 1 + max(int(k.split(".")[1]) for k in a if k.startswith("pts_linears."))
    W, input_ch = a["pts_linears.0.weight"].shape
    skips = [i for i in range(D - 1) if a["pts_linears.%d.weight" % (i + 1)].shape[1] == W + input_ch]
    use_viewdirs = "output_linear.weight" not in a
    if (input_ch - 3) % 6:
        raise NotImplementedError("input_ch %r is not 3 + 6 L (get_embedder RH:51-66)" % (input_ch,))
    in_v = a["views_linears.0.weight"].shape[1] - W if "views_linears.0.weight" in a else 3
    if use_viewdirs and (in_v < 3 or (in_v - 3) % 6):
        raise NotImplementedError("input_ch_views %r is not 3 + 6 L" % (in_v,))
    if len(skips) > MAX_SKIPS:
        raise NotImplementedError("%d skips (at most %d)" % (len(skips), MAX_SKIPS))
    net = NsrwNet(D, W, (input_ch - 3) // 6, (in_v - 3) // 6 if use_viewdirs else 0, 1 if use_viewdirs else 0,
                  4 if use_viewdirs else int(a["output_linear.weight"].shape[0]), len(skips),
                  (C.c_int32 * MAX_SKIPS)(*(skips + [0] * (MAX_SKIPS - len(skips)))))
    names = ["pts_linears.%d" % i for i in range(D)]
    names += ["feature_linear", "alpha_linear", "views_linears.0", "rgb_linear"] if use_viewdirs else ["output_linear"]
    flat = np.concatenate([np.concatenate([a[n + ".weight"].ravel(), a[n + ".bias"].ravel()]) for n in names]).astype(np.float32)
    return net, np.ascontiguousarray(flat)


def _dev(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def workspace_cap_env():
    """Upper bound of the workspace a launch call may use: $NSR_WIDE_WORKSPACE_GB, else 64 GiB (r06: of 288 GB; 16 GiB cost a 400x400 forward + gradient call
    6-8 % in chunk overheads, profiles/r06/extra/ab_wide_h2_w512.txt) -- and never more than half of the free memory
    (workspace_cap_bytes).  A smaller workspace means more,
    smaller chunks of rays.  On fp32 and bf16x3 handles that is never another result, and on an f16x2 handle neither while no pass
    leaves fp16's range.  An f16x2 pass that does is re-run on bf16x3 over its whole chunk (rerun="pass", the default): results then
    stay arithmetic-equivalent -- fp32-grade either way -- but are not bit-stable across chunkings, since which rays share a re-run
    pass depends on the chunk.  With rerun="rows" only the points that left the range are re-computed, and the bits are a ray's own:
    stable across chunkings and neighbours."""
    return int(float(os.environ.get("NSR_WIDE_WORKSPACE_GB", "64")) * (1 << 30))


def workspace_cap_bytes(device, reusable=0):
    """... and never more than half of what the device has free (`reusable`: bytes of a buffer that is about to be released).
    Only consulted when the shared workspace has to GROW (WideModel._workspace): one driver query per growth, not per launch."""
    free, _ = torch.cuda.mem_get_info(device)
    return min(workspace_cap_env(), (free + reusable) // 2)


def _cuda_f32(x, device=None):
    t = torch.as_tensor(x, dtype=torch.float32)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise _lib.NsrError("no HIP device visible: the render path has no CPU fallback")
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous()


def sample_pdf(bins, weights, u):
    """nsrw_sample_pdf: sample_pdf (RH:199-243) for any bin / sample count.  bins [..., B], weights [..., B - 1]; u: [S] (shared by
    all rows: det=True) or [..., S] (det=False).  -> (samples [..., S] float32, inds [..., S] int64) on the device."""
    lib = load()
    bins = _cuda_f32(bins)
    dev = bins.device
    weights, u = _cuda_f32(weights, dev), _cuda_f32(u, dev)
    lead, B = tuple(bins.shape[:-1]), int(bins.shape[-1])
    if tuple(weights.shape) != lead + (B - 1,):
        raise ValueError("sample_pdf: weights must be bins' shape with one entry less (got %r, %r)" % (tuple(bins.shape), tuple(weights.shape)))
    S = int(u.shape[-1])
    per_row = u.dim() > 1
    if per_row and tuple(u.shape[:-1]) != lead:
        raise ValueError("sample_pdf: per-row uniforms must have bins' leading shape")
    if not 2 <= B <= MAX_SAMPLES or not 1 <= S <= MAX_SAMPLES:
        raise NotImplementedError("sample_pdf: 2..%d bins and 1..%d samples (got %d, %d)" % (MAX_SAMPLES, MAX_SAMPLES, B, S))
    n = int(np.prod(lead)) if lead else 1
    samples = torch.empty(lead + (S,), dtype=torch.float32, device=dev)
    inds = torch.empty(lead + (S,), dtype=torch.int64, device=dev)
    scratch = torch.empty(2 * n * (B + 1), dtype=torch.float32, device=dev)
    check(lib.nsrw_sample_pdf(dev.index, _dev(bins), _dev(weights), n, B, _dev(u), 1 if per_row else 0, S, _dev(samples), _dev(inds),
                              _dev(scratch), _stream_ptr(dev)))
    return samples, inds


def embed_vjp(x, grad_out, multires):
    """nsrw_embed_vjp: d(sum(embed(x) * grad_out)) / dx for x [..., 3], grad_out [..., 3 + 6 multires]."""
    lib = load()
    x = _cuda_f32(x)
    g = _cuda_f32(grad_out, x.device)
    if x.shape[-1:] != (3,) or tuple(g.shape) != tuple(x.shape[:-1]) + (3 + 6 * int(multires),):
        raise ValueError("embed_vjp: x [..., 3] and grad_out [..., 3 + 6 multires] (got %r, %r)" % (tuple(x.shape), tuple(g.shape)))
    gx = torch.empty_like(x)
    n = x.numel() // 3
    check(lib.nsrw_embed_vjp(x.device.index, _dev(x), _dev(g), n, int(multires), _dev(gx), _stream_ptr(x.device)))
    return gx


# ONE workspace per (device, stream), shared by every handle that launches there: a handle's launch calls are stream-ordered, so
# two handles on one stream can never use it at the same time, and the drop-in API's cache of up to eight handles per module
# (render options x streams) does not multiply a buffer of tens of GiB.  release_workspaces() hands the memory back to torch.
_WORKSPACES = {}


def release_workspaces():
    _WORKSPACES.clear()


class WideModel:
    variant = 0
    schedule = "layers"

    def __init__(self, sd_coarse, sd_fine=None, device=None, n_importance=128, white_bkgd=False, lindisp=False, n_samples=64,
                 mlp=None, trunk=None, heads=None, trunk_width=None, trunk_bwd=None, trunk_keep=None, stages=None,
                 trunk_rerun=None, embed=None, rerun=None):
        """mlp: the arithmetic of the layer GEMMs -- "bf16x3" (bf16 MFMAs on three-way split fp32 operands, fp32-grade results at
        2.67x the matrix-pipe rate: csrc/nsr_wide_gemm.inc), "fp32" (fp32 MFMAs, the strict mode) or "f16x2" (fp16 MFMAs with
        two-piece operands -- the fused default kernel's arithmetic; a network pass that leaves fp16's range is re-run on bf16x3
        inside the call); default $NSR_WIDE_MLP, else DEFAULT_MLP.
        trunk: "layers" (a GEMM launch per pts_linears layer, activations through HBM) or "onchip" (f16x2 only: a network of
        padded width <= 128 and depth >= 2 runs its pts_linears in ONE launch with the activations in LDS wherever no activation is
        kept for a backward -- the same bits; any other network on the handle runs layer by layer: trunk_plan); default
        $NSR_WIDE_TRUNK (which handles of the other arithmetics ignore, while an explicit trunk="onchip" there raises), else "layers".
        heads: "layers" (a GEMM launch per head behind the trunk) or "onchip" (with trunk="onchip" only: wherever the trunk runs on
        chip the heads run behind it in the same launch and only the raw outputs reach memory -- the same bits: heads_plan);
        default $NSR_WIDE_HEADS (which handles that cannot honour it ignore, while an explicit heads="onchip" there raises), else
        "layers".
        trunk_width: the largest padded width trunk="onchip" takes -- 128, or 256 (with trunk="onchip" only: networks of padded
        width 160 .. 256 run their pts_linears in one launch too, on blocks of 64 points instead of 128 -- the same bits; their
        heads stay a launch each, whatever `heads` says); default $NSR_WIDE_TRUNK_WIDTH (which handles that cannot honour it ignore,
        while an explicit trunk_width=256 there raises), else 128.
        trunk_bwd: "layers" (the gradient calls run a GEMM launch per product of the input-gradient chain) or "onchip" (with
        trunk="onchip" only: a network the on-chip trunk takes in its 128-row form runs that chain in ONE launch behind the
        backward's head launches, the gradient between two layers in LDS -- the same bits; the kept forward pass and any other
        network stay layer by layer: trunk_bwd_plan); default $NSR_WIDE_TRUNK_BWD (which handles that cannot honour it ignore, while
        an explicit trunk_bwd="onchip" there raises), else "layers".
        trunk_keep: "layers" (a forward pass that keeps its activations for a backward runs a GEMM launch per layer and keeps fp32
        rows) or "onchip" (with trunk="onchip" and trunk_bwd="onchip" only: on a network whose backward trunk is on chip the f16x2
        pass of such a forward is ONE launch too -- with heads="onchip" the heads behind it -- and keeps the relu masks as one bit per
        (point, unit), which the on-chip backward reads -- the same bits; the workspace of a gradient call grows by W / 8 bytes per
        point and kept layer: trunk_keep_plan, keep_status); default $NSR_WIDE_TRUNK_KEEP (which handles that cannot honour it
        ignore, while an explicit trunk_keep="onchip" there raises), else "layers".
        stages: "threads" (compositing, resampling and the compositing backward run one thread per ray) or "wave" (one wave per
        ray: consecutive lanes at consecutive samples, every ordered sum on one lane in its order -- the same bits; any arithmetic,
        any other knob; the workspace and the chunks are the same: stage_plan, stages_status); default $NSR_WIDE_STAGES, else
        "threads".
        trunk_rerun: "layers" (the conditional bf16x3 re-run of a pass that left fp16's range is a GEMM launch per layer, fp32
        activations through HBM) or "onchip" (with trunk="onchip" only: where the trunk ran on chip in its 128-row form and no
        activation is kept, the re-run's pts_linears are ONE conditional launch with the activations in LDS, the heads a launch each
        behind it -- the same bits; the re-run of a kept pass and of a backward stay layer by layer: trunk_rerun_plan,
        rerun_status); default $NSR_WIDE_TRUNK_RERUN (which handles that cannot honour it ignore, while an explicit
        trunk_rerun="onchip" there raises), else "layers".
        embed: "layers" (the kw_embed launch writes the encodings of every pass, and the pass reads them back) or "onchip" (with
        trunk="onchip" only: wherever the f16x2 pass of a network is one on-chip launch -- trunk, heads form, wide form, kept
        forward -- that launch computes the position encodings of its points itself, and in a heads form the direction encodings
        too; behind a trunk-only launch kw_embed writes the direction encodings alone; a conditional kw_embed stands in front of the
        bf16x3 re-run -- the same bits, the same workspace: embed_plan, embed_status); default $NSR_WIDE_EMBED (which handles that
        cannot honour it ignore, while an explicit embed="onchip" there raises), else "layers".
        rerun: the unit of the f16x2 safety net -- "pass" (a network pass over a chunk in which any value reaches fp16's largest number
        is run again on bf16x3 as a whole: every ray of the chunk then has bf16x3's bits, so bits depend on the neighbours and on the
        chunk size once a pass re-runs) or "rows" (mlp="f16x2" with trunk="layers" only: the f16x2 GEMMs flag the points that leave the
        range, and the bf16x3 chain walks the tile blocks that hold one and stores those points alone -- a flagged point has a bf16x3
        handle's bits, every other point keeps its f16x2 bits, and a ray's bits depend on that ray only; range_status() counts
        `rows` / `rows_rerun`); default $NSR_WIDE_RERUN (which handles that cannot honour it ignore, while an explicit rerun="rows"
        there raises), else "pass"."""
        mlp = mlp or os.environ.get("NSR_WIDE_MLP") or DEFAULT_MLP
        if mlp not in MLPS:
            raise ValueError("mlp must be one of %s (got %r)" % (MLPS, mlp))
        knobs = resolve_knobs(mlp, dict(trunk=trunk, heads=heads, trunk_width=trunk_width, trunk_bwd=trunk_bwd, trunk_keep=trunk_keep,
                                        stages=stages, trunk_rerun=trunk_rerun, embed=embed, rerun=rerun), os.environ)
        for k in KNOBS:
            setattr(self, k.name, knobs[k.name])
        self.mlp = "layered-" + mlp
        if not torch.cuda.is_available():
            raise _lib.NsrError("no HIP device visible: the render path has no CPU fallback")
        self.lib = load()
        if isinstance(device, torch.device):
            device = device.index
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        n_samples, n_importance = int(n_samples), int(n_importance)
        if not 3 <= n_samples <= MAX_SAMPLES or not 0 <= n_importance <= MAX_SAMPLES:
            raise NotImplementedError("N_samples must be 3..%d and N_importance 0..%d (got %r, %r)"
                                      % (MAX_SAMPLES, MAX_SAMPLES, n_samples, n_importance))
        self.n_samples, self.n_importance = n_samples, n_importance
        self.ni_kernel = n_importance
        self.u_width = n_importance                       # rows of the u draws as nsrw_render_rays reads them
        self.nf_kernel = n_samples + n_importance
        self.white_bkgd, self.lindisp = bool(white_bkgd), bool(lindisp)
        self.rays_launched = 0
        self.workspace_bytes = 0
        self._util = None
        self._ws_need = {}                                # (rays, grad) -> bytes one chunk of that many rays needs
        cfg = NsrwConfig(self.device.index, n_samples, n_importance,
                         (FLAG_WHITE_BKGD if white_bkgd else 0) | (FLAG_LINDISP if lindisp else 0) |
                         _mlp_flags(mlp) | knob_flags(**knobs))
        h = C.c_void_p()
        check(self.lib.nsrw_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.upload(sd_coarse, sd_fine)
        t = torch.linspace(0., 1., steps=n_samples).numpy().astype(np.float32)          # RN:439: on the host, then moved
        u = torch.linspace(0., 1., steps=max(n_importance, 1)).numpy().astype(np.float32)   # RH:208
        check(self.lib.nsrw_upload_tables(self.h, t.ctypes.data_as(C.POINTER(C.c_float)), n_samples,
                                          u.ctypes.data_as(C.POINTER(C.c_float)), n_importance))

    def upload(self, sd_coarse, sd_fine=None):
        self.nets = []
        for net_id, sd in enumerate((sd_coarse, sd_fine)):
            if sd is None:
                continue
            net, flat = describe(sd)
            check(self.lib.nsrw_upload_network(self.h, net_id, C.byref(net), flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size))
            self.nets.append(net)
        last = self.nets[-1] if self.n_importance > 0 else self.nets[0]
        self.raw_ch = 4 if last.use_viewdirs else int(last.output_ch)
        self.raw_ch0 = 4 if self.nets[0].use_viewdirs else int(self.nets[0].output_ch)

    def close(self):
        if getattr(self, "h", None):
            self.lib.nsrw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers ------------------------------------------------------------------------------------
    def _f32(self, x, shape=None):
        t = torch.as_tensor(x, dtype=torch.float32, device=self.device).contiguous()
        return t.reshape(shape) if shape is not None else t

    def _new(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _need(self, n_rays, grad):
        """bytes one chunk of n_rays rays needs (cached per handle: the bilevel loop asks for the same 512 rays 313 times a pose).
        grad: 0 / False, 1 / True (the last pass's backward), 2 (the coarse pass's as well: nsrw_workspace_bytes)"""
        key = (int(n_rays), int(grad))
        v = self._ws_need.get(key)
        if v is None:
            need = C.c_size_t()
            check(self.lib.nsrw_workspace_bytes(self.h, key[0], key[1], C.byref(need)))
            v = self._ws_need[key] = int(need.value)
        return v

    def _workspace(self, n_rays, grad):
        """(shared workspace of this stream, bytes of it the launch call may use).  A buffer that already holds the call's one
        chunk -- or is as large as the cap allowed when it was made -- is reused without a driver query (the cap used
        to be recomputed from mem_get_info on every launch, AFTER the workspace itself had shrunk the free memory)."""
        floor = self._need(64, grad)
        need = max(min(self._need(n_rays, grad), workspace_cap_env()), floor)
        key = (self.device.index, torch.cuda.current_stream(self.device).cuda_stream)
        ws, capped = _WORKSPACES.get(key, (None, False))
        have = ws.numel() if ws is not None else 0
        if have < need and not (capped and have >= floor):
            want = max(min(need, workspace_cap_bytes(self.device, have)), floor)
            if want > have:
                _WORKSPACES.pop(key, None)                     # release before asking for the larger one
                ws = None
                ws = torch.empty(want, dtype=torch.uint8, device=self.device)
                have = want
            _WORKSPACES[key] = (ws, have < need)               # capped: as large as the device allows -- do not ask again
        use = min(need, have)
        self.workspace_bytes = use                             # what the launch call is told it may use (<= the shared buffer)
        return ws, use

    def _extras(self, extras, n):
        if not extras or all(v is None for v in extras.values()):
            return None, None
        widths = dict(viewdirs=3, near=1, far=1, t_rand=self.n_samples, u=self.n_importance, noise0=self.n_samples,
                      noise1=self.nf_kernel, z_fine=self.nf_kernel)
        unknown = set(extras) - set(widths)
        if unknown:
            raise ValueError("unknown ray extras: %s" % sorted(unknown))
        keep = {k: self._f32(v, (n, widths[k])) for k, v in extras.items() if v is not None}
        if ("near" in keep) != ("far" in keep):
            raise ValueError("per-ray bounds: near and far come together")
        ex = NsrwExtras(*[_dev(keep.get(k)) for k in ("viewdirs", "near", "far", "t_rand", "u", "noise0", "noise1", "z_fine")])
        return ex, keep

    def _outs(self, n, debug):
        fine = self.n_importance > 0
        o = dict(rgb_map=self._new(n, 3), disp_map=self._new(n), acc_map=self._new(n))
        if fine:
            o.update(rgb0=self._new(n, 3), disp0=self._new(n), acc0=self._new(n), z_std=self._new(n))
        d = {}
        if debug:                                   # engine.NsrModel's tap names
            d = dict(weights0=self._new(n, self.n_samples), raw0=self._new(n, self.n_samples, self.raw_ch0))
            if fine:
                d.update(z_samples=self._new(n, self.n_importance), inds=self._new(n, self.n_importance, dtype=torch.int64),
                         z_fine=self._new(n, self.nf_kernel), raw=self._new(n, self.nf_kernel, self.raw_ch))
            else:
                d.update(z_coarse=self._new(n, self.n_samples))
            o.update(d)
        last_raw, last_z = (d.get("raw"), d.get("z_fine")) if fine else (d.get("raw0"), d.get("z_coarse"))
        out = NsrwOut(_dev(o["rgb_map"]), _dev(o["disp_map"]), _dev(o["acc_map"]), _dev(o.get("rgb0")), _dev(o.get("disp0")),
                      _dev(o.get("acc0")), _dev(o.get("z_std")), _dev(last_raw), _dev(last_z), _dev(d.get("weights0")),
                      _dev(d.get("z_samples")), _dev(d.get("inds")), _dev(d.get("raw0")) if fine else None)
        return o, out

    @property
    def util(self):
        """the fused library's handle for the network-free stage kernels (get_rays, pose_grad, ndc_rays)"""
        if self._util is None:
            from .run_nerf_noscale import _util_model
            self._util = _util_model(self.device)
        return self._util

    # ---- the path -----------------------------------------------------------------------------------
    def render_rays(self, rays_o, rays_d, near, far, debug=False, extras=None):
        """render(rays=...) (RN:58-123): rays_o, rays_d [N,3] -> dict of [N,...] tensors on the device (engine.NsrModel's keys;
        debug adds raw / z_fine / weights0 / z_samples / inds)."""
        rays_o, rays_d = self._f32(rays_o, (-1, 3)), self._f32(rays_d, (-1, 3))
        n = rays_o.shape[0]
        self.rays_launched += n
        o, out = self._outs(n, debug)
        ex, keep = self._extras(extras, n)
        ws, nbytes = self._workspace(n, False)
        check(self.lib.nsrw_render_rays(self.h, _dev(rays_o), _dev(rays_d), n, float(near), float(far), C.byref(ex) if ex else None,
                                        C.byref(out), _dev(ws), nbytes, _stream_ptr(self.device)))
        return o

    def render_views(self, c2w, H, W, K, near, far, debug=False):
        """render(c2w=...) for V views: get_rays (RH:156-165) for all of them in ONE launch into one buffer (nsr_get_rays_views;
        r05 ran a launch per view and concatenated), then ONE render_rays call."""
        ro, rd = self.util.get_rays_views(int(H), int(W), K, self._f32(c2w))
        return self.render_rays(ro, rd, near, far, debug=debug)

    def render_rays_vjp(self, rays_o, rays_d, near, far, grad_rgb=None, with_forward=False, z_fine=None, extras=None, debug=False,
                        cotangents=None):
        """Forward + input-side VJP (RN:168-178): grad_rgb [N,3] -> (grad_rays_o, grad_rays_d) [N,3] each (+ grad_viewdirs with
        extras["viewdirs"], + the forward's rgb / disp / acc with with_forward).
        cotangents: {output name: cotangent} for any of render()'s differentiable outputs (COTANGENTS: rgb_map / disp_map / acc_map
        of the last pass, rgb0 / disp0 / acc0 of the coarse one when N_importance > 0) instead of -- or, for rgb_map, besides --
        grad_rgb: the gradient of the sum of their contractions (nsrw_render_rays_vjp_cot).  A missing or None entry contributes
        nothing; a given one follows torch's autograd of the reference, NaN included."""
        if debug:
            raise NotImplementedError("the layered renderer has no relu taps")
        if z_fine is not None:                      # given depths for the fine pass (constants of the gradient, RN:475)
            extras = dict(extras or {}, z_fine=z_fine)
        rays_o, rays_d = self._f32(rays_o, (-1, 3)), self._f32(rays_d, (-1, 3))
        n = rays_o.shape[0]
        self.rays_launched += n
        cot = None
        if cotangents is not None:
            cot = {k: v for k, v in dict(cotangents).items() if v is not None}
            unknown = set(cot) - set(COTANGENTS)
            if unknown:
                raise ValueError("cotangents: not differentiable outputs of render(): %s (z_std and raw are not: RN:475)" % sorted(unknown))
            if grad_rgb is not None:
                if "rgb_map" in cot:
                    raise ValueError("grad_rgb and cotangents['rgb_map'] both given")
                cot["rgb_map"] = grad_rgb
            if self.n_importance == 0 and any(k in cot for k in COARSE_COTANGENTS):
                raise ValueError("cotangents %s: a coarse-only handle's outputs are rgb_map / disp_map / acc_map"
                                 % sorted(k for k in cot if k in COARSE_COTANGENTS))
            cot = {k: self._f32(v, (n, COTANGENTS[k][1]) if COTANGENTS[k][1] > 1 else (n,)) for k, v in cot.items()}
        elif grad_rgb is None:
            raise ValueError("render_rays_vjp: grad_rgb or cotangents")
        go, gd = self._new(n, 3), self._new(n, 3)
        fwd, out = None, None
        if with_forward:
            fwd = dict(rgb_map=self._new(n, 3), disp_map=self._new(n), acc_map=self._new(n))
            out = NsrwOut(_dev(fwd["rgb_map"]), _dev(fwd["disp_map"]), _dev(fwd["acc_map"]))
        ex, keep = self._extras(extras, n)
        gv = self._new(n, 3) if (keep and "viewdirs" in keep) else None
        if cot is None:
            g = self._f32(grad_rgb, (n, 3))
            ws, nbytes = self._workspace(n, True)
            check(self.lib.nsrw_render_rays_vjp(self.h, _dev(rays_o), _dev(rays_d), n, float(near), float(far),
                                                C.byref(ex) if ex else None, _dev(g), C.byref(out) if out else None, _dev(go),
                                                _dev(gd), _dev(gv), _dev(ws), nbytes, _stream_ptr(self.device)))
        else:
            ct = NsrwCotangents(*[_dev(cot.get(k)) for k in COTANGENTS])
            coarse = self.n_importance > 0 and any(k in cot for k in COARSE_COTANGENTS)
            ws, nbytes = self._workspace(n, 2 if coarse else 1)
            check(self.lib.nsrw_render_rays_vjp_cot(self.h, _dev(rays_o), _dev(rays_d), n, float(near), float(far),
                                                    C.byref(ex) if ex else None, C.byref(ct), C.byref(out) if out else None,
                                                    _dev(go), _dev(gd), _dev(gv), _dev(ws), nbytes, _stream_ptr(self.device)))
        res = (go, gd) if gv is None else (go, gd, gv)
        return res + (fwd,) if with_forward else res

    def run_network(self, pts, viewdirs, net_id=0):
        """run_network (RN:26-40): pts [..,3], viewdirs [..,3] (unit length) -> raw [.., 4 or output_ch]."""
        shape = tuple(torch.as_tensor(pts).shape[:-1])
        p = self._f32(pts, (-1, 3))
        net = self.nets[net_id]
        v = self._f32(viewdirs, (-1, 3)) if net.use_viewdirs else None
        ch = 4 if net.use_viewdirs else int(net.output_ch)
        raw = self._new(p.shape[0], ch)
        ws, nbytes = self._workspace(max(1, p.shape[0] // max(self.nf_kernel, 1) + 1), False)
        check(self.lib.nsrw_run_network(self.h, int(net_id), _dev(p), _dev(v), p.shape[0], _dev(raw), _dev(ws), nbytes,
                                        _stream_ptr(self.device)))
        return raw.reshape(shape + (ch,))

    # network-free stage kernels: the fused library's
    def get_rays(self, H, W, K, c2w):
        return self.util.get_rays(H, W, K, c2w)

    def pose_grad(self, grad_o, grad_d, H, W, K, patch):
        return self.util.pose_grad(grad_o, grad_d, H, W, K, patch)

    def ndc_rays(self, *a, **k):
        return self.util.ndc_rays(*a, **k)

    def ndc_rays_vjp(self, *a, **k):
        return self.util.ndc_rays_vjp(*a, **k)

    def range_status(self):
        """fp32 / bf16x3: no range to leave.  f16x2: `passes` network passes launched so far, `passes_rerun` of them re-run on
        bf16x3 because an activation reached fp16's largest number; nothing is ever dropped.  (The keys of NsrModel.range_status
        are kept: `points` / `rays` stay 0 -- the unit of the layered renderer's safety net is a pass over a chunk of rays.)
        rerun="rows" handles: `rows` points those passes covered and `rows_rerun` of them re-computed on bf16x3 (a pass counts in
        `passes_rerun` when any of its rows was); both 0 on every other handle."""
        out = dict(last_items=0, points=0, rays=0, dropped_items=0, passes=0, passes_rerun=0, rows=0, rows_rerun=0)
        if self.mlp == "layered-f16x2":
            a, b = C.c_ulonglong(), C.c_ulonglong()
            check(self.lib.nsrw_range_status(self.h, C.byref(a), C.byref(b)))
            out["passes"], out["passes_rerun"] = int(a.value), int(b.value)
            if self.rerun == "rows":
                check(self.lib.nsrw_range_rows_status(self.h, C.byref(a), C.byref(b)))
                out["rows"], out["rows_rerun"] = int(a.value), int(b.value)
        return out

    def keep_status(self):
        """nsrw_keep_status: `passes_onchip` kept forward passes launched on chip so far (trunk_keep="onchip" handles; 0 elsewhere)"""
        n = C.c_ulonglong()
        check(self.lib.nsrw_keep_status(self.h, C.byref(n)))
        return dict(passes_onchip=int(n.value))

    def stages_status(self):
        """nsrw_stages_status: `launches_wave` wave-per-ray stage launches enqueued so far (stages="wave" handles; 0 elsewhere)"""
        n = C.c_ulonglong()
        check(self.lib.nsrw_stages_status(self.h, C.byref(n)))
        return dict(launches_wave=int(n.value))

    def rerun_status(self):
        """nsrw_rerun_status: `launches_onchip` conditional kw_rerun_b3 launches enqueued so far, whether or not their pass left
        the range (trunk_rerun="onchip" handles; 0 elsewhere)"""
        n = C.c_ulonglong()
        check(self.lib.nsrw_rerun_status(self.h, C.byref(n)))
        return dict(launches_onchip=int(n.value))

    def embed_status(self):
        """nsrw_embed_status, counted on the host as enqueued: `passes_onchip` network passes whose f16x2 launch computed its position
        encodings itself (embed="onchip" handles; 0 elsewhere), `embed_launches` unconditional kw_embed launches (whole, or the
        direction encodings alone), `embed_launches_conditional` kw_embed launches in front of a bf16x3 re-run"""
        a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        check(self.lib.nsrw_embed_status(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(passes_onchip=int(a.value), embed_launches=int(b.value), embed_launches_conditional=int(c.value))

    def debug_bounds_status(self):
        """(built_with_checks, first_bad_line): see nsrw_debug_bounds_status / `make debug`."""
        built, line = C.c_int(), C.c_uint()
        check(self.lib.nsrw_debug_bounds_status(C.byref(built), C.byref(line)))
        return bool(built.value), int(line.value)

    def last_kernel_ms(self):
        """(device ms of the last launch call, chunks of rays it ran)"""
        ms, ch = C.c_float(), C.c_int()
        check(self.lib.nsrw_last_ms(self.h, C.byref(ms), C.byref(ch)))
        return float(ms.value), int(ch.value)
