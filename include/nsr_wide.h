/*
 * nsr_wide.h -- C ABI of the LAYERED renderer inside libnsr.so: the same path as include/nsr.h (render_rays RN:390-501 and its
 * input-side VJP, RN:168-178) for the configurations the fused kernels are not built for -- a NeRF (RH:70-122) of ANY depth,
 * width and skip list, any N_samples / N_importance (RN:439, RN:474), with or without view directions.
 *
 * (RN = optimization/utils/run_nerf_noscale.py, RH = optimization/utils/run_nerf_helpers.py of the reference.)
 *
 * Design: one MFMA GEMM kernel per network layer over ALL points of a chunk of rays -- on fp16 MFMAs with two-piece
 * operands, on bf16 MFMAs with three-piece operands or on fp32 MFMAs (NsrwConfig.flags), fp32 in HBM and fp32-grade results in
 * every case -- activations resident in HBM between the layers (288 GB: a chunk is thousands of rays), the per-ray stages (depths,
 * compositing RN:343-387, resampling RH:199-243, sort RN:477) as small kernels of their own between them, and for the gradient the
 * same GEMM kernel on the transposed weights with the relu masks read back from the stored activations.  Nothing here runs on the host CPU
 * and nothing falls back to another library: a network the fused kernels cannot hold costs layer-by-layer HBM traffic, not
 * correctness.
 *
 * Conventions are those of include/nsr.h: int status (0 = OK, message via nsrw_last_error), caller-owned DEVICE buffers passed
 * as raw pointers, stream-ordered, no hidden synchronisation in the launch calls, one handle per (model, stream); a handle is
 * not thread-safe, distinct handles are.  The scratch memory is the CALLER's too: nsrw_workspace_bytes says how much one
 * chunk of rays needs, the launch calls split the rays into as many chunks as the workspace they are handed allows.  Chunking never
 * changes a result on fp32 and bf16x3 handles, nor on an f16x2 handle while no pass leaves fp16's range; an f16x2 pass that does is
 * re-run on bf16x3 over its whole chunk, so there the results are arithmetic-equivalent (fp32-grade either way) but not bit-stable
 * across chunkings -- unless the handle has NSRW_FLAG_RERUN_ROWS, whose re-run is per point and whose results are bit-stable.
 */
#ifndef NSR_WIDE_H_
#define NSR_WIDE_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct NsrwHandle_* nsrw_handle;

#define NSRW_MAX_SKIPS 16
#define NSRW_MAX_DEPTH 64
#define NSRW_MAX_WIDTH 4096
#define NSRW_MAX_SAMPLES 512         /* N_samples, N_importance (torch.sum's first cascade level: oracle/_torch_sum_lastdim) */

enum { NSRW_FLAG_WHITE_BKGD = 1,     /* RN:384-385 */
       NSRW_FLAG_LINDISP = 2,        /* RN:443 */
       NSRW_FLAG_MLP_BF16X3 = 4,     /* r06: the layer GEMMs on bf16 MFMAs, every fp32 operand split exactly into three bf16 pieces, six
                                      * piece products per product, fp32 accumulate (csrc/nsr_wide_gemm.inc): fp32-grade results, fp32's
                                      * exponent range, 2.67x the matrix-pipe rate of the fp32 MFMAs.  Without a flag: fp32 MFMAs. */
       NSRW_FLAG_MLP_F16X2 = 8 };    /* r06: the layer GEMMs on fp16 MFMAs, every fp32 operand as two fp16 pieces, three piece products
                                      * (the arithmetic of the fused default kernel, csrc/nsr_h2.inc: |error| <= 2^-22 per product;
                                      * weights pre-scaled per matrix, gradients normalised per point).  A network pass -- forward or
                                      * backward -- in which a value reaches fp16's largest number is run again on bf16x3 inside the
                                      * same call (nsrw_range_status counts them), so no result depends on the range: a re-run pass has
                                      * bf16x3's bits, which are fp32-grade like f16x2's but not the same.  The unit of that re-run is
                                      * the pass over a chunk, so once a pass re-runs a ray's BITS depend on its chunk's other rays and
                                      * on the chunk size (arithmetic-equivalent, not bit-stable); NSRW_FLAG_RERUN_ROWS makes the unit
                                      * the point, and the bits a ray's own. */
enum { NSRW_FLAG_TRUNK_ONCHIP = 16 };/* opt-in, f16x2 handles only (nsrw_create refuses it without NSRW_FLAG_MLP_F16X2): a network of padded width
                                      * <= 128 and depth >= 2 runs ALL its pts_linears in one launch with the activations in LDS
                                      * (csrc/nsr_wide_trunk.inc) wherever no activation is kept for a backward -- the same arithmetic per
                                      * output element, so the same bits as layer by layer.  Any other network on such a handle runs
                                      * layer by layer, as do the bf16x3 re-runs (nsrw_trunk_plan says which). */

enum { NSRW_FLAG_HEADS_ONCHIP = 32 };/* opt-in, with NSRW_FLAG_TRUNK_ONCHIP only (nsrw_create refuses it without): wherever the trunk runs on chip
                                      * the heads -- alpha_linear, feature_linear, views_linears.0 and rgb_linear, or output_linear --
                                      * run behind it in the same launch on the same rows, and nothing but the raw outputs of a point
                                      * reaches memory; the same arithmetic per output element, so the same bits.  With view directions
                                      * the direction encoding must be at most 96 columns wide (multires_views <= 15 is); otherwise
                                      * the heads stay one launch each behind the trunk launch (nsrw_heads_plan says which). */

enum { NSRW_FLAG_TRUNK_WIDE = 64 }; /* opt-in, with NSRW_FLAG_TRUNK_ONCHIP only (nsrw_create refuses it without): the on-chip trunk also takes
                                      * networks of padded width 160 .. 256 (the other conditions unchanged), in its wide form -- blocks
                                      * of 64 points instead of 128, the same arithmetic per output element, so the same bits.  The
                                      * heads of such a network stay one launch each behind the trunk launch, NSRW_FLAG_HEADS_ONCHIP
                                      * or not; networks of padded width <= 128 run as without this flag. */

enum { NSRW_FLAG_TRUNK_BWD = 128 }; /* opt-in, with NSRW_FLAG_TRUNK_ONCHIP only (nsrw_create refuses it without, hence without NSRW_FLAG_MLP_F16X2):
                                      * the gradient calls run the input-gradient chain of a network the on-chip trunk serves in its
                                      * 128-row form -- per pts layer the products with the transposed weights, the relu masks read from
                                      * the kept activations -- in one launch behind the backward's head launches, the gradient between
                                      * two layers in LDS (kw_trunk_bwd_h2); the same arithmetic per output element, so the same bits.
                                      * The kept forward pass, the bf16x3 re-runs and the networks of the wide form stay layer by layer
                                      * (nsrw_trunk_bwd_plan says which). */

enum { NSRW_FLAG_TRUNK_KEEP = 256 };/* opt-in, with NSRW_FLAG_TRUNK_BWD only (nsrw_create refuses it without, hence without NSRW_FLAG_TRUNK_ONCHIP and
                                      * NSRW_FLAG_MLP_F16X2): on a network whose backward trunk is on chip the f16x2 pass of every forward
                                      * that KEEPS its activations for a backward -- the last network's, and the coarse network's second
                                      * one under coarse cotangents -- runs as one launch too (kw_keep_h2; with NSRW_FLAG_HEADS_ONCHIP the
                                      * heads behind it).  It leaves the relu masks of the layers 0 .. D - 2 as one bit per (point, unit)
                                      * instead of fp32 rows, and the on-chip backward reads those bits (kw_keep_bwd_h2); the last
                                      * layer's and views_linears.0's fp32 outputs stay, for the backward's head launches.  The same
                                      * arithmetic per output element, so the same bits; the bf16x3 re-runs stay layer by layer on fp32
                                      * activations, with a conversion between the two forms in front of or behind them.  The workspace
                                      * of a gradient call grows by the masks, W / 8 bytes per point and kept layer
                                      * (nsrw_trunk_keep_plan says which networks; nsrw_keep_status counts the passes). */

enum { NSRW_FLAG_STAGES_WAVE = 512 };   /* opt-in, any arithmetic, needs nothing beside it */
                                     /* The render and gradient calls run the per-ray stages between the network passes -- compositing
                                      * (RN:343-387), resampling (RH:199-243) and the compositing backward -- with ONE WAVE per ray
                                      * (csrc/nsr_wide_stages.inc) instead of one thread: consecutive lanes at consecutive samples,
                                      * every sum and product whose order the reference fixes on one lane in that order -- the same
                                      * IEEE operations on the same values in the same order, so the same bits in every output, tap
                                      * and gradient.  The workspace and the chunking are unchanged (nsrw_stage_plan says how a stage
                                      * runs; nsrw_stages_status counts the launches).  The stage entry nsrw_sample_pdf stays as it is. */

enum { NSRW_FLAG_TRUNK_RERUN = (1 << 10) }; /* opt-in, with NSRW_FLAG_TRUNK_ONCHIP only (nsrw_create refuses it without, hence without NSRW_FLAG_MLP_F16X2) */
                                     /* On a network whose trunk runs on chip in its 128-row form, the conditional bf16x3 re-run of a
                                      * forward pass that keeps no activations runs its pts_linears as ONE launch too (kw_rerun_b3:
                                      * the bf16x3 arithmetic of the per-layer chain per output element, activations in LDS, tiles of
                                      * 128 points up to a padded width of 64 and of 64 points at 96 and 128), which returns at once
                                      * unless the f16x2 pass left fp16's range; the re-run's heads stay a conditional launch each
                                      * behind it.  The same bits.  The re-run of a kept pass and of a backward, and the networks of
                                      * the wide form, stay layer by layer (nsrw_trunk_rerun_plan says which networks;
                                      * nsrw_rerun_status counts the launches).  The workspace is unchanged. */

enum { NSRW_FLAG_EMBED_ONCHIP = (1 << 11) }; /* opt-in, with NSRW_FLAG_TRUNK_ONCHIP only (nsrw_create refuses it without, hence without NSRW_FLAG_MLP_F16X2) */
                                     /* Wherever the f16x2 pass of a network runs as one on-chip launch -- the trunk's, the heads form's,
                                      * the wide form's, the kept forward's -- that launch computes the position encodings of its block
                                      * of points itself, from the rays and depths (or the points of nsrw_run_network), by the very
                                      * functions of the encoding kernel: the kw_embed launch, its write of [P, Ci] floats and the
                                      * trunk's read of them go.  In a heads form the direction encodings too; behind a trunk-only or
                                      * wide launch the heads are launches that read them from memory, so kw_embed still writes them
                                      * (alone).  The same bits.  The conditional bf16x3 re-run reads encodings from memory: an
                                      * encoding launch conditional on the range word stands in front of it.  A pass that runs layer
                                      * by layer is encoded as without the flag.  The workspace and the chunking are unchanged
                                      * (nsrw_embed_plan says which encodings of which pass; nsrw_embed_status counts). */

enum { NSRW_FLAG_RERUN_ROWS = (1 << 12) }; /* opt-in, f16x2 handles without NSRW_FLAG_TRUNK_ONCHIP only (nsrw_create refuses it otherwise) */
                                     /* The range safety net per POINT instead of per pass: the f16x2 GEMMs of a pass set one bit per row
                                      * (point) in which a value they split reaches fp16's largest number; a small kernel lists the
                                      * 256-row and 128-row tile blocks that hold such a row; the bf16x3 chain then walks the listed
                                      * blocks alone and stores only the flagged rows -- with the sums of a whole-pass bf16x3 re-run, so a
                                      * flagged point has a bf16x3 handle's bits and every other point keeps its f16x2 bits.  Which of
                                      * the two a point gets depends on that point's own values, so a ray's bits depend on the ray alone:
                                      * not on its neighbours, not on the chunk size.  Stream-ordered and capturable like the per-pass
                                      * form.  nsrw_range_status keeps its meaning (a pass counts as re-run when any row was flagged),
                                      * nsrw_range_rows_status counts rows.  The workspace grows by the bits and the two lists, about
                                      * 0.2 bytes per point. */

typedef struct NsrwConfig {
  int32_t device;
  int32_t n_samples;                 /* N_samples (RN:439): 3 .. NSRW_MAX_SAMPLES -- sample_pdf needs an interior weight; nsrw_create refuses less */
  int32_t n_importance;              /* N_importance >= 0 (RN:474); 0 = coarse only */
  int32_t flags;
  int32_t reserved[4];
} NsrwConfig;

/* One NeRF module (RH:70-97).  input_ch = 3 + 6 multires, input_ch_views = 3 + 6 multires_views (get_embedder RH:51-66;
 * multires = 0 is i_embed = -1, the identity).  skips: layer indices i whose OUTPUT is concatenated behind the input
 * encoding (RH:105-106), each < D - 1.  use_viewdirs = 0: outputs = output_linear(h) with output_ch rows (RH:119-120), of
 * which render_rays reads the first four. */
typedef struct NsrwNet {
  int32_t D, W;
  int32_t multires, multires_views;
  int32_t use_viewdirs;
  int32_t output_ch;
  int32_t n_skips;
  int32_t skips[NSRW_MAX_SKIPS];
} NsrwNet;

/* Per-ray inputs of the options beyond the deterministic test-time path, all nullable DEVICE pointers (cf. NsrRayExtras):
 * viewdirs [N,3] given view directions (c2w_staticcam RN:91-96, ndc RN:101-103); near / far [N] (RN:106-108);
 * t_rand [N, N_samples] (RN:451), u [N, N_importance] (RH:211), noise0 [N, N_samples] / noise1 [N, N_samples + N_importance]
 * (RN:365-374, already multiplied by raw_noise_std); z_fine [N, N_samples + N_importance]: sorted sample depths the fine pass
 * is to use INSTEAD of its own resampling (z_samples is detached, RN:475: the depths are constants of the gradient -- this is how
 * the parity tests differentiate at the reference's own depths). */
typedef struct NsrwExtras {
  const float* d_viewdirs;
  const float* d_near;
  const float* d_far;
  const float* d_t_rand;
  const float* d_u;
  const float* d_noise0;
  const float* d_noise1;
  const float* d_z_fine;
} NsrwExtras;

/* Outputs, all nullable DEVICE pointers: the returns of render_rays (RN:488-495) -- rgb [N,3], disp [N], acc [N] of the last
 * pass, rgb0 / disp0 / acc0 of the coarse pass and z_std [N] when N_importance > 0 -- plus the taps the parity tests read:
 * raw [N, S, C] of the last pass (retraw; C = 4, or output_ch without view directions), z_vals [N, S] of the last pass,
 * weights0 [N, N_samples] of the coarse pass, z_samples [N, N_importance], inds int64 [N, N_importance], raw0 [N, N_samples, C]
 * of the coarse pass when there is a fine one. */
typedef struct NsrwOut {
  float* d_rgb;
  float* d_disp;
  float* d_acc;
  float* d_rgb0;
  float* d_disp0;
  float* d_acc0;
  float* d_z_std;
  float* d_raw;
  float* d_z_vals;
  float* d_weights0;
  float* d_z_samples;
  int64_t* d_inds;
  float* d_raw0;
} NsrwOut;

const char* nsrw_last_error(void);

/* Which opt-in flags go together is stated once on each side of this interface: the table kFlagNeeds in csrc/nsr_wide.hip (what each
 * flag needs and excludes; nsrw_create refuses the first row that is not met, nsrw_flags_refusal says which) and wide.KNOBS in
 * neural_sim_nerf_amd/wide.py (the same for WideModel's arguments).  tests/test_wide_options_host.py holds the two to each other. */
int nsrw_create(const NsrwConfig* cfg, nsrw_handle* out);
int nsrw_destroy(nsrw_handle h);

/* Network net_id (0 = network_fn, 1 = network_fine) from HOST memory: the parameters in the module's own order and layout
 * (torch [out, in] row-major), weight then bias per layer -- pts_linears.0 .. D-1, then with view directions feature_linear,
 * alpha_linear, views_linears.0, rgb_linear, without them output_linear.  SETUP call: allocates, copies, synchronises. */
int nsrw_upload_network(nsrw_handle h, int net_id, const NsrwNet* net, const float* weights, size_t n_floats);
/* Number of floats nsrw_upload_network expects for `net` (0 if the description is invalid; nsrw_last_error says why). */
size_t nsrw_network_floats(const NsrwNet* net);

/* torch.linspace(0, 1, N_samples) and torch.linspace(0, 1, N_importance) as the HOST's torch computes them (RN:439, RH:208:
 * ATen's values are not np.linspace's); n_fine may be 0.  SETUP call. */
int nsrw_upload_tables(nsrw_handle h, const float* t_coarse, int n_coarse, const float* u_fine, int n_fine);

/* Bytes of workspace ONE chunk of `rays` rays needs (with_grad = 1: for nsrw_render_rays_vjp, which keeps every activation of the
 * last network; with_grad = 2: for nsrw_render_rays_vjp_cot with a coarse cotangent and N_importance > 0, whose gradient
 * buffers hold either network).  The launch calls accept any workspace that holds a chunk of at least 64 rays; the chunk
 * size decides nothing but how many rays one f16x2 re-run covers (per-pass re-run; with NSRW_FLAG_RERUN_ROWS nothing at all). */
int nsrw_workspace_bytes(nsrw_handle h, int64_t rays, int with_grad, size_t* bytes);

/* render_rays (RN:390-501) over n_rays rays.  near / far: scalars, overridden per ray by ex->d_near / d_far. */
int nsrw_render_rays(nsrw_handle h, const float* d_rays_o, const float* d_rays_d, int64_t n_rays, float near_, float far_,
                     const NsrwExtras* ex, const NsrwOut* out, void* d_workspace, size_t workspace_bytes, void* stream);

/* The same forward plus d(sum(rgb * grad_rgb)) / d(rays_o, rays_d) (RN:177; weights frozen, z_samples detached RN:475, so
 * an rgb cotangent flows through the LAST pass only): d_grad_o, d_grad_d [N,3]; d_grad_viewdirs [N,3] iff ex->d_viewdirs is
 * given (d_grad_d then holds no view-direction term).  out (nullable) receives the forward's results.
 * = nsrw_render_rays_vjp_cot with {d_rgb = d_grad_rgb} and every other cotangent NULL. */
int nsrw_render_rays_vjp(nsrw_handle h, const float* d_rays_o, const float* d_rays_d, int64_t n_rays, float near_, float far_,
                         const NsrwExtras* ex, const float* d_grad_rgb, const NsrwOut* out, float* d_grad_o, float* d_grad_d,
                         float* d_grad_viewdirs, void* d_workspace, size_t workspace_bytes, void* stream);

/* Cotangents of render_rays' differentiable outputs (RN:488-494; z_std is not one: z_samples is detached, RN:475), all nullable
 * DEVICE pointers: rgb / rgb0 [N,3], disp / acc / disp0 / acc0 [N].  rgb / disp / acc are the LAST pass's; with N_importance = 0
 * that is the coarse pass, and rgb0 / disp0 / acc0 must be NULL.  A NULL cotangent contributes nothing; a given one -- zeros
 * included -- contributes as torch's autograd would, NaN included: a ray with acc == 0 has disp = NaN (RN:381), and a disp
 * cotangent there makes its d_grad_d NaN (through dists |d|, RN:361) while relu's backward keeps its d_grad_o finite. */
typedef struct NsrwCotangents {
  const float* d_rgb;
  const float* d_disp;
  const float* d_acc;
  const float* d_rgb0;
  const float* d_disp0;
  const float* d_acc0;
} NsrwCotangents;

/* The forward plus d(sum over the given outputs of output * cotangent) / d(rays_o, rays_d[, viewdirs]), as
 * nsrw_render_rays_vjp.  A coarse cotangent (N_importance > 0) runs, after the last pass's backward, the coarse network's
 * forward once more with its activations kept, its backward, and adds its share into the same gradients -- the fp32 sum of
 * the two passes' fp32 gradients; the workspace for that is nsrw_workspace_bytes(.., with_grad = 2).  On f16x2 handles those
 * network passes are counted and re-run on bf16x3 like every other (nsrw_range_status). */
int nsrw_render_rays_vjp_cot(nsrw_handle h, const float* d_rays_o, const float* d_rays_d, int64_t n_rays, float near_, float far_,
                             const NsrwExtras* ex, const NsrwCotangents* cot, const NsrwOut* out, float* d_grad_o, float* d_grad_d,
                             float* d_grad_viewdirs, void* d_workspace, size_t workspace_bytes, void* stream);

/* run_network (RN:26-40): d_pts [P,3], d_viewdirs [P,3] (unit length; ignored without view directions) -> d_raw [P, C],
 * C = 4 or output_ch.  Workspace: nsrw_workspace_bytes(h, ceil(P / max(N_samples + N_importance, 1)), 0) suffices. */
int nsrw_run_network(nsrw_handle h, int net_id, const float* d_pts, const float* d_viewdirs, int64_t n_pts, float* d_raw,
                     void* d_workspace, size_t workspace_bytes, void* stream);

/* Stage entries that need no handle (stream-ordered launch calls on `device`; they restore the caller's current device).
 * nsrw_sample_pdf = sample_pdf (RH:199-243) for ANY bin and sample count: d_bins [N, n_bins], d_weights [N, n_bins - 1], the
 * uniforms d_u -- [n_samples] shared by all rows (det=True: the HOST's torch.linspace(0, 1, n_samples), RH:208) or, u_per_row != 0,
 * [N, n_samples] (det=False: the caller's torch.rand, RH:211; the library has no generator) -> d_samples [N, n_samples], d_inds
 * (nullable) int64 [N, n_samples] = searchsorted(cdf, u, right=True) (RH:227).  d_scratch: 2 N (n_bins + 1) floats.  Bit-exact
 * against the reference: torch.sum's association order, fp64-accumulate cdf.
 * nsrw_embed_vjp = the VJP of Embedder.embed (RH:39-48): d_x [P,3], d_grad_out [P, 3 + 6 multires] -> d_grad_x [P,3]. */
int nsrw_sample_pdf(int device, const float* d_bins, const float* d_weights, int64_t n_rows, int n_bins, const float* d_u,
                    int u_per_row, int n_samples, float* d_samples, int64_t* d_inds, float* d_scratch, void* stream);
int nsrw_embed_vjp(int device, const float* d_x, const float* d_grad_out, int64_t n_points, int multires, float* d_grad_x, void* stream);

/* NSRW_FLAG_MLP_F16X2 handles: network passes (forward and backward) launched so far and how many of them were re-run on bf16x3
 * because an activation or a gradient left fp16's range (both 0 for the other arithmetics).  Synchronises the device. */
int nsrw_range_status(nsrw_handle h, unsigned long long* passes, unsigned long long* passes_rerun);

/* NSRW_FLAG_RERUN_ROWS handles: rows (points) of the network passes launched so far and how many of them were flagged and re-computed
 * on bf16x3 (both 0 on every other handle).  Synchronises the device. */
int nsrw_range_rows_status(nsrw_handle h, unsigned long long* rows, unsigned long long* rows_rerun);

/* DIAGNOSTIC; needs no device and no handle.  The host restatement of the list kernel of NSRW_FLAG_RERUN_ROWS: from the row bits
 * `words` (n_words 32-bit words; bit r % 32 of word r / 32 = row r; rows >= M and words behind n_words count as clear) the ascending
 * tile blocks of tile_rows (128 or 256) rows of an M-row pass that hold a flagged row.  Writes the first `max` of them to list_out
 * and returns how many there are; -1 for an argument out of range.  (The device list holds the same blocks in no fixed order.) */
int nsrw_rerun_rows_plan(const uint32_t* words, int64_t n_words, int64_t M, int tile_rows, int32_t* list_out, int64_t max);

/* DIAGNOSTIC stage entry; needs no handle (a stream-ordered launch on `device`).  The list kernel of NSRW_FLAG_RERUN_ROWS on the
 * caller's row bits: d_words [(M + 31) / 32] as above -> d_list [1 + max] int32, which the caller has zeroed at [0]: [0] receives the
 * number of tile blocks of tile_rows rows that hold a flagged row below M, [1 ..] the blocks, in no fixed order; max >= the number of
 * blocks of the pass.  d_range (nullable): 8 zeroed uint32 of which [0] receives (count > 0) and, as two 64-bit counters at [4..7],
 * M and the number of flagged rows are added.  The tests hold it to nsrw_rerun_rows_plan. */
int nsrw_rerun_rows_list(int device, const uint32_t* d_words, int64_t M, int tile_rows, int32_t* d_list, int64_t max, uint32_t* d_range,
                         void* stream);

/* Device time of the last launch call (ms; synchronises on its closing event) and the number of chunks it ran. */
int nsrw_last_ms(nsrw_handle h, float* ms, int* chunks);

/* DIAGNOSTIC; needs no device and no handle.  The launches one layer GEMM is cut into along N: for a matrix packed with
 * n_packed_rows rows (a multiple of 32 in the library's own use; its weight image is padded to an even count of 32-column blocks) of
 * which the caller stores n_stored_columns columns, on a handle whose 256-column tiles have tile_wm = 4 (256 rows, the default) or 2
 * (128 rows: NSRW_B3_WM=2) wave rows.  A part is `tiles` tiles of 64 nj columns from 32-column block col_block on, run by the kernel
 * form <nj, wm>; a part that would start behind the last stored column is not launched and not listed.  Writes the first max_parts
 * parts and returns how many there are (at most 3); -1 for an argument out of range.  The tests hold their own statement of the rule
 * to this one. */
typedef struct NsrwGemmPart {
  int32_t nj, wm, tiles, col_block;
} NsrwGemmPart;
int nsrw_gemm_plan(int n_packed_rows, int n_stored_columns, int tile_wm, NsrwGemmPart* parts_out, int max_parts);

/* DIAGNOSTIC; needs no device and no handle.  NULL when nsrw_create accepts the flag word `flags`, else the words it refuses it with
 * (static storage).  Leaves nsrw_last_error alone. */
const char* nsrw_flags_refusal(int flags);

/* DIAGNOSTIC; needs no device and no handle.  How a handle created with `flags` runs the pts_linears of `net`: onchip = 1
 * -- one kw_trunk_h2<nj> launch over tiles of tile_rows points with lds_bytes of LDS per workgroup -- or onchip = 0 (layer by layer;
 * nj = tile_rows = lds_bytes = 0) with the reason.  nj is the number of 32-column blocks of the output one wave accumulates and
 * tile_rows says how the eight waves share a tile: tile_rows = 128 is 4 wave rows x 2 wave columns, a tile of 64 nj columns (padded
 * width <= 128); tile_rows = 64 is the wide form of NSRW_FLAG_TRUNK_WIDE, 2 wave rows x 4 wave columns, nj = 2, a tile of 256
 * columns (padded width 160 .. 256).  Returns 0, or -1 for an invalid network description (nsrw_last_error says why). */
typedef struct NsrwTrunkPlan {
  int32_t onchip, nj, tile_rows, lds_bytes;
  char reason[64];
} NsrwTrunkPlan;
int nsrw_trunk_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);

/* DIAGNOSTIC; needs no device and no handle.  How a handle created with `flags` runs the input-gradient chain of `net` in its gradient
 * calls: onchip = 1 -- one kw_trunk_bwd_h2<nj> launch over tiles of tile_rows = 128 points with lds_bytes of LDS per
 * workgroup, nj covering the wider of the padded width and the padded encoding (<= 64 columns: 1, else 2) -- or onchip = 0 (a GEMM
 * launch per product; nj = tile_rows = lds_bytes = 0) with the reason.  Returns 0, or -1 for an invalid network description. */
int nsrw_trunk_bwd_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);

/* DIAGNOSTIC; needs no device and no handle.  How a handle created with `flags` runs the f16x2 pass of a forward of `net` that keeps
 * its activations for a backward: onchip = 1 -- one kw_keep_h2<nj, heads> launch over tiles of tile_rows = 128 points
 * with lds_bytes of LDS per workgroup (the trunk's nj and LDS; heads as nsrw_heads_plan decides), the relu masks kept as bits, and
 * the backward launch kw_keep_bwd_h2<nj of nsrw_trunk_bwd_plan> in place of kw_trunk_bwd_h2 -- or onchip = 0 (a GEMM launch per
 * layer, fp32 activations kept; nj = tile_rows = lds_bytes = 0) with the reason.  Returns 0, or -1 for an invalid network description. */
int nsrw_trunk_keep_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);

/* NSRW_FLAG_TRUNK_KEEP handles: kept forward passes launched on chip so far (kw_keep_h2 launches, counted on the host as they are
 * enqueued; 0 on every other handle).  Does not synchronise. */
int nsrw_keep_status(nsrw_handle h, unsigned long long* passes_onchip);

/* DIAGNOSTIC; needs no device and no handle.  How a handle created with `flags` runs the pts_linears of the conditional bf16x3
 * re-run of a forward pass of `net` that keeps no activations: onchip = 1 -- one kw_rerun_b3<nj, wave rows> launch over
 * tiles of tile_rows points with lds_bytes of LDS per workgroup, nj = 1: tile_rows = 128 (4 wave rows x 2 wave columns, padded width
 * <= 64) or 64 (2 x 4, padded width 96 or 128) -- or onchip = 0 (a conditional GEMM launch per layer; nj = tile_rows = lds_bytes = 0)
 * with the reason.  Returns 0, or -1 for an invalid network description. */
int nsrw_trunk_rerun_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out);

/* NSRW_FLAG_TRUNK_RERUN handles: kw_rerun_b3 launches enqueued so far, whether or not their pass left the range (counted on the host as
 * they are enqueued; 0 on every other handle).  Does not synchronise. */
int nsrw_rerun_status(nsrw_handle h, unsigned long long* launches_onchip);

/* DIAGNOSTIC; needs no device and no handle.  Where a handle created with `flags` computes the encodings of a pass of `net`
 * -- kept = 0: a pass that keeps no activations, kept = 1: one that keeps them for a backward -- separately for the positions and for
 * the directions: onchip = 1 -- inside the pass's one f16x2 launch -- or 0 (the kw_embed launch writes them) with the reason.  The
 * positions go on chip with any on-chip form of the pass, the directions with a heads form.  Returns 0, or -1 for an invalid network
 * description. */
typedef struct NsrwEmbedPlan {
  int32_t positions_onchip, directions_onchip;
  char positions_reason[64], directions_reason[64];
} NsrwEmbedPlan;
int nsrw_embed_plan(const NsrwNet* net, int flags, int kept, NsrwEmbedPlan* plan_out);

/* Counted on the host as enqueued, on every handle: passes_onchip network passes whose f16x2 launch computed its position encodings
 * itself (NSRW_FLAG_EMBED_ONCHIP handles; 0 elsewhere), embed_launches unconditional kw_embed launches (whole, or the direction
 * encodings alone), embed_launches_conditional kw_embed launches conditional on the range word in front of a bf16x3 re-run (one per
 * pass counted in passes_onchip).  Does not synchronise. */
int nsrw_embed_status(nsrw_handle h, unsigned long long* passes_onchip, unsigned long long* embed_launches,
                      unsigned long long* embed_launches_conditional);

/* DIAGNOSTIC; needs no device and no handle.  How a handle created with `flags` runs one per-ray stage of a pass with `samples`
 * samples per ray -- N_samples for the coarse pass, N_samples + N_importance for the fine one; NSRW_STAGE_SAMPLE_PDF: N_samples, and
 * n_importance samples to draw (n_importance is read for that stage only).  wave = 0: the thread-per-ray kernel (rays_per_group =
 * lds_bytes = 0) with the reason.  wave = 1 (NSRW_FLAG_STAGES_WAVE): the wave-per-ray kernel, lds_bytes of dynamic LDS per RAY --
 * composite 20 samples, sample_pdf 4 (3 samples + n_importance), composite_bwd 16 samples -- and rays_per_group waves per workgroup,
 * the largest of 4, 2, 1 with rays_per_group * lds_bytes <= 65536.  Returns 0, or -1 for an argument out of range. */
enum { NSRW_STAGE_COMPOSITE = 0, NSRW_STAGE_SAMPLE_PDF = 1, NSRW_STAGE_COMPOSITE_BWD = 2 };
typedef struct { int wave; int rays_per_group; int lds_bytes; char reason[96]; } NsrwStagePlan;
int nsrw_stage_plan(int stage, int samples, int n_importance, int flags, NsrwStagePlan* plan_out);

/* NSRW_FLAG_STAGES_WAVE handles: wave-per-ray stage launches enqueued so far (counted on the host; 0 on every other handle) -- per
 * chunk of rays two or three for a forward (compositing per pass, resampling), one more per pass whose backward runs.  Does not
 * synchronise. */
int nsrw_stages_status(nsrw_handle h, unsigned long long* launches_wave);

/* DIAGNOSTIC; needs no device and no handle.  How a handle created with `flags` runs the heads of `net` behind its pts_linears
 * (DESIGN.md 8): onchip = 1 -- inside the trunk's one launch, kw_trunk_h2<nj, true>, with lds_bytes of LDS per workgroup -- or
 * onchip = 0 (a GEMM launch per head; lds_bytes = 0) with the reason.  Returns 0, or -1 for an invalid network description. */
typedef struct NsrwHeadsPlan {
  int32_t onchip, lds_bytes;
  char reason[64];
} NsrwHeadsPlan;
int nsrw_heads_plan(const NsrwNet* net, int flags, NsrwHeadsPlan* plan_out);

/* libnsr_debug.so (-DNSR_DEBUG_BOUNDS) checks every global / LDS index of this unit's kernels against its extent; a violation is
 * recorded, not trapped.  built_with_checks: 1 in that build, 0 in the product library; first_bad_line: 0 = clean, else the source
 * line of the (highest) failed check -- nsr_wide.hip's line, 100000 + the line of nsr_wide_gemm.inc, or 200000 + the line of
 * nsr_wide_trunk.inc (all forms of kw_trunk_h2, the wide one included, kw_trunk_bwd_h2, kw_keep_h2, kw_keep_bwd_h2 and the two mask
 * kernels), or 300000 + the line of nsr_wide_stages.inc (the three wave-per-ray stage kernels).  Synchronises the device. */
int nsrw_debug_bounds_status(int* built_with_checks, unsigned* first_bad_line);

#ifdef __cplusplus
}
#endif
#endif /* NSR_WIDE_H_ */
