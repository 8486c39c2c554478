// nsr_wide.hip -- the LAYERED renderer (include/nsr_wide.h): render_rays (RN:390-501) and its input-side VJP (RN:168-178) for
// NeRFs (RH:70-122) of any depth / width / skip list and any sample counts, i.e. everything the fused kernels of
// nsr_kernels.hip are not specialised to.  A translation unit of its own (its kernels share nothing with the fused ones but the
// arithmetic they restate), linked into libnsr.so.
//
// Shape of the computation.  The rays of a call are cut into chunks of R rays; per chunk
//   depths -> [encode -> D+3 GEMMs -> composite] (coarse) -> sample_pdf -> sort -> [encode -> GEMMs -> composite] (fine)
// with every activation matrix [points, width] resident in the caller's workspace (HBM), and for the gradient
//   composite_bwd -> the same GEMM kernel on the transposed weights, relu masks read from the stored activations
//   -> encode_bwd + the per-ray reductions.
// The GEMM (nsr_wide_gemm.inc) is fp32 in HBM on both sides and runs on fp16 MFMAs with two-piece operands (f16x2, the default),
// on bf16 MFMAs with three-piece operands (bf16x3) or on fp32 MFMAs (the strict mode): fp32-grade results in every case.  Every K
// and N extent is padded to a multiple of 32 with zero weights, so no kernel carries a K tail; M (points) is arbitrary.
//
// (RN = optimization/utils/run_nerf_noscale.py, RH = optimization/utils/run_nerf_helpers.py of the reference.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nsr_wide.h"

namespace nsrw {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// `make debug` (-DNSR_DEBUG_BOUNDS, libnsr_debug.so): every global / LDS index the kernels of this unit compute is checked against
// the extent it must stay inside; a violation records (file tag + source line) in a device word -- no trap (that would take the
// HSA queue down), the evidence is read back by nsrw_debug_bounds_status().  Release build: nothing.
#ifdef NSR_DEBUG_BOUNDS
__device__ unsigned g_wide_violation = 0u;
#define NSRW_CHECK(cond)                                                                             \
  do {                                                                                               \
    if (!(cond)) atomicMax(&nsrw::g_wide_violation, (unsigned)(NSRW_FILE_TAG + __LINE__));           \
  } while (0)
#else
#define NSRW_CHECK(cond) do { } while (0)
#endif
#define NSRW_FILE_TAG 0            /* nsr_wide.hip: the line itself; nsr_wide_gemm.inc: 100000 + line, nsr_wide_trunk.inc: 200000 + line, nsr_wide_stages.inc: 300000 + line (they set their own tags) */

// ------------------------------------------------------------------------------------------------------------------------
// The encodings (ahead of the on-chip kernels, which compute them too: trunk_rows_encode of nsr_wide_trunk.inc)
// ------------------------------------------------------------------------------------------------------------------------
// gamma(x) (RH:18-48): sin / cos of the fp32 argument a = 2^l x (the scaling is exact) by sincos_enc.  For |a| < 2^24 the result is
// within 2 ulp OF THE TRUE VALUE plus |a| 2^-52: the one-product reduction leaves an absolute |a| 2^-52 radians (2 / pi and the
// product round at 2^-53 each), which is far below an ulp of 1 (3.7e-9 at 2^24) but many ulp of a result near a zero of sin or cos
// -- 4464 ulp of the -3.4e-8 that is cos(267058.94), 1.6e-11 absolute.  (The reference's libm stays within 0.61 ulp of the result
// over the whole argument set of the tests.)  Beyond 2^24: the fp64 library value rounded once, < 1 ulp.  sin / cos of inf / NaN are
// NaN, as in torch.  Held element by element by tests/test_gpu_wide_encodings.py (measured: 0.79 of that bound at worst;
// profiles/r20/extra/encodings.txt).
struct EmbedArgs {
  const float* rays_o; const float* rays_d;   // rays form: point (r, s) = o + d z[r][s]  (RN:463, RN:478)
  const float* z; const float* vd;            // [R,S], [R,3]
  const float* pts; const float* dirs;        // points form (run_network): [P,3] each; used when rays_o == nullptr
  long long P; int S;
  int L, Lv;                                  // frequencies; Lv < 0: no direction encoding
  float* E; int ldE;                          // [P, Ci]; nullptr: the direction encodings alone (the positions are encoded on chip)
  float* ED; int ldED;                        // [P, Cv]
  const unsigned* run_if;                     // nullable: the launch returns at once unless the word is set (the bf16x3 re-run's encodings)
};

// sin and cos of the fp32 argument a for the encodings.  |a| < 2^24 (every scene: 2^14 |x| < 2^24 means |x| < 1024): ONE fp64
// range reduction -- t = a * 2 / pi has >= 24 spare bits, the split into quadrant and fraction is exact -- and the Cephes
// single-precision minimax polynomials on [-pi / 4, pi / 4] (1 ulp of their own value; the result's bound is above), as the fused
// kernels' enc_trig (nsr_kernels.hip); ~30 VALU for the pair where the fp64 library sincos costs several hundred (r06: kw_embed was
// 2-9 % of a layered render).  Beyond that, and for inf / NaN: the fp64 library routine, rounded once, as before.  (In three pieces,
// so that a caller with many columns a lane -- trunk_rows_encode -- can keep the library routine out of its unrolled path:
// sincos_enc itself is what it was.)
__device__ __forceinline__ bool sincos_enc_is_fast(float a) { return fabsf(a) < 16777216.0f; }
__device__ __forceinline__ void sincos_enc_slow(float a, float& s, float& c) {
  double sd, cd;
  sincos((double)a, &sd, &cd);
  s = (float)sd; c = (float)cd;
}
__device__ __forceinline__ void sincos_enc_fast(float a, float& s, float& c) {
  const double kMagic = 6755399441055744.0;                 // 1.5 * 2^52: t + kMagic holds rint(t) in its low word
  const double t = (double)a * 0.63661977236758134308;      // a * 2 / pi
  const double tm = t + kMagic;
  const int n = __double2loint(tm);
  const double f = t - (tm - kMagic);                       // [-0.5, 0.5], exact
  const float r = (float)(f * 1.57079632679489661923);
  const float z = r * r;
  float ps = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
  ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
  ps = __builtin_fmaf(ps * z, r, r);
  float pc = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
  pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
  pc = __builtin_fmaf(pc * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
  const float vs = (n & 1) ? pc : ps, vc = (n & 1) ? ps : pc;              // sin(a) = sin(r + n pi/2), cos(a) = sin(r + (n + 1) pi/2)
  s = __uint_as_float(__float_as_uint(vs) ^ ((unsigned)(n & 2) << 30));
  c = __uint_as_float(__float_as_uint(vc) ^ ((unsigned)((n + 1) & 2) << 30));
}
__device__ __forceinline__ void sincos_enc(float a, float& s, float& c) {
  if (!sincos_enc_is_fast(a)) sincos_enc_slow(a, s, c);
  else sincos_enc_fast(a, s, c);
}

// THE point and THE encoding column, stated once for kw_embed and for trunk_rows_encode (nsr_wide_trunk.inc), whose bits are kw_embed's.
// embed_point: coordinate c of o + d z (RN:463, RN:478) -- a multiplication and an addition (the build has -ffp-contract=off).
__device__ __forceinline__ float embed_point(float o, float d, float z) { return o + d * z; }
// embed_arg: the fp32 argument 2^band x[c] of a band (exact scaling).  embed_band: columns 3 + 6 band + c (the sine) and 6 + 6 band + c
// (the cosine) of the row of x, from its coordinate xc = x[c]: one sincos_enc serves both, which is how kw_embed asks.  embed_col:
// column i of the row of an encoding with L bands, whichever it is -- x[i], one of that pair, or the exact zero of a padding column --
// which is how a lane that owns arbitrary columns asks; trig(a, s, c) is sincos_enc, or a caller's wrapper of its pieces.
__device__ __forceinline__ float embed_arg(float xc, int band) { return xc * ldexpf(1.0f, band); }
__device__ __forceinline__ void embed_band(float xc, int band, float& s, float& c) { sincos_enc(embed_arg(xc, band), s, c); }
template <class Trig>
__device__ __forceinline__ float embed_col(const float (&x)[3], int i, int L, const Trig& trig) {
  if (i >= 3 + 6 * L) return 0.0f;
  if (i < 3) return i == 0 ? x[0] : i == 1 ? x[1] : x[2];
  const int j = i - 3, band = j / 6, w = j - 6 * band, c = w < 3 ? w : w - 3;
  float s, co;
  trig(embed_arg(c == 0 ? x[0] : c == 1 ? x[1] : x[2], band), s, co);
  return w < 3 ? s : co;
}

// ------------------------------------------------------------------------------------------------------------------------
// GEMM: C[m][n] = epi( sum_k A[m][k] * Wt[n][k] + bias[n] ), A = [A1 | A2] (two row-major segments: the skip concatenation
// cat[input_pts, h] RH:105-106 and cat[feature, input_views] RH:113 without materialising them), both K extents multiples of 32.
// ONE kernel body for the three arithmetics (nsr_wide_gemm.inc: gemm_split_body -> kw_gemm_h2 / kw_gemm_b3 / kw_gemm_f32): weights as an
// LDS image moved by LDS-DMA, activations staged through registers, 256 x 256 tiles in 512-thread workgroups, persistent tiles with
// the next tile's first stages in flight, XCD-aware tile order (the N-tiles of one M-block go to ONE XCD back to back: an A tile
// is read from HBM once and then from that XCD's L2).  MFMA operand roles: A-operand = activations, B-operand = weights, so a
// lane's 16 accumulators share ONE output column: bias and relu mask cost one load per 16 values and every store instruction
// writes two full 128-byte rows.  (r05's separate fp32 kernel kw_gemm -- 128 x 128 tiles, XOR-swizzled register-staged LDS tiles --
// was retired in r06: the shared body on fp32 MFMAs is 9-12 % faster, profiles/r06/extra/layered_fp32_ab.txt.)
// ------------------------------------------------------------------------------------------------------------------------
enum { kRelu = 1, kAccum = 2, kMaskEpi = 4 };

#include "nsr_wide_gemm.inc"
#include "nsr_wide_trunk.inc"
#undef NSRW_FILE_TAG
#define NSRW_FILE_TAG 0

// ------------------------------------------------------------------------------------------------------------------------
// per-ray and per-point stages
// ------------------------------------------------------------------------------------------------------------------------
struct RayArgs {                  // one chunk of R rays, first ray = row0 of the call's arrays
  const float* rays_o; const float* rays_d;      // [N,3] (already offset to the chunk)
  const float* viewdirs_in;                      // nullable [N,3] (offset)
  const float* near_in; const float* far_in;     // nullable [N] (offset)
  float near_, far_;
  int R, S0, NI, flags;
  const float* t_tab; const float* u_tab;        // linspace tables
  const float* t_rand; const float* u_rays; const float* noise0; const float* noise1;   // nullable, offset to the chunk
  float* vd; float* nrm; float* z0;              // chunk scratch: [R,3], [R], [R,S0]
};

__device__ __forceinline__ float coarse_z(float near_, float far_, float t, int lindisp) {      // RN:441-443
  if (lindisp) return 1.0f / (((1.0f / near_) * (1.0f - t)) + ((1.0f / far_) * t));
  return (near_ * (1.0f - t)) + (far_ * t);
}

// viewdirs = d / |d| (RN:97-98; torch.norm = sqrt of the sequential fp32 sum of squares), |d| for RN:361, the coarse depths
// (RN:439-443) and their stratified perturbation (RN:447-459).  One thread per ray.
__global__ void __launch_bounds__(256) kw_ray_setup(const RayArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  const float dx = a.rays_d[r * 3 + 0], dy = a.rays_d[r * 3 + 1], dz = a.rays_d[r * 3 + 2];
  const float nrm = sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
  a.nrm[r] = nrm;
  if (a.viewdirs_in) {
    a.vd[r * 3 + 0] = a.viewdirs_in[r * 3 + 0]; a.vd[r * 3 + 1] = a.viewdirs_in[r * 3 + 1]; a.vd[r * 3 + 2] = a.viewdirs_in[r * 3 + 2];
  } else {
    a.vd[r * 3 + 0] = dx / nrm; a.vd[r * 3 + 1] = dy / nrm; a.vd[r * 3 + 2] = dz / nrm;
  }
  const float nr = a.near_in ? a.near_in[r] : a.near_, fr = a.far_in ? a.far_in[r] : a.far_;
  const int lindisp = a.flags & NSRW_FLAG_LINDISP;
  float* z = a.z0 + (long long)r * a.S0;
  if (!a.t_rand) {
    for (int i = 0; i < a.S0; ++i) z[i] = coarse_z(nr, fr, a.t_tab[i], lindisp);
    return;
  }
  const float* tr = a.t_rand + (long long)r * a.S0;
  float prev = coarse_z(nr, fr, a.t_tab[0], lindisp), cur = prev;     // z[i-1], z[i]
  for (int i = 0; i < a.S0; ++i) {
    const float next = i + 1 < a.S0 ? coarse_z(nr, fr, a.t_tab[i + 1], lindisp) : cur;
    const float lower = i > 0 ? 0.5f * (cur + prev) : cur;            // RN:449-450: mids = .5 (z[1:] + z[:-1])
    const float upper = i + 1 < a.S0 ? 0.5f * (next + cur) : cur;
    z[i] = lower + (upper - lower) * tr[i];                           // RN:459
    prev = cur; cur = next;
  }
}

// 16 threads per point, 16 points per workgroup: thread q computes x (q = 0) or band q - 1 (1 <= q <= L) of the position row and the
// same of the direction row into LDS; the workgroup then writes its 16 consecutive rows of E (and of ED) -- one contiguous piece of
// memory -- 16 bytes per thread, padding columns included (r06: the rows used to be written 24 strided bytes per thread, twelve
// dword stores each; the kernel was 4-15 % of a layered render).  E == nullptr: the direction rows alone (a pass whose positions are
// encoded in its on-chip launch); run_if: nothing unless the word is set (the encodings a bf16x3 re-run reads, behind such a pass).
constexpr int kEmbedLdMax = 96;          // pad32(3 + 6 * 15)
__global__ void __launch_bounds__(256) kw_embed(const EmbedArgs a) {
  __shared__ __attribute__((aligned(16))) float sE[16 * kEmbedLdMax];
  __shared__ __attribute__((aligned(16))) float sD[16 * kEmbedLdMax];
  const int tid = threadIdx.x;
  const long long p0 = (long long)blockIdx.x * 16;
  const int lp = tid >> 4, q = tid & 15;
  const long long p = p0 + lp;
  if (a.run_if && !*a.run_if) return;
  const int nE = a.E ? 16 * a.ldE / 4 : 0, nD = a.Lv >= 0 ? 16 * a.ldED / 4 : 0;          // float4s of the workgroup's rows
  for (int t = tid; t < nE; t += 256) reinterpret_cast<f32x4*>(sE)[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = tid; t < nD; t += 256) reinterpret_cast<f32x4*>(sD)[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  __syncthreads();
  if (p < a.P) {
    float x[3], v[3] = {0.0f, 0.0f, 0.0f};
    if (a.rays_o) {
      const long long r = p / a.S;
      const float zz = a.z[p];
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = embed_point(a.rays_o[r * 3 + c], a.rays_d[r * 3 + c], zz);
      if (a.Lv >= 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = a.vd[r * 3 + c];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = a.pts[p * 3 + c];
      if (a.Lv >= 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = a.dirs[p * 3 + c];
    }
    float* e = sE + lp * a.ldE;
    NSRW_CHECK(a.ldE <= kEmbedLdMax && a.ldED <= kEmbedLdMax && 3 + 6 * a.L <= a.ldE && (a.Lv < 0 || a.ED) && (a.E || a.Lv >= 0));
    if (!a.E) {
    } else if (q == 0) {
      e[0] = x[0]; e[1] = x[1]; e[2] = x[2];
    } else if (q <= a.L) {
#pragma unroll
      for (int c = 0; c < 3; ++c) embed_band(x[c], q - 1, e[3 + 6 * (q - 1) + c], e[6 + 6 * (q - 1) + c]);
    }
    if (a.Lv >= 0) {
      float* ed = sD + lp * a.ldED;
      if (q == 0) {
        ed[0] = v[0]; ed[1] = v[1]; ed[2] = v[2];
      } else if (q <= a.Lv) {
#pragma unroll
        for (int c = 0; c < 3; ++c) embed_band(v[c], q - 1, ed[3 + 6 * (q - 1) + c], ed[6 + 6 * (q - 1) + c]);
      }
    }
  }
  __syncthreads();
  const long long rows = a.P - p0 < 16 ? a.P - p0 : 16;
  const int mE = a.E ? (int)(rows * a.ldE / 4) : 0, mD = a.Lv >= 0 ? (int)(rows * a.ldED / 4) : 0;
  f32x4* gE = reinterpret_cast<f32x4*>(a.E + p0 * a.ldE);
  for (int t = tid; t < mE; t += 256) gE[t] = reinterpret_cast<const f32x4*>(sE)[t];
  if (mD) {
    f32x4* gD = reinterpret_cast<f32x4*>(a.ED + p0 * a.ldED);
    for (int t = tid; t < mD; t += 256) gD[t] = reinterpret_cast<const f32x4*>(sD)[t];
  }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float relu_nan(float x) { return (x < 0.0f) ? 0.0f : x; }      // F.relu: a NaN density stays NaN (RN:356)

// raw2outputs (RN:343-387), one thread per ray, the reference's operations in its order: dists (last = 1e10) * |d|, sigmoid,
// alpha = 1 - exp(-relu(sigma + noise) dists), the exclusive transmittance product as torch-CPU's cumprod computes it -- a
// sequential fp64 product, every prefix rounded to fp32 -- weights, the five weighted sums (sequential fp32), disparity with
// its NaN case, white background.
struct CompositeArgs {
  int R, S, flags;
  const float* rgb; int ld_rgb;        // raw rgb logits of point p at rgb[p * ld_rgb + 0..2]
  const float* sigma; int ld_sigma;    // raw density at sigma[p * ld_sigma]
  const float* z; const float* nrm;    // [R,S], [R]
  const float* noise;                  // nullable [R,S]
  float* weights;                      // [R,S]
  float* rgb_map; float* disp; float* acc;       // nullable outputs [R,3], [R], [R]
  float* raw_out; int raw_ch;          // nullable [R,S,raw_ch]: the raw the reference returns with retraw (RN:490-491)
  const float* raw_src; int ld_raw;    // raw_ch channels per point (raw_out given, raw_ch != 4: the output_linear rows)
};

__global__ void __launch_bounds__(256) kw_composite(const CompositeArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  const float* z = a.z + (long long)r * a.S;
  const float nrm = a.nrm[r];
  double T = 1.0;
  float cr = 0.f, cg = 0.f, cb = 0.f, depth = 0.f, acc = 0.f;
  for (int i = 0; i < a.S; ++i) {
    const long long p = (long long)r * a.S + i;
    float dist = (i < a.S - 1) ? (z[i + 1] - z[i]) : 1e10f;               // RN:358-359
    dist = dist * nrm;                                                     // RN:361
    float sg = a.sigma[p * a.ld_sigma];
    if (a.noise) sg = sg + a.noise[p];                                     // RN:374
    const float al = 1.0f - expf(-relu_nan(sg) * dist);                    // RN:356
    const float w = al * (float)T;                                         // RN:376
    T = T * (double)((1.0f - al) + 1e-10f);
    a.weights[p] = w;
    const float* q = a.rgb + p * a.ld_rgb;
    cr = cr + w * sigmoidf_(q[0]);                                         // RN:363, RN:378
    cg = cg + w * sigmoidf_(q[1]);
    cb = cb + w * sigmoidf_(q[2]);
    depth = depth + w * z[i];                                              // RN:380
    acc = acc + w;                                                         // RN:382
    if (a.raw_out) {
      float* o = a.raw_out + p * a.raw_ch;
      if (a.raw_src) { for (int c = 0; c < a.raw_ch; ++c) o[c] = a.raw_src[p * a.ld_raw + c]; }
      else { o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = a.sigma[p * a.ld_sigma]; }
    }
  }
  if (a.rgb_map) {
    const float qd = depth / acc;
    const float disp = (qd != qd) ? qd : 1.0f / fmaxf(1e-10f, qd);         // RN:381: 0/0 -> NaN propagates through torch.max
    if (a.flags & NSRW_FLAG_WHITE_BKGD) {                                   // RN:384-385
      const float bg = 1.0f - acc;
      cr = cr + bg; cg = cg + bg; cb = cb + bg;
    }
    a.rgb_map[r * 3 + 0] = cr; a.rgb_map[r * 3 + 1] = cg; a.rgb_map[r * 3 + 2] = cb;
    a.disp[r] = disp; a.acc[r] = acc;
  }
}

// sample_pdf (RH:199-243) for bins = mid-points of the coarse depths (RN:473) and the coarse weights[1:-1], one thread per ray:
// weights + 1e-5, torch.sum in ATen's association order for a contiguous fp32 row (oracle/nerf_oracle.py:_torch_sum_lastdim
// -- 8 vector lanes x 4 partial vectors, the left-over whole vectors into the first, partials folded 0 += 1, 2, 3, then the
// scalar tail and the 8 lanes in sequence), pdf, the cdf as a sequential fp64 sum rounded per prefix (torch.cumsum on the CPU),
// searchsorted(right=True), the gathers, denom < 1e-5 -> 1, the interpolation.  Also z_std = std(z_samples, unbiased=False)
// (RN:495), fp64 two-pass.
struct PdfArgs {
  int R, S0, NI;
  const float* z0; const float* w0;      // [R,S0] coarse depths and weights
  const float* u_tab; const float* u_rays;      // [NI] table, or nullable [R,NI] draws
  float* pdf; float* cdf;                // scratch [R,S0] each
  float* zs;                             // [R,NI]
  int64_t* inds;                         // nullable [R,NI]
  float* z_std;                          // nullable [R]
  const float* bins;                     // nullable: the stage entry nsrw_sample_pdf -- bins [R,S0-1] GIVEN (z0 unused), w0 = weights [R,S0-2]
};

__global__ void __launch_bounds__(256) kw_sample_pdf(const PdfArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  const int NW = a.S0 - 2, NC = a.S0 - 1;
  const float* z = a.z0 + (long long)r * a.S0;
  const float* w = a.bins ? a.w0 + (long long)r * NW : a.w0 + (long long)r * a.S0 + 1;
  const float* bn = a.bins ? a.bins + (long long)r * NC : nullptr;
  float* x = a.pdf + (long long)r * a.S0;
  float* cdf = a.cdf + (long long)r * a.S0;
  for (int i = 0; i < NW; ++i) x[i] = w[i] + 1e-5f;                        // RH:201
  const int nvec = NW / 8, silp = nvec / 4;
  float ps[4][8];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) ps[k][jj] = 0.0f;
  for (int i = 0; i < silp; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) ps[k][jj] = ps[k][jj] + x[(i * 4 + k) * 8 + jj];
  for (int v = silp * 4; v < nvec; ++v)
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) ps[0][jj] = ps[0][jj] + x[v * 8 + jj];
  float total = 0.0f;
  for (int i = nvec * 8; i < NW; ++i) total = total + x[i];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) total = total + (((ps[0][jj] + ps[1][jj]) + ps[2][jj]) + ps[3][jj]);
  double run = 0.0;
  cdf[0] = 0.0f;
  for (int i = 0; i < NW; ++i) {
    const float pdf = x[i] / total;                                        // RH:202
    run = run + (double)pdf;                                               // RH:203
    cdf[i + 1] = (float)run;
  }
  float* zs = a.zs + (long long)r * a.NI;
  double sum = 0.0;
  for (int k = 0; k < a.NI; ++k) {
    const float u = a.u_rays ? a.u_rays[(long long)r * a.NI + k] : a.u_tab[k];
    int lo = 0, hi = NC;                                                   // RH:227: first index with cdf > u
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
    }
    const int below = max(lo - 1, 0), above = min(lo, NC - 1);             // RH:228-229
    NSRW_CHECK(lo >= 0 && lo <= NC && below >= 0 && above + 1 < a.S0 && below + 1 < a.S0 && NC < a.S0);
    const float c0 = cdf[below], c1 = cdf[above];
    const float b0 = bn ? bn[below] : 0.5f * (z[below + 1] + z[below]);     // RN:473
    const float b1 = bn ? bn[above] : 0.5f * (z[above + 1] + z[above]);
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.0f;                                       // RH:238-239
    const float t = (u - c0) / denom;
    const float s = b0 + t * (b1 - b0);                                    // RH:241
    zs[k] = s;
    sum += (double)s;
    if (a.inds) a.inds[(long long)r * a.NI + k] = (int64_t)lo;
  }
  if (a.z_std) {
    const double mean = sum / a.NI;
    double var = 0.0;
    for (int k = 0; k < a.NI; ++k) { const double d = (double)zs[k] - mean; var += d * d; }
    a.z_std[r] = (float)sqrt(var / a.NI);
  }
}

// z_vals, _ = torch.sort(torch.cat([z_vals, z_samples], -1), -1) (RN:477): one wave per ray, exact and stable for ANY input --
// the rank of an element is the number of elements that sort before it (NaN after every number, ties by position).
__global__ void __launch_bounds__(64) kw_sort(const float* __restrict__ z0, const float* __restrict__ zs, int S0, int NI,
                                              float* __restrict__ zf) {
  extern __shared__ float sz[];
  const long long r = blockIdx.x;
  const int S = S0 + NI, lane = threadIdx.x;
  for (int i = lane; i < S; i += 64) sz[i] = i < S0 ? z0[r * S0 + i] : zs[r * NI + (i - S0)];
  __syncthreads();
  for (int i = lane; i < S; i += 64) {
    const float x = sz[i];
    const bool xn = x != x;
    int rank = 0;
    for (int k = 0; k < S; ++k) {
      const float y = sz[k];
      const bool yn = y != y;
      const bool before = xn ? (!yn || k < i) : (!yn && (y < x || (y == x && k < i)));
      rank += before ? 1 : 0;
    }
    NSRW_CHECK(rank >= 0 && rank < S);
    zf[r * S + rank] = x;
  }
}

// Backward of one pass's raw2outputs for the cotangents of its rgb_map / disp_map / acc_map, one thread per ray, fp32 forward
// quantities recomputed exactly as kw_composite computed them, derivative arithmetic in fp64:
//   w_i = alpha_i T_i, T_k (k > i) carries the factor om_i = 1 - alpha_i + 1e-10 -> dL/dalpha_i = A_i T_i - (sum_{k>i} A_k w_k) / om_i
//   with A_i = dL/dw_i = g . sigmoid(rgb_i) [- sum g with a white background, RN:384-385] + g_acc + dL/d(depth) z_i + dL/d(acc)
//   through disp; alpha = 1 - exp(-relu(sigma) dz |d|).  disp = 1 / max(1e-10, depth / acc) (RN:380-382) is differentiated as
//   torch does it: reciprocal -g disp^2, torch.max's backward (the whole cotangent to the quotient above 1e-10 AND for a NaN
//   quotient, half of it on a tie), then the quotient rule.  A ray with acc == 0 has disp = NaN, so every A_i -- hence dL/dalpha
//   and dL/d|d| -- is NaN, while relu's backward masks the density row to 0 (threshold_backward) exactly as in the reference.
//   Without g_disp / g_acc the arithmetic is the rgb-only one, operation for operation.
// Writes dL/draw [P,32] (rgb logits, sigma, zero padding: the K extent of the first backward GEMM) and dL/d|d| per ray.
struct CompositeBwdArgs {
  int R, S, flags;
  const float* rgb; int ld_rgb; const float* sigma; int ld_sigma;
  const float* z; const float* nrm; const float* noise;
  const float* grad_rgb;              // nullable [R,3]
  const float* grad_disp;             // nullable [R]
  const float* grad_acc;              // nullable [R]
  float* draw;                        // [P,32]
  float* gnorm;                       // [R]
  float* scr_a; float* scr_t;         // scratch [R,S] each: alpha_i, T_i
  float* gscale;                      // nullable [P]: f16x2 handles -- the row leaves NORMALISED, gscale[p] undoes it (kw_embed_bwd)
};

// f16x2 gradient GEMMs (csrc/nsr_h2_bwd.inc has the reasoning): the backward chain is LINEAR in a point's dL/d raw, whose size is
// whatever the cotangent and the compositing weights make it (1e-12 for an occluded sample, 1e+3 for a summed loss) -- no
// upload-time scale can fit it into fp16.  So every point's four inputs are multiplied by s = 2^(7 - floor(log2 max|.|)) (exact),
// the chain runs on gradients of magnitude ~2^7 (2^9 of head-room; a point that outgrows it raises the range flag and the chain is
// re-run on bf16x3), and kw_embed_bwd multiplies what comes out by 1 / s.  0 / denormal-small / inf / NaN rows stay as they are.
__device__ __forceinline__ float grad_norm_scale(float g0, float g1, float g2, float g3, float& inv) {
  const float m = fmaxf(fmaxf(fabsf(g0), fabsf(g1)), fmaxf(fabsf(g2), fabsf(g3)));
  const unsigned ef = (__float_as_uint(m) >> 23) & 0xffu;
  const bool ok = ef >= 8u && ef <= 253u;
  inv = ok ? __uint_as_float((ef - 7u) << 23) : 1.0f;                  // 2^(ef - 127 - 7)
  return ok ? __uint_as_float((254u - ef + 7u) << 23) : 1.0f;          // 2^(127 - ef + 7)
}

__global__ void __launch_bounds__(256) kw_composite_bwd(const CompositeBwdArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.R) return;
  const float* z = a.z + (long long)r * a.S;
  const float nrm = a.nrm[r];
  float* al_s = a.scr_a + (long long)r * a.S;
  float* t_s = a.scr_t + (long long)r * a.S;
  double T = 1.0;
  float depth = 0.f, acc = 0.f;       // the forward's sequential fp32 sums (RN:380, RN:382), for disp only
  for (int i = 0; i < a.S; ++i) {
    const long long p = (long long)r * a.S + i;
    float dist = (i < a.S - 1) ? (z[i + 1] - z[i]) : 1e10f;
    dist = dist * nrm;
    float sg = a.sigma[p * a.ld_sigma];
    if (a.noise) sg = sg + a.noise[p];
    const float al = 1.0f - expf(-relu_nan(sg) * dist);
    al_s[i] = al;
    t_s[i] = (float)T;
    if (a.grad_disp) {
      const float w = al * (float)T;
      depth = depth + w * z[i];
      acc = acc + w;
    }
    T = T * (double)((1.0f - al) + 1e-10f);
  }
  const double g0 = a.grad_rgb ? a.grad_rgb[r * 3 + 0] : 0.0, g1 = a.grad_rgb ? a.grad_rgb[r * 3 + 1] : 0.0,
               g2 = a.grad_rgb ? a.grad_rgb[r * 3 + 2] : 0.0;
  const double gsum = (a.flags & NSRW_FLAG_WHITE_BKGD) ? (g0 + g1 + g2) : 0.0;
  // dL/dw_i beyond the rgb term: g_w + g_z z_i (acc_map and depth_map; disp through depth and acc)
  const bool extra = a.grad_disp || a.grad_acc;
  double g_w = a.grad_acc ? (double)a.grad_acc[r] : 0.0, g_z = 0.0;
  if (a.grad_disp) {
    const float qd = depth / acc;
    const float disp = (qd != qd) ? qd : 1.0f / fmaxf(1e-10f, qd);
    double dq = -(double)a.grad_disp[r] * ((double)disp * (double)disp);       // reciprocal
    if (qd < 1e-10f) dq = 0.0;                                                // torch.max: the clamp binds
    else if (qd == 1e-10f) dq = 0.5 * dq;                                     // ... a tie splits the cotangent
    g_z = dq / (double)acc;
    g_w += -dq * ((double)depth / (double)acc) / (double)acc;
  }
  double suffix = 0.0, dn = 0.0;
  for (int i = a.S - 1; i >= 0; --i) {
    const long long p = (long long)r * a.S + i;
    const float* q = a.rgb + p * a.ld_rgb;
    const double c0 = sigmoidf_(q[0]), c1 = sigmoidf_(q[1]), c2 = sigmoidf_(q[2]);
    const double al = al_s[i], Ti = t_s[i];
    const double w = (double)(al_s[i] * t_s[i]);
    double A = g0 * c0 + g1 * c1 + g2 * c2 - gsum;
    if (extra) A += g_w + g_z * (double)z[i];
    const double om = (double)((1.0f - al_s[i]) + 1e-10f);
    const double d_alpha = A * Ti - suffix / om;
    suffix += A * w;
    float sg = a.sigma[p * a.ld_sigma];
    if (a.noise) sg = sg + a.noise[p];
    const double dz = (i < a.S - 1) ? (double)(z[i + 1] - z[i]) : 1e10;
    const double e = 1.0 - al;
    float* o = a.draw + p * 32;
    float o0 = (float)(w * g0 * c0 * (1.0 - c0));
    float o1 = (float)(w * g1 * c1 * (1.0 - c1));
    float o2 = (float)(w * g2 * c2 * (1.0 - c2));
    float o3 = sg > 0.0f ? (float)(d_alpha * (dz * (double)nrm) * e) : 0.0f;
    if (a.gscale) {
      float inv;
      const float sc = grad_norm_scale(o0, o1, o2, o3, inv);
      o0 *= sc; o1 *= sc; o2 *= sc; o3 *= sc;
      a.gscale[p] = inv;
    }
    o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
    dn += d_alpha * (double)relu_nan(sg) * e * dz;                       // d(dz |d|) / d|d| = dz
  }
  a.gnorm[r] = (float)dn;
}

// the same three stages with one wave per ray (NSRW_FLAG_STAGES_WAVE)
#include "nsr_wide_stages.inc"
#undef NSRW_FILE_TAG
#define NSRW_FILE_TAG 0

__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, mask);
  hi = __shfl_xor(hi, mask);
  return __hiloint2double(hi, lo);
}

// Backward of the encodings and of pts = o + d z (RN:478), viewdirs = d / |d| (RN:97), dists |d| (RN:361), one wave per ray:
// lane l owns samples l, l + 64, ...; fp64 throughout (the per-ray sums run over hundreds of samples of either sign).
struct EmbedBwdArgs {
  int R, S, L, Lv;
  const float* rays_o; const float* rays_d; const float* z; const float* vd; const float* nrm; const float* gnorm;
  const float* GE; int ldE; const float* GED; int ldED;       // dL/d encodings [P, Ci], [P, Cv] (GED nullable)
  int given_viewdirs;
  int accumulate;                                             // 0: write the gradients; 1: add them to what is there (a second pass)
  float* grad_o; float* grad_d; float* grad_v;                // [R,3]; grad_v only with given view directions
  const float* gscale;                                        // nullable [P]: 1 / s of the point's normalised chain (kw_composite_bwd)
};

__device__ __forceinline__ void embed_bwd(const float* G, const double (&x)[3], int L, double (&out)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = (double)G[c];
  for (int l = 0; l < L; ++l) {
    const double f = (double)ldexpf(1.0f, l);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s, co;
      sincos((double)((float)x[c] * (float)f), &s, &co);     // the forward's fp32 argument
      out[c] += f * ((double)G[3 + 6 * l + c] * co - (double)G[6 + 6 * l + c] * s);
    }
  }
}

__global__ void __launch_bounds__(64) kw_embed_bwd(const EmbedBwdArgs a) {
  const long long r = blockIdx.x;
  const int lane = threadIdx.x;
  double o[3], d[3], v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { o[c] = a.rays_o[r * 3 + c]; d[c] = a.rays_d[r * 3 + c]; v[c] = a.vd[r * 3 + c]; }
  double go[3] = {0, 0, 0}, gd[3] = {0, 0, 0}, gv[3] = {0, 0, 0};
  for (int i = lane; i < a.S; i += 64) {
    const long long p = r * a.S + i;
    const float zz = a.z[p];
    double x[3], gp[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = (double)(a.rays_o[r * 3 + c] + a.rays_d[r * 3 + c] * zz);
    embed_bwd(a.GE + p * a.ldE, x, a.L, gp);
    const double un = a.gscale ? (double)a.gscale[p] : 1.0;             // (a power of two: exact)
#pragma unroll
    for (int c = 0; c < 3; ++c) { go[c] += gp[c] * un; gd[c] += gp[c] * un * (double)zz; }
    if (a.GED) {
      double g2[3];
      embed_bwd(a.GED + p * a.ldED, v, a.Lv, g2);
#pragma unroll
      for (int c = 0; c < 3; ++c) gv[c] += g2[c] * un;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      go[c] += shfl_xor_f64(go[c], m); gd[c] += shfl_xor_f64(gd[c], m); gv[c] += shfl_xor_f64(gv[c], m);
    }
  if (lane != 0) return;
  const double nrm = a.nrm[r], gn = a.gnorm[r];
  double u[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) u[c] = d[c] / nrm;                       // d|d| / dd = d / |d|
  float ro[3], rd[3], rv[3] = {0.f, 0.f, 0.f};
  if (a.given_viewdirs) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ro[c] = (float)go[c];
      rd[c] = (float)(gd[c] + gn * u[c]);
      rv[c] = (float)gv[c];
    }
  } else {
    const double dot = gv[0] * u[0] + gv[1] * u[1] + gv[2] * u[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ro[c] = (float)go[c];
      rd[c] = (float)(gd[c] + gn * u[c] + (gv[c] - u[c] * dot) / nrm);      // d(d / |d|)
    }
  }
  // accumulate: the fp32 sum of the two passes' fp32 gradients, as autograd adds the two branches that reach the rays
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a.grad_o[r * 3 + c] = a.accumulate ? a.grad_o[r * 3 + c] + ro[c] : ro[c];
    a.grad_d[r * 3 + c] = a.accumulate ? a.grad_d[r * 3 + c] + rd[c] : rd[c];
    if (a.given_viewdirs && a.grad_v) a.grad_v[r * 3 + c] = a.accumulate ? a.grad_v[r * 3 + c] + rv[c] : rv[c];
  }
}

__global__ void __launch_bounds__(256) kw_copy_rows(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int ld_dst,
                                                    long long rows, int cols) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long p = gid / cols;
  const int c = (int)(gid - p * cols);
  if (p < rows) dst[p * ld_dst + c] = src[p * ld_src + c];
}

// VJP of Embedder.embed (RH:39-48) alone: gx[c] = g[c] + sum_l 2^l (g_sin[l][c] cos(2^l x_c) - g_cos[l][c] sin(2^l x_c)), the
// trigonometric values at the forward's own fp32 arguments, the sum in fp64 rounded once.  One thread per point.
__global__ void __launch_bounds__(256) kw_embed_vjp(const float* __restrict__ x, const float* __restrict__ g, long long P, int L,
                                                    float* __restrict__ gx) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int C = 3 + 6 * L;
  const float* gp = g + p * C;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float xc = x[p * 3 + c];
    double acc = (double)gp[c];
    for (int l = 0; l < L; ++l) {
      const float f = ldexpf(1.0f, l);
      float sn, cs;
      sincos_enc(xc * f, sn, cs);
      acc += (double)f * ((double)gp[3 + 6 * l + c] * (double)cs - (double)gp[6 + 6 * l + c] * (double)sn);
    }
    gx[p * 3 + c] = (float)acc;
  }
}

}  // namespace nsrw

// ------------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------------
namespace {

using namespace nsrw;

thread_local std::string g_err;

int fail(const std::string& m) {
  g_err = m;
  return 1;
}

#define NSRW_HIP(expr)                                                                      \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)

struct DeviceGuard {
  int prev = -1, dev;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int d) : dev(d) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};
#define NSRW_DEVICE(h) DeviceGuard guard_((h)->cfg.device); NSRW_HIP(guard_.err)

inline int pad32(int x) { return (x + 31) / 32 * 32; }

// The arithmetic of a GEMM launch: the pieces per operand, gemm_split_body's NP.  A handle has ONE (nsrw_create); a chain of
// launches runs on one -- an f16x2 handle's on kH2 and then, conditionally, on kB3 (net_forward, net_backward).
enum Arith { kF32 = 1, kH2 = 2, kB3 = 3 };
constexpr Arith kAriths[] = {kF32, kH2, kB3};
constexpr int kArithSlots = 4;                                                    // arrays indexed by an Arith
constexpr int frag_bytes(Arith a) { return a == kB3 ? 3072 : 2048; }              // one (col-block, k16 block) of a weight image
constexpr const char* arith_name(Arith a) { return a == kB3 ? "bf16x3" : a == kH2 ? "f16x2" : "fp32"; }
// the weight images a handle of arithmetic `handle` uploads: its own, and bf16x3 for the re-runs of an f16x2 handle
constexpr bool has_image(Arith handle, Arith a) { return a == handle || (handle == kH2 && a == kB3); }

// col-blocks of the weight image of a matrix with Np packed rows: Np / 32 rounded up to an even count (the padding holds zero weights)
inline int col_blocks(int Np) { return ((Np + 31) / 32 + 1) / 2 * 2; }

struct Mat {                 // one packed matrix [Np][K1p + K2p] and its (nullable) bias
  size_t w = 0;              // offset of the plain fp32 packing in the host vector the images are made from (nsrw_upload_network)
  size_t b = (size_t)-1;     // offset of the bias in Net::dBias
  int Np = 0, K1p = 0, K2p = 0;
  int ncb = 0;               // col_blocks(Np)
  size_t img[kArithSlots] = {};      // per arithmetic: byte offset of the weight image in Net::dImg (pack_image)
  float cscale = 1.0f;       // 2^-sw, which undoes the f16x2 image's weight scale in the epilogue
};

// What a handle runs on chip for one network (onchip_plan): per decision the kernel form that does it -- a row of kTrunkForms -- or
// why there is none.  trunk: the pts_linears in one launch; heads: the heads behind them in that launch (its form replaces the
// trunk's); bwd: the layer loop of the input-gradient chain in one launch; keep: the f16x2 pass of a forward that keeps its
// activations in one launch (with it, keep_bwd: the backward launch that reads the masks as bits instead of bwd's); rerun: the
// pts_linears of the conditional bf16x3 re-run of a forward pass that keeps nothing, in one launch.
struct TrunkForm;
struct Onchip {
  const TrunkForm* form = nullptr;
  const char* why = "";
};
// embed (NSRW_FLAG_EMBED_ONCHIP): which encodings the f16x2 launch of a pass computes itself -- form: the ENC twin of the pass's
// form, which encodes the positions (nullptr: kw_embed writes them, why says why); dirs: it encodes the directions too (the heads
// forms; else kw_embed writes ED alone, why_dirs says why)
struct EmbedOn {
  const TrunkForm* form = nullptr;
  bool dirs = false;
  const char* why = "";
  const char* why_dirs = "";
};
struct OnchipPlan {
  Onchip trunk, heads, bwd, keep, rerun;
  const TrunkForm* keep_bwd = nullptr;
  EmbedOn embed[2];                   // [0]: a pass that keeps nothing (the form of forward()), [1]: a kept pass (keep.form)
  const TrunkForm* forward() const { return heads.form ? heads.form : trunk.form; }      // the form of the forward's launch
};

struct Net {
  NsrwNet d{};
  bool loaded = false;
  int in_ch = 0, in_v = 0, Ci = 0, Cv = 0, Wp = 0, W2 = 0, W2p = 0, ldfa = 0, raw_ch = 4;
  int ldraw = 32;                     // row length of the raw outputs: 4 = [r g b sigma] dense (view directions), else 32
  std::vector<char> skip_in;          // skip_in[i]: layer i takes cat[input_pts, h]  (i - 1 in skips)
  float* dBias = nullptr;             // device: every bias, padded (all the device reads in fp32 form)
  unsigned bias_floats = 0;
  char* dImg[kArithSlots] = {};       // device, per arithmetic the handle has an image of: the weight images of every matrix
  size_t img_bytes[kArithSlots] = {};
  std::vector<Mat> fwd;               // pts_linears
  OnchipPlan onchip;                  // onchip_plan: which kernels of nsr_wide_trunk.inc run this network's passes, if any
  TrunkLayer* dTrunk = nullptr;       // device: trunk_table -- the rows of the forward launch, the backward launch's behind them,
  int trunk_rows = 0, trunk_bwd_rows = 0, trunk_rerun_rows = 0;       // the bf16x3 re-run launch's behind those
  Mat fa, al, hv, rgb, out;           // feature_linear, alpha_linear, views_linears.0, rgb_linear / output_linear
  std::vector<Mat> bwd_h, bwd_e;      // per pts layer: G W_i[:, hidden part] (i >= 1), G W_i[:, encoding part] (layer 0, skip layers)
  Mat b_rgb, b_feat, b_ed, b_head;
};

// every matrix of a network (the unused ones have Np == 0)
template <typename F>
void for_each_mat(Net& n, F f) {
  for (Mat& m : n.fwd) f(m);
  for (Mat& m : n.bwd_h) f(m);
  for (Mat& m : n.bwd_e) f(m);
  for (Mat* m : {&n.fa, &n.al, &n.hv, &n.rgb, &n.out, &n.b_rgb, &n.b_feat, &n.b_ed, &n.b_head}) f(*m);
}

void free_net(Net& n) {      // (the caller has selected the handle's device)
  if (n.dBias) (void)hipFree(n.dBias);
  n.dBias = nullptr;
  if (n.dTrunk) (void)hipFree(n.dTrunk);
  n.dTrunk = nullptr;
  for (Arith a : kAriths) {
    if (n.dImg[a]) (void)hipFree(n.dImg[a]);
    n.dImg[a] = nullptr;
  }
  n.loaded = false;
}

std::string check_net(const NsrwNet& n) {
  char buf[160];
  if (n.D < 1 || n.D > NSRW_MAX_DEPTH) { snprintf(buf, sizeof buf, "netdepth %d (1..%d)", n.D, NSRW_MAX_DEPTH); return buf; }
  if (n.W < 2 || n.W > NSRW_MAX_WIDTH) { snprintf(buf, sizeof buf, "netwidth %d (2..%d)", n.W, NSRW_MAX_WIDTH); return buf; }
  if (n.multires < 0 || n.multires > 15 || n.multires_views < 0 || n.multires_views > 15) return "multires / multires_views (0..15)";
  if (n.n_skips < 0 || n.n_skips > NSRW_MAX_SKIPS) return "more skips than NSRW_MAX_SKIPS";
  for (int i = 0; i < n.n_skips; ++i)
    if (n.skips[i] < 0 || n.skips[i] >= n.D - 1) {
      snprintf(buf, sizeof buf, "skip after layer %d of %d (the reference itself fails on a skip behind the last layer, RH:109)", n.skips[i], n.D);
      return buf;
    }
  if (!n.use_viewdirs && (n.output_ch < 4 || n.output_ch > 32)) return "output_ch (4..32) of a network without view directions";
  return "";
}

bool is_skip(const NsrwNet& n, int i) {
  for (int k = 0; k < n.n_skips; ++k) if (n.skips[k] == i) return true;
  return false;
}

size_t net_floats(const NsrwNet& n) {
  const size_t in_ch = 3 + 6 * n.multires, in_v = 3 + 6 * n.multires_views, W = n.W;
  size_t t = W * in_ch + W;
  for (int i = 1; i < n.D; ++i) t += W * (W + (is_skip(n, i - 1) ? in_ch : 0)) + W;
  if (n.use_viewdirs) t += W * W + W + W + 1 + (W / 2) * (W + in_v) + W / 2 + 3 * (W / 2) + 3;
  else t += (size_t)n.output_ch * W + n.output_ch;
  return t;
}

// How the GEMM kernels are launched: fixed per handle by nsrw_create (a setup call; launch calls read no environment).
struct GemmCfg {
  int cus = 256;                        // compute units of the handle's device
  Arith arith = kF32;                   // NsrwConfig::flags: NSRW_FLAG_MLP_F16X2 -> kH2, NSRW_FLAG_MLP_BF16X3 -> kB3, neither -> kF32
  int tile_wm = 4;                      // 256-column tiles with 256 rows / 512 threads (4) or 128 rows / 256 threads (2: NSRW_B3_WM = 2)
  int flags = 0;                        // NsrwConfig::flags (onchip_plan reads the arithmetic and the seven on-chip flags)
  unsigned long long* keep_passes = nullptr;      // host: kept forward passes launched on chip so far (Handle::keep_passes)
  unsigned long long* rerun_launches = nullptr;   // host: kw_rerun_b3 launches enqueued so far (Handle::rerun_launches)
  unsigned long long* embed_counts = nullptr;     // host: Handle::embed_counts (nsrw_embed_status)
  unsigned* d_range = nullptr;          // device: [0] flag of the f16x2 pass in flight, [1] passes run, [2] passes re-run on bf16x3;
                                        // [4..7] two 64-bit counters of NSRW_FLAG_RERUN_ROWS: rows seen, rows flagged (kw_rows_list)
  bool rows = false;                    // NSRW_FLAG_RERUN_ROWS: the f16x2 passes of net_forward / net_backward re-run per row
};

// The row-granular re-run's buffers of one pass (Chunk::RW / RL, in the workspace): the row bits and, per tile height -- [0]: 128 rows,
// [1]: 256 -- the list of M-blocks with a flagged row ([0] the count) and the entries it has room for.  words == nullptr: not that mode.
struct RowsRun {
  unsigned* words = nullptr;
  int* list[2] = {nullptr, nullptr};
  int list_max[2] = {0, 0};
};

// One chain of GEMM launches (a network pass): the arithmetic it runs on and, nullable, the device word its launches are conditional
// on.  An f16x2 pass is the chain {kH2, nullptr} -- an activation that leaves fp16's range sets d_range[0] -- and then the same chain
// {kB3, d_range}, whose launches return at once unless the flag is set.
struct Run {
  Arith arith;
  const unsigned* run_if;
  RowsRun rows{};                       // NSRW_FLAG_RERUN_ROWS: the kH2 chain sets row bits, the kB3 chain walks the lists (gemm)
};

struct Handle {
  NsrwConfig cfg{};
  GemmCfg gemm_cfg;
  Net net[2];
  float* d_tab = nullptr;           // [n_samples] t, [n_importance] u
  bool tables = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  unsigned* d_range = nullptr;      // GemmCfg::d_range
  bool timed = false;
  int chunks = 0;
  unsigned long long keep_passes = 0;     // nsrw_keep_status
  unsigned long long rerun_launches = 0;  // nsrw_rerun_status
  unsigned long long stage_launches = 0;  // nsrw_stages_status
  unsigned long long embed_counts[3] = {0, 0, 0};      // nsrw_embed_status: passes encoded on chip, kw_embed launches, conditional ones
};

// appends a packed [Np][Kp] matrix to `img`; get(n, k) is consulted for n < rows, k < cols only
template <typename F>
size_t pack(std::vector<float>& img, int Np, int Kp, F get) {
  const size_t off = img.size();
  img.resize(off + (size_t)Np * Kp, 0.0f);
  for (int n = 0; n < Np; ++n)
    for (int k = 0; k < Kp; ++k) img[off + (size_t)n * Kp + k] = get(n, k);
  return off;
}

size_t pack_bias(std::vector<float>& img, int Np, const float* b, int n_real, int at = 0) {
  const size_t off = img.size();
  img.resize(off + Np, 0.0f);
  for (int n = 0; n < n_real; ++n) img[off + at + n] = b[n];
  return off;
}

// fp32 -> nearest-even bf16 (bit pattern); the three round-to-nearest pieces of a weight sum to it exactly
inline uint16_t bf16_rn(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));      // inf / NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_f(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// Appends the weight image of the packed fp32 matrix src [Np][Kp] (Kp a multiple of 16) for arithmetic `a` and returns its byte offset.
// Every image is [col-block][k16 block][frag_bytes(a)] over col_blocks(Np) col-blocks (zero weights behind row Np), and within a block
// lane l <-> (column 32 cb + l % 32, k = 16 kb + 8 (l / 32) + e, e = 0..7): a block IS the LDS image of the B fragments that the
// kernel's LDS-DMA moves.  The arithmetics differ in what they write for one weight, put(block, l, e, w):
//   bf16x3  [piece 3][64 lanes][8 bf16]: the three round-to-nearest bf16 pieces, which sum to w exactly;
//   f16x2   [piece 2][64 lanes][8 fp16]: w 2^sw as two round-to-nearest fp16 pieces -- sw the power of two that puts the matrix's
//           largest |entry| into [2^14, 2^15), 0 for a zero matrix; *cscale = 2^-sw undoes it in the epilogue;
//   fp32    [chunk 2][64 lanes][4 floats]: w itself, k = .. + 4 chunk + 0..3.
template <typename Put>
size_t pack_blocks(std::vector<char>& img, Arith a, const float* src, int Np, int Kp, Put put) {
  const int cbs = col_blocks(Np), KB = Kp / 16, fb = frag_bytes(a);
  const size_t off = img.size();
  img.resize(off + (size_t)cbs * KB * fb, 0);
  for (int cb = 0; cb < cbs; ++cb)
    for (int kb = 0; kb < KB; ++kb) {
      char* blk = img.data() + off + ((size_t)cb * KB + kb) * fb;
      for (int l = 0; l < 64; ++l) {
        const int n = 32 * cb + (l & 31);
        if (n >= Np) continue;
        for (int e = 0; e < 8; ++e) put(blk, l, e, src[(size_t)n * Kp + 16 * kb + 8 * (l >> 5) + e]);
      }
    }
  return off;
}

size_t pack_image(std::vector<char>& img, Arith a, const float* src, int Np, int Kp, float* cscale) {
  auto put16 = [](char* blk, int piece, int l, int e, const void* v) { memcpy(blk + 2 * (piece * 512 + l * 8 + e), v, 2); };
  if (a == kB3)
    return pack_blocks(img, a, src, Np, Kp, [&](char* blk, int l, int e, float w) {
      const uint16_t p0 = bf16_rn(w);
      const float r1 = w - bf16_f(p0);
      const uint16_t p1 = bf16_rn(r1);
      const uint16_t p2 = bf16_rn(r1 - bf16_f(p1));
      put16(blk, 0, l, e, &p0); put16(blk, 1, l, e, &p1); put16(blk, 2, l, e, &p2);
    });
  if (a == kH2) {
    float amax = 0.0f;
    for (size_t i = 0; i < (size_t)Np * Kp; ++i) if (std::isfinite(src[i])) amax = std::max(amax, std::fabs(src[i]));
    int sw = 0;
    if (amax > 0.0f) { int e; (void)std::frexp(amax, &e); sw = 15 - e; }        // amax = f 2^e, f in [0.5, 1): amax 2^sw in [2^14, 2^15)
    sw = std::max(-100, std::min(100, sw));
    const float up = std::ldexp(1.0f, sw);
    *cscale = std::ldexp(1.0f, -sw);
    return pack_blocks(img, a, src, Np, Kp, [&](char* blk, int l, int e, float w0) {
      const float w = w0 * up;                                                   // exact (a non-finite weight stays non-finite)
      const _Float16 p0 = (_Float16)w;
      const _Float16 p1 = (_Float16)(w - (float)p0);
      put16(blk, 0, l, e, &p0); put16(blk, 1, l, e, &p1);
    });
  }
  return pack_blocks(img, a, src, Np, Kp, [](char* blk, int l, int e, float w) { memcpy(blk + 4 * ((e >> 2) * 256 + l * 4 + (e & 3)), &w, 4); });
}

// Chunk workspace: the same carve runs with base = nullptr to size it.
struct Carve {
  char* base; size_t off = 0;
  explicit Carve(void* b) : base(static_cast<char*>(b)) {}
  float* f(size_t n) {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += (n * sizeof(float) + 255) / 256 * 256;
    return p;
  }
};

struct Chunk {
  float *vd, *nrm, *z0, *w0, *zs, *zf, *wf, *pdf, *cdf, *gnorm, *scr_a, *scr_t;
  float *E, *ED, *FA, *HV, *RAW;
  std::vector<float*> H;
  float *DRAW, *GV, *G0, *G1, *GEP, *GED, *gscale;
  unsigned short* MB = nullptr;     // NSRW_FLAG_TRUNK_KEEP, grad >= 1: the relu masks of a kept pass as bits (keep_masks)
  RowsRun rows{};                   // NSRW_FLAG_RERUN_ROWS: the row bits and the two lists of the pass in flight (carve_rows)
};

// the row bits of up to P points and the lists of their 128-row and 256-row blocks, ONE contiguous region from rows.words on (cleared
// as one: rows_bytes) -- behind everything else, and only on a handle with the flag: without it the carve is what it was
size_t rows_bytes(long long P) { return (size_t)((P + 31) / 32 + 2 + (P + 127) / 128 + (P + 255) / 256) * sizeof(unsigned); }
void carve_rows(int flags, long long P, Carve& c, Chunk& k) {
  k.rows = RowsRun{};
  if (!(flags & NSRW_FLAG_RERUN_ROWS) || P <= 0) return;
  unsigned* base = reinterpret_cast<unsigned*>(c.f(rows_bytes(P) / sizeof(unsigned)));
  const long long nw = (P + 31) / 32;
  k.rows.list_max[0] = (int)std::min<long long>((P + 127) / 128, 0x7fffffff);
  k.rows.list_max[1] = (int)std::min<long long>((P + 255) / 256, 0x7fffffff);
  k.rows.words = base;
  if (base) {
    k.rows.list[0] = reinterpret_cast<int*>(base + nw);
    k.rows.list[1] = k.rows.list[0] + 1 + k.rows.list_max[0];
  }
}

// grad: 0 = forward only, 1 = + the last pass's backward (nsrw_render_rays_vjp), 2 = + the coarse pass's backward as well
// (nsrw_render_rays_vjp_cot with coarse cotangents and N_importance > 0: the gradient buffers hold either network)
void carve_chunk(const Handle& h, long long R, int grad, Carve& c, Chunk& k) {
  const int S0 = h.cfg.n_samples, NI = h.cfg.n_importance, S1 = NI > 0 ? S0 + NI : 0;
  const long long Smax = std::max(S0, S1), P = R * Smax;
  const Net& n0 = h.net[0];
  const Net& n1 = (NI > 0 && h.net[1].loaded) ? h.net[1] : h.net[0];
  auto mx = [&](int Net::*f) { return (size_t)std::max(n0.*f, n1.*f); };
  k.vd = c.f(R * 3); k.nrm = c.f(R); k.gnorm = c.f(R);
  k.z0 = c.f(R * S0); k.w0 = c.f(R * S0); k.pdf = c.f(R * S0); k.cdf = c.f(R * S0);
  k.zs = c.f(R * std::max(NI, 1)); k.zf = c.f(R * std::max(S1, 1)); k.wf = c.f(R * std::max(S1, 1));
  k.E = c.f(P * mx(&Net::Ci)); k.ED = c.f(P * mx(&Net::Cv));
  k.FA = c.f(P * mx(&Net::ldfa)); k.HV = c.f(P * mx(&Net::W2p)); k.RAW = c.f(P * 32);
  const Net& last = NI > 0 ? n1 : n0;
  const int nH = grad >= 2 ? std::max(2, std::max(n0.d.D, last.d.D)) : grad ? std::max(2, last.d.D) : 2;
  k.H.resize(nH);
  for (int i = 0; i < nH; ++i) k.H[i] = c.f(P * mx(&Net::Wp));
  if (grad >= 2) {
    const long long Pg = R * (S1 > 0 ? S1 : S0);
    k.scr_a = c.f(Pg); k.scr_t = c.f(Pg); k.gscale = c.f(Pg);
    k.DRAW = c.f(Pg * 32); k.GV = c.f(Pg * mx(&Net::W2p)); k.G0 = c.f(Pg * mx(&Net::Wp)); k.G1 = c.f(Pg * mx(&Net::Wp));
    k.GEP = c.f(Pg * mx(&Net::Ci)); k.GED = c.f(Pg * mx(&Net::Cv));
  } else if (grad) {
    const long long Pg = R * (S1 > 0 ? S1 : S0);
    k.scr_a = c.f(Pg); k.scr_t = c.f(Pg); k.gscale = c.f(Pg);
    k.DRAW = c.f(Pg * 32); k.GV = c.f(Pg * last.W2p); k.G0 = c.f(Pg * last.Wp); k.G1 = c.f(Pg * last.Wp);
    k.GEP = c.f(Pg * last.Ci); k.GED = c.f(Pg * last.Cv);
  } else {
    k.scr_a = k.scr_t = k.DRAW = k.GV = k.G0 = k.G1 = k.GEP = k.GED = k.gscale = nullptr;
  }
  // handles with NSRW_FLAG_TRUNK_KEEP: the masks of a kept on-chip pass, Wp / 8 bytes per point and kept layer over whole blocks of 128
  // points, for the larger of the networks that have the form (behind everything else: without the flag the carve is what it was)
  k.MB = nullptr;
  if (grad && (h.cfg.flags & NSRW_FLAG_TRUNK_KEEP)) {
    size_t words = 0;
    for (const Net* n : {&n0, &n1})
      if (n->onchip.keep.form) words = std::max(words, (size_t)(n->d.D - 1) * (size_t)((P + 127) / 128) * (n->Wp / 32) * 256);
    if (words) k.MB = reinterpret_cast<unsigned short*>(c.f((words + 1) / 2));
  }
  carve_rows(h.cfg.flags, P, c, k);
}

// The launch plan of one GEMM -- pure host arithmetic, no HIP call (nsrw_gemm_plan exposes it).  The N extent of a matrix whose image
// has ncb col-blocks, in units of 64 columns: tiles of 256 where they divide it; else tiles of 192 where THEY do (r06: 384 = 2 x 192 and
// 192 itself are ONE launch -- as 256 + 128 resp. 128 + 64 the second launch read the whole A matrix from HBM again); else 256s and one
// remainder tile of 192, or of 128 and / or 64.  The 192-column form exists with 256-row tiles only (tile_wm == 4); a 64-column
// remainder keeps 128 rows.  The image is padded to an even number of col-blocks with zero weights and columns >= N are never
// stored: a part that starts at or behind column N is not launched.  Returns the number of parts (<= kMaxGemmParts).
constexpr int kMaxGemmParts = 3;
int gemm_plan(int ncb, int N, int tile_wm, NsrwGemmPart* parts) {
  int count = 0, cb = 0;
  auto part = [&](int nj, int tiles) {
    if (N - cb * 32 > 0) parts[count++] = NsrwGemmPart{nj, (nj >= 2 && tile_wm == 4) ? 4 : 2, tiles, cb};
    cb += tiles * nj * 2;
  };
  const int u = ncb / 2;
  const bool three = tile_wm == 4;
  if (u % 4 != 0 && u % 3 == 0 && three) {
    part(3, u / 3);
  } else {
    if (u / 4) part(4, u / 4);
    const int r = u % 4;
    if (r == 3 && three) part(3, 1);
    else {
      if (r >= 2) part(2, 1);
      if (r & 1) part(1, 1);
    }
  }
  return count;
}

// The 72 GEMM kernels, by (arithmetic, tile form <NJ, WM>, epilogue): the forms below are the ones gemm_plan produces.
typedef void (*GemmKernel)(GemmArgs);
struct GemmForm {
  int nj, wm, wgs_per_cu;               // wgs_per_cu: the kernel's own __launch_bounds__ figure
  GemmKernel epi[5];                    // indexed by the epilogue: 0, kRelu, kAccum, (3: none), kMaskEpi
};
template <int NP, int NJ, int EPI, int WM>
GemmKernel gemm_kernel() {
  if constexpr (NP == kB3) return kw_gemm_b3<NJ, EPI, WM>;
  else if constexpr (NP == kH2) return kw_gemm_h2<NJ, EPI, WM>;
  else return kw_gemm_f32<NJ, EPI, WM>;
}
template <int NP, int NJ, int WM>
GemmForm gemm_form() {
  GemmForm f{NJ, WM, wgs_per_cu<NJ, WM>(), {}};
  // (in this order, and f32 / h2 / b3 in find_form: the order of instantiation is the order of the kernels in the code object)
  f.epi[kRelu] = gemm_kernel<NP, NJ, kRelu, WM>();
  f.epi[kMaskEpi] = gemm_kernel<NP, NJ, kMaskEpi, WM>();
  f.epi[kAccum] = gemm_kernel<NP, NJ, kAccum, WM>();
  f.epi[0] = gemm_kernel<NP, NJ, 0, WM>();
  return f;
}
constexpr int kGemmForms = 6;
template <int NP>
const GemmForm* gemm_forms() {
  static const GemmForm forms[kGemmForms] = {gemm_form<NP, 4, 4>(), gemm_form<NP, 3, 4>(), gemm_form<NP, 2, 4>(),
                                             gemm_form<NP, 4, 2>(), gemm_form<NP, 2, 2>(), gemm_form<NP, 1, 2>()};
  return forms;
}
// ... and their row-granular twins (kw_gemm_h2_rows / kw_gemm_b3_rows), a table of its own behind the 72: the same forms, f16x2 and
// bf16x3 only
template <int NP, int NJ, int EPI, int WM>
GemmKernel gemm_rows_kernel() {
  if constexpr (NP == kB3) return kw_gemm_b3_rows<NJ, EPI, WM>;
  else return kw_gemm_h2_rows<NJ, EPI, WM>;
}
template <int NP, int NJ, int WM>
GemmForm gemm_rows_form() {
  GemmForm f{NJ, WM, wgs_per_cu<NJ, WM>(), {}};
  f.epi[kRelu] = gemm_rows_kernel<NP, NJ, kRelu, WM>();
  f.epi[kMaskEpi] = gemm_rows_kernel<NP, NJ, kMaskEpi, WM>();
  f.epi[kAccum] = gemm_rows_kernel<NP, NJ, kAccum, WM>();
  f.epi[0] = gemm_rows_kernel<NP, NJ, 0, WM>();
  return f;
}
template <int NP>
const GemmForm* gemm_rows_forms() {
  static const GemmForm forms[kGemmForms] = {gemm_rows_form<NP, 4, 4>(), gemm_rows_form<NP, 3, 4>(), gemm_rows_form<NP, 2, 4>(),
                                             gemm_rows_form<NP, 4, 2>(), gemm_rows_form<NP, 2, 2>(), gemm_rows_form<NP, 1, 2>()};
  return forms;
}
const GemmForm* find_form(Arith a, int nj, int wm, bool rows = false) {
  if (rows) {
    if (a == kF32) return nullptr;
    const GemmForm* forms = a == kH2 ? gemm_rows_forms<kH2>() : gemm_rows_forms<kB3>();
    for (int i = 0; i < kGemmForms; ++i)
      if (forms[i].nj == nj && forms[i].wm == wm) return &forms[i];
    return nullptr;
  }
  const GemmForm* forms = a == kF32 ? gemm_forms<kF32>() : a == kH2 ? gemm_forms<kH2>() : gemm_forms<kB3>();
  for (int i = 0; i < kGemmForms; ++i)
    if (forms[i].nj == nj && forms[i].wm == wm) return &forms[i];
  return nullptr;
}

// C = epi(A W^T + bias) for one matrix of `net` on the arithmetic of `run`: one launch per part of the plan
int gemm(const GemmCfg& cfg, Run run, hipStream_t st, const Net& net, const Mat& m, const float* A1, int lda1, const float* A2, int lda2,
         float* C, int ldc, int N, long long M, int flags, const float* mask = nullptr, int ldm = 0) {
  if (M <= 0) return 0;
  const int epi = mask ? kMaskEpi : (flags & kAccum) ? kAccum : (flags & kRelu) ? kRelu : 0;     // (never combined: net_*)
  const float* bias = m.b != (size_t)-1 ? net.dBias + m.b : nullptr;
  GemmArgs g{};
  g.A1 = A1; g.A2 = m.K2p ? A2 : nullptr; g.lda1 = lda1; g.lda2 = lda2; g.K1 = m.K1p; g.K2 = m.K2p;
  g.M = M; g.ldc = ldc; g.ldm = ldm;
  g.cscale = run.arith == kH2 ? m.cscale : 1.0f; g.range_flag = cfg.d_range; g.run_if = run.run_if;
  const bool rows = run.rows.words != nullptr;
  if (rows) { g.row_words = run.rows.words; g.n_words = (int)((M + 31) / 32); }
  const int kfrag = frag_bytes(run.arith), KB = (m.K1p + m.K2p) / 16;
  NsrwGemmPart parts[kMaxGemmParts];
  const int n_parts = gemm_plan(m.ncb, N, cfg.tile_wm, parts);
  for (int i = 0; i < n_parts; ++i) {
    const NsrwGemmPart& p = parts[i];
    const GemmForm* form = find_form(run.arith, p.nj, p.wm, rows);
    if (!form) return fail("nsrw: internal error: the launch plan names a tile form that is not compiled");
    const int tm = 64 * p.wm, cb = p.col_block;
    const long long mblocks = (M + tm - 1) / tm, mgroups = (mblocks + 7) / 8;
    GemmArgs t = g;
    const size_t boff = (size_t)cb * KB * kfrag;
    t.Wb = net.dImg[run.arith] + m.img[run.arith] + boff;
    t.wb_bytes = (unsigned)((size_t)m.ncb * KB * kfrag - boff);
    t.bias = bias ? bias + cb * 32 : nullptr;
    t.C = C + cb * 32; t.N = N - cb * 32;
    t.mask = mask ? mask + cb * 32 : nullptr;
    t.n_tiles = p.tiles;
    if (rows) { t.row_list = run.rows.list[p.wm == 4 ? 1 : 0]; t.list_max = run.rows.list_max[p.wm == 4 ? 1 : 0]; }
    const long long all = mgroups * 8 * p.tiles;
    const unsigned grid = (unsigned)std::max<long long>(8, std::min<long long>(all, (long long)cfg.cus * form->wgs_per_cu / 8 * 8));
    hipLaunchKernelGGL(form->epi[epi], dim3(grid), dim3(128 * p.wm), 0, st, t);
  }
  return 0;
}

// The on-chip forms: one row per kernel of nsr_wide_trunk.inc that is instantiated, with the shape it has.  onchip_plan chooses among
// these rows and the launches run the row they are handed: the kernel, its tile rows and its LDS bytes are stated here and nowhere else.
typedef void (*TrunkKernel)(TrunkArgs);
typedef void (*TrunkBwdKernel)(TrunkBwdArgs);
typedef void (*TrunkKeepKernel)(TrunkArgs, TrunkKeepArgs);
typedef void (*TrunkKeepBwdKernel)(TrunkBwdArgs, KeepMasks);
typedef void (*TrunkRerunKernel)(TrunkArgs, const unsigned*);
enum TrunkKind { kFormFwd, kFormBwd, kFormKeep, kFormKeepBwd, kFormRerun };
struct TrunkForm {
  TrunkKind kind;                       // which of the five kernels below the row has
  int nj, tile_rows;                    // 32-column blocks of the output one wave accumulates; points of a block
  bool heads;                           // forward rows: the heads run behind the trunk in the launch
  bool encode;                          // forward and kept rows: the launch computes its encodings from the points (the ENC forms)
  TrunkKernel fwd;                      // kw_trunk_h2, or
  TrunkBwdKernel bwd;                   // kw_trunk_bwd_h2, or
  TrunkKeepKernel keep;                 // kw_keep_h2, or
  TrunkKeepBwdKernel keep_bwd;          // kw_keep_bwd_h2, or
  TrunkRerunKernel rerun;               // kw_rerun_b3: exactly one of the five
  int lds_bytes;                        // the kernel's own (static) LDS
};
template <int NJ, bool HEADS, int WR = 4, bool ENC = false>
TrunkForm trunk_fwd_form() { return {kFormFwd, NJ, trunk_rows<WR>(), HEADS, ENC, ENC ? kw_enc_trunk_h2<NJ, HEADS, WR> : kw_trunk_h2<NJ, HEADS, WR>, nullptr, nullptr, nullptr, nullptr, trunk_lds_bytes<NJ, WR>()}; }
template <int NJ>
TrunkForm trunk_bwd_form_row() { return {kFormBwd, NJ, trunk_rows<4>(), false, false, nullptr, kw_trunk_bwd_h2<NJ>, nullptr, nullptr, nullptr, trunk_bwd_lds_bytes<NJ>()}; }
template <int NJ, bool HEADS, bool ENC = false>
TrunkForm trunk_keep_form() { return {kFormKeep, NJ, trunk_rows<4>(), HEADS, ENC, nullptr, nullptr, ENC ? kw_enc_keep_h2<NJ, HEADS> : kw_keep_h2<NJ, HEADS>, nullptr, nullptr, trunk_lds_bytes<NJ, 4>()}; }
template <int NJ>
TrunkForm trunk_keep_bwd_form() { return {kFormKeepBwd, NJ, trunk_rows<4>(), false, false, nullptr, nullptr, nullptr, kw_keep_bwd_h2<NJ>, nullptr, trunk_bwd_lds_bytes<NJ>()}; }
template <int NJ, int WR>
TrunkForm trunk_rerun_form() { return {kFormRerun, NJ, trunk_rows<WR>(), false, false, nullptr, nullptr, nullptr, nullptr, kw_rerun_b3<NJ, WR>, trunk_lds_bytes<NJ, WR, 3>()}; }
// (in this order: the order of instantiation is the order of the kernels in the code object; the ENC twins of the forward and kept
// forms stand behind everything that was there)
const TrunkForm kTrunkForms[] = {trunk_fwd_form<1, true>(), trunk_fwd_form<2, true>(), trunk_fwd_form<1, false>(), trunk_fwd_form<2, false>(),
                                 trunk_fwd_form<2, false, 2>(), trunk_bwd_form_row<1>(), trunk_bwd_form_row<2>(),
                                 trunk_keep_form<1, true>(), trunk_keep_form<2, true>(), trunk_keep_form<1, false>(), trunk_keep_form<2, false>(),
                                 trunk_keep_bwd_form<1>(), trunk_keep_bwd_form<2>(), trunk_rerun_form<1, 4>(), trunk_rerun_form<1, 2>(),
                                 trunk_fwd_form<1, true, 4, true>(), trunk_fwd_form<2, true, 4, true>(), trunk_fwd_form<1, false, 4, true>(),
                                 trunk_fwd_form<2, false, 4, true>(), trunk_fwd_form<2, false, 2, true>(),
                                 trunk_keep_form<1, true, true>(), trunk_keep_form<2, true, true>(), trunk_keep_form<1, false, true>(),
                                 trunk_keep_form<2, false, true>()};
constexpr int kTrunkThreads = 512;

const TrunkForm* find_trunk_form(TrunkKind kind, int nj, int tile_rows, bool heads, bool encode = false) {
  for (const TrunkForm& f : kTrunkForms)
    if (f.kind == kind && f.nj == nj && f.tile_rows == tile_rows && f.heads == heads && f.encode == encode) return &f;
  return nullptr;
}

// What a handle created with `flags` runs on chip for the network `d` -- pure host arithmetic, no HIP call (nsrw_trunk_plan,
// nsrw_heads_plan, nsrw_trunk_bwd_plan, nsrw_trunk_keep_plan and nsrw_trunk_rerun_plan expose its five decisions; nsrw_upload_network
// keeps it).  DESIGN.md 8 has the table.
//   trunk: an f16x2 handle with NSRW_FLAG_TRUNK_ONCHIP, at least two layers, and a packed width of at most 128, so that the whole N
//     extent is one tile of 128 rows (NJ = 1: <= 64 columns, NJ = 2: 128); with NSRW_FLAG_TRUNK_WIDE on top a packed width of
//     160 .. 256 too: the wide form, tiles of 64 rows by 256 columns.
//   heads: NSRW_FLAG_HEADS_ONCHIP, a trunk on chip in its 128-row form, and, with view directions, a direction encoding that fits
//     the encoding image it takes over.  The kernel's LDS is the trunk's.
//   bwd: NSRW_FLAG_TRUNK_BWD and a trunk on chip in its 128-row form (hence f16x2 and at least two layers: there is a hidden row).
//     NJ covers the wider of the two outputs: the hidden width and the encoding.
//   keep: NSRW_FLAG_TRUNK_KEEP and a backward trunk on chip (hence f16x2, the 128-row forward form and at least two layers).  The
//     forward form the heads decision chooses, with the trunk's NJ and LDS; the backward launch becomes the bit-reading one of bwd's NJ.
//   rerun: NSRW_FLAG_TRUNK_RERUN and a trunk on chip in its 128-row form.  Three bf16 pieces take more LDS than two fp16 ones: a
//     packed width of at most 64 keeps tiles of 128 rows, 96 and 128 take tiles of 64 rows by 128 columns; one column block a wave.
OnchipPlan onchip_plan(const NsrwNet& d, int flags) {
  OnchipPlan p;
  auto decide = [](Onchip& c, const char* why, TrunkKind kind, int nj, int tile_rows, bool heads) {
    if (!why && !(c.form = find_trunk_form(kind, nj, tile_rows, heads))) why = "internal error: form not compiled";
    c.why = why ? why : "";
  };
  if (!check_net(d).empty()) {
    p.trunk.why = p.heads.why = p.bwd.why = p.keep.why = p.rerun.why = "invalid network";
    for (EmbedOn& e : p.embed) e.why = e.why_dirs = "invalid network";
    return p;
  }
  const int Wp = pad32(d.W), Ci = pad32(3 + 6 * d.multires), narrow = trunk_rows<4>();
  const bool wide = (flags & NSRW_FLAG_TRUNK_WIDE) && Wp > 128;
  const int nj = Wp <= 64 ? 1 : 2;
  decide(p.trunk,
         !(flags & NSRW_FLAG_TRUNK_ONCHIP) ? "NSRW_FLAG_TRUNK_ONCHIP not set"
         : !(flags & NSRW_FLAG_MLP_F16X2)  ? "not an f16x2 handle"
         : d.D < 2                         ? "one layer: nothing to keep on chip"
         : wide && Wp > 256                ? "padded width above 256"
         : !wide && Wp > 128               ? "padded width above 128"
         : Ci > kTrunkCiMax                ? "encoding wider than 96"
                                           : nullptr,
         kFormFwd, nj, wide ? trunk_rows<2>() : narrow, false);
  const bool narrow_trunk = p.trunk.form && p.trunk.form->tile_rows == narrow;
  decide(p.heads,
         !(flags & NSRW_FLAG_HEADS_ONCHIP) ? "NSRW_FLAG_HEADS_ONCHIP not set"
         : !p.trunk.form                   ? "the trunk is not on chip"
         : !narrow_trunk                   ? "padded width above 128: the wide trunk has no heads form"
         : d.use_viewdirs && pad32(3 + 6 * d.multires_views) > kTrunkCiMax ? "direction encoding wider than 96"
                                           : nullptr,
         kFormFwd, nj, narrow, true);
  decide(p.bwd,
         !(flags & NSRW_FLAG_TRUNK_BWD) ? "NSRW_FLAG_TRUNK_BWD not set"
         : !p.trunk.form                ? "the trunk is not on chip"
         : !narrow_trunk                ? "padded width above 128: the wide trunk has no backward form"
                                        : nullptr,
         kFormBwd, std::max(nj, Ci <= 64 ? 1 : 2), narrow, false);
  decide(p.keep,
         !(flags & NSRW_FLAG_TRUNK_KEEP) ? "NSRW_FLAG_TRUNK_KEEP not set"
         : !p.bwd.form                   ? "the backward trunk is not on chip"
                                         : nullptr,
         kFormKeep, nj, narrow, p.heads.form != nullptr);
  if (p.keep.form && !(p.keep_bwd = find_trunk_form(kFormKeepBwd, p.bwd.form->nj, narrow, false))) {
    p.keep.form = nullptr;
    p.keep.why = "internal error: form not compiled";
  }
  decide(p.rerun,
         !(flags & NSRW_FLAG_TRUNK_RERUN) ? "NSRW_FLAG_TRUNK_RERUN not set"
         : !p.trunk.form                  ? "the trunk is not on chip"
         : !narrow_trunk                  ? "padded width above 128: the wide trunk has no re-run form"
                                          : nullptr,
         kFormRerun, 1, Wp <= 64 ? trunk_rows<4>() : trunk_rows<2>(), false);
  // embed: per kind of pass, the ENC twin of the form its f16x2 launch has -- it encodes the positions; the directions too where the
  // heads run in that launch (no view directions: there is nothing to encode)
  for (int kept = 0; kept < 2; ++kept) {
    EmbedOn& e = p.embed[kept];
    const TrunkForm* f = kept ? p.keep.form : p.forward();
    const char* no_form = kept ? "the kept forward is not on chip" : "the trunk is not on chip";
    e.why = !(flags & NSRW_FLAG_EMBED_ONCHIP) ? "NSRW_FLAG_EMBED_ONCHIP not set" : !f ? no_form : nullptr;
    if (!e.why && !(e.form = find_trunk_form(f->kind, f->nj, f->tile_rows, f->heads, true))) e.why = "internal error: form not compiled";
    e.why_dirs = e.why ? e.why : !d.use_viewdirs ? "no view directions" : !f->heads ? "the heads are not on chip" : nullptr;
    e.dirs = !e.why_dirs;
    if (!e.why) e.why = "";
    if (!e.why_dirs) e.why_dirs = "";
  }
  return p;
}

// the opt-in flags and what each takes of the rest of the flag word: `needs` (0: nothing) must be set beside it, `excludes` must not.
// The first row that is not met refuses the word (flags_refusal).  wide.KNOBS (neural_sim_nerf_amd/wide.py) states the same
// dependencies for WideModel's arguments; tests/test_wide_options_host.py holds the two to each other on every combination.
struct FlagNeeds {
  int flag, needs, excludes;
  const char* refusal;
};
constexpr FlagNeeds kFlagNeeds[] = {
    {NSRW_FLAG_TRUNK_ONCHIP, NSRW_FLAG_MLP_F16X2, 0,
     "nsrw_create: NSRW_FLAG_TRUNK_ONCHIP needs NSRW_FLAG_MLP_F16X2 (the on-chip trunk exists for the f16x2 arithmetic only)"},
    {NSRW_FLAG_TRUNK_WIDE, NSRW_FLAG_TRUNK_ONCHIP, 0,
     "nsrw_create: NSRW_FLAG_TRUNK_WIDE needs NSRW_FLAG_TRUNK_ONCHIP (it extends the on-chip trunk to padded widths up to 256)"},
    {NSRW_FLAG_HEADS_ONCHIP, NSRW_FLAG_TRUNK_ONCHIP, 0,
     "nsrw_create: NSRW_FLAG_HEADS_ONCHIP needs NSRW_FLAG_TRUNK_ONCHIP (the on-chip heads run behind the on-chip trunk, in its launch)"},
    {NSRW_FLAG_TRUNK_BWD, NSRW_FLAG_TRUNK_ONCHIP, 0,
     "nsrw_create: NSRW_FLAG_TRUNK_BWD needs NSRW_FLAG_TRUNK_ONCHIP (the on-chip backward trunk serves the networks the on-chip trunk serves)"},
    {NSRW_FLAG_TRUNK_KEEP, NSRW_FLAG_TRUNK_BWD, 0,
     "nsrw_create: NSRW_FLAG_TRUNK_KEEP needs NSRW_FLAG_TRUNK_BWD (the kept on-chip forward leaves its relu masks as bits, which only the on-chip backward trunk reads)"},
    {NSRW_FLAG_TRUNK_RERUN, NSRW_FLAG_TRUNK_ONCHIP, 0,
     "nsrw_create: NSRW_FLAG_TRUNK_RERUN needs NSRW_FLAG_TRUNK_ONCHIP (the on-chip bf16x3 re-run serves the passes whose f16x2 trunk ran on chip)"},
    {NSRW_FLAG_EMBED_ONCHIP, NSRW_FLAG_TRUNK_ONCHIP, 0,
     "nsrw_create: NSRW_FLAG_EMBED_ONCHIP needs NSRW_FLAG_TRUNK_ONCHIP (the encodings are computed in the on-chip trunk's launch)"},
    {NSRW_FLAG_RERUN_ROWS, NSRW_FLAG_MLP_F16X2, 0,
     "nsrw_create: NSRW_FLAG_RERUN_ROWS needs NSRW_FLAG_MLP_F16X2 (only the f16x2 arithmetic has a range to leave and a re-run)"},
    {NSRW_FLAG_RERUN_ROWS, 0, NSRW_FLAG_TRUNK_ONCHIP,
     "nsrw_create: NSRW_FLAG_RERUN_ROWS does not combine with NSRW_FLAG_TRUNK_ONCHIP (the on-chip forms feed one range word per pass)"},
};
const char* flags_refusal(int flags) {
  for (const FlagNeeds& r : kFlagNeeds)
    if ((flags & r.flag) && ((r.needs && !(flags & r.needs)) || (flags & r.excludes))) return r.refusal;
  return nullptr;
}

// the decisions as the diagnostic entries report them (no form: every figure 0, and the reason)
NsrwTrunkPlan as_trunk_plan(const Onchip& c) {
  NsrwTrunkPlan p{};
  if (c.form) { p.onchip = 1; p.nj = c.form->nj; p.tile_rows = c.form->tile_rows; p.lds_bytes = c.form->lds_bytes; }
  else snprintf(p.reason, sizeof p.reason, "%s", c.why);
  return p;
}
NsrwHeadsPlan as_heads_plan(const Onchip& c) {
  NsrwHeadsPlan p{};
  if (c.form) { p.onchip = 1; p.lds_bytes = c.form->lds_bytes; }
  else snprintf(p.reason, sizeof p.reason, "%s", c.why);
  return p;
}

// Whether the one launch of form `f` (nullable) runs a pass over P points: the f16x2 pass proper -- the conditional bf16x3 re-run
// stays layer by layer -- over a number of blocks that the grid arithmetic holds.  Its grid: a block per tile, at most one per CU.
bool onchip_pass(Run run, const TrunkForm* f, long long P) {
  return f && run.arith == kH2 && !run.run_if && P > 0 && P / f->tile_rows < 0x7fffffffll;
}
dim3 trunk_grid(const GemmCfg& cfg, const TrunkForm& f, long long P) {
  const long long mblocks = (P + f.tile_rows - 1) / f.tile_rows;
  return dim3((unsigned)std::min<long long>(mblocks, cfg.cus));
}

// The per-row table of the on-chip launches of `n` (Net::dTrunk; launch calls only enqueue): the rows of the forward launch -- the D
// layers, with the heads behind them where n.onchip says so -- then the backward launch's.  Empty when the trunk is not on chip.
std::vector<TrunkLayer> trunk_table_h2(const Net& n, int* fwd_rows, int* bwd_rows) {
  std::vector<TrunkLayer> trunk;
  *fwd_rows = *bwd_rows = 0;
  if (!n.onchip.trunk.form) return trunk;
  const int D = n.d.D, Ci = n.Ci, Wp = n.Wp;
  const bool heads = n.onchip.heads.form != nullptr;
  // a row: the matrix, its K as k16 blocks of the encoding image and of the activation image, and its epilogue
  auto row = [&](const Mat& m, int kbe, int kbh, bool h_first, bool relu, int dest, int ncols = 0, int col0 = 0, int ld = 0) {
    TrunkLayer t{};
    t.img_off = (unsigned)m.img[kH2]; t.bias_off = (unsigned)m.b;
    t.kbe = kbe; t.kbh = kbh;
    t.cscale = m.cscale;
    t.form = trunk_form(m.ncb, m.Np / 32, h_first, relu, dest); t.store = trunk_store(ncols, col0, ld);
    trunk.push_back(t);
  };
  for (int i = 0; i < D; ++i)
    row(n.fwd[i], (i == 0 || n.skip_in[i]) ? Ci / 16 : 0, i == 0 ? 0 : Wp / 16, false, true, (i + 1 < D || heads) ? kTrunkToLds : kTrunkToC);
  if (heads && n.d.use_viewdirs) {                 // net_forward_chain's four head launches, alpha_linear first: it reads the h
    row(n.al, 0, Wp / 16, false, false, kTrunkToRaw, 1, 3, n.ldraw);                 // that feature_linear overwrites
    row(n.fa, 0, Wp / 16, false, false, kTrunkToLds);
    row(n.hv, n.Cv / 16, Wp / 16, true, true, kTrunkToLds);
    row(n.rgb, 0, n.W2p / 16, false, false, kTrunkToRaw, 3, 0, n.ldraw);
  } else if (heads) {
    row(n.out, 0, Wp / 16, false, false, kTrunkToRaw, n.d.output_ch, 0, 32);
  }
  *fwd_rows = (int)trunk.size();
  if (!n.onchip.bwd.form) return trunk;
  // the backward trunk's rows, in the order net_backward_chain issues its launches: per layer i = D - 1 .. 0 the encoding product
  // (layer 0 and the skip layers; every one but the first adds) and, i > 0, the hidden product masked by h_{i-1}
  auto brow = [&](const Mat& m, int dest, bool accum, int mask_layer) {
    TrunkLayer t{};
    t.img_off = (unsigned)m.img[kH2];
    t.kbh = Wp / 16;
    t.cscale = m.cscale;
    t.form = trunk_bwd_form(m.Np / 32, dest, accum); t.store = mask_layer;
    trunk.push_back(t);
  };
  bool first_e = true;
  for (int i = D - 1; i >= 0; --i) {
    if (i == 0 || n.skip_in[i]) {                  // (its mask is the one the hidden row behind it reads: fetched, not used)
      brow(n.bwd_e[i], kTrunkToGep, !first_e, i > 0 ? i - 1 : 0);
      first_e = false;
    }
    if (i > 0) brow(n.bwd_h[i], kTrunkToLds, false, i - 1);
  }
  *bwd_rows = (int)trunk.size() - *fwd_rows;
  return trunk;
}
// ... and behind those rows, so that none of them moves, the bf16x3 re-run launch's (n.onchip.rerun): the forward launch's D
// pts_linears rows once more -- the same K, the same bias -- on the bf16x3 image, without cscale, the last one to C whatever the heads do
std::vector<TrunkLayer> trunk_table(const Net& n, int* fwd_rows, int* bwd_rows, int* rerun_rows) {
  std::vector<TrunkLayer> trunk = trunk_table_h2(n, fwd_rows, bwd_rows);
  *rerun_rows = 0;
  if (!n.onchip.rerun.form) return trunk;
  for (int i = 0; i < n.d.D; ++i) {
    TrunkLayer t = trunk[i];
    t.img_off = (unsigned)n.fwd[i].img[kB3];
    t.cscale = 1.0f;
    t.form = trunk_form(n.fwd[i].ncb, n.fwd[i].Np / 32, false, true, i + 1 < n.d.D ? kTrunkToLds : kTrunkToC);
    trunk.push_back(t);
  }
  *rerun_rows = n.d.D;
  return trunk;
}

// all D pts_linears layers over P points in ONE launch: k.E -> k.H[(D - 1) & 1], where net_forward_chain's layer loop leaves them;
// or (the heads form) the heads too: k.E, k.ED -> k.RAW, where net_forward_chain's head launches leave them
// (src: the pass's points, where the launch computes its encodings itself -- the ENC twin of the form, n.onchip.embed; else nullptr)
TrunkPoints trunk_points(const EmbedArgs& a) { return TrunkPoints{a.rays_o, a.rays_d, a.z, a.vd, a.pts, a.dirs, a.S, a.L, a.Lv}; }
// What the one-launch forwards share of their TrunkArgs: image and bias of `arith`, `rows` rows of the table from `layers` on, the
// network's shape, the P points and their encodings (k.E, or src's points).  A launch adds C and what else is its own.
TrunkArgs trunk_args(const Net& n, const Chunk& k, long long P, int arith, const TrunkLayer* layers, int rows, const EmbedArgs* src) {
  TrunkArgs t{};
  t.E = src ? nullptr : k.E; t.ldE = n.Ci;
  if (src) t.pts = trunk_points(*src);
  t.img = n.dImg[arith]; t.img_bytes = (unsigned)n.img_bytes[arith];
  t.bias = n.dBias; t.bias_floats = n.bias_floats;
  t.layers = layers; t.D = rows; t.Dt = n.d.D;
  t.Wp = n.Wp; t.M = P;
  return t;
}
void trunk_launch(const GemmCfg& cfg, hipStream_t st, const Net& n, const Chunk& k, long long P, const EmbedArgs* src) {
  const TrunkForm& f = src ? *n.onchip.embed[0].form : *n.onchip.forward();
  TrunkArgs t = trunk_args(n, k, P, kH2, n.dTrunk, n.trunk_rows, src);
  t.C = k.H[(n.d.D - 1) & 1];
  t.ED = n.d.use_viewdirs ? k.ED : nullptr; t.ldED = n.Cv;
  t.RAW = k.RAW;
  t.range_flag = cfg.d_range;
  hipLaunchKernelGGL(f.fwd, trunk_grid(cfg, f, P), dim3(kTrunkThreads), 0, st, t);
}

// The pts_linears of the conditional bf16x3 re-run of a pass over P points that keeps nothing, in ONE launch (n.onchip.rerun): k.E ->
// k.H[(D - 1) & 1], where the layer loop of net_forward_chain leaves them for its head launches.  Returns at once unless *run_if is set.
bool rerun_pass(Run run, const Net& n, long long P) {
  const TrunkForm* f = n.onchip.rerun.form;
  return f && run.arith == kB3 && run.run_if && P > 0 && P / f->tile_rows < 0x7fffffffll;
}
void rerun_launch(const GemmCfg& cfg, Run run, hipStream_t st, const Net& n, const Chunk& k, long long P) {
  const TrunkForm& f = *n.onchip.rerun.form;
  TrunkArgs t = trunk_args(n, k, P, kB3, n.dTrunk + n.trunk_rows + n.trunk_bwd_rows, n.trunk_rerun_rows, nullptr);
  t.C = k.H[(n.d.D - 1) & 1];         // (no range_flag: the range word is only read, as run_if)
  hipLaunchKernelGGL(f.rerun, trunk_grid(cfg, f, P), dim3(kTrunkThreads), 0, st, t, run.run_if);
  if (cfg.rerun_launches) ++*cfg.rerun_launches;
}

// The masks of a kept on-chip pass of `n` over P points inside k.MB, in the layout of keep_mask_word (nsr_wide_trunk.inc)
KeepMasks keep_masks(const Net& n, const Chunk& k, long long P) {
  const int nblk = (int)((P + 127) / 128);
  return KeepMasks{k.MB, (long long)nblk * (n.Wp / 32) * 256, nblk, n.d.D - 1};
}

// The f16x2 pass of a forward that KEEPS its activations, in one launch (n.onchip.keep): k.E, k.ED -> the masks of layers 0 .. D - 2
// as bits in k.MB, fp32 k.H[D - 1] -- where the kept per-layer chain leaves it -- and, in the heads form, fp32 k.HV and k.RAW
int keep_launch(const GemmCfg& cfg, hipStream_t st, const Net& n, const Chunk& k, long long P, const EmbedArgs* src) {
  const TrunkForm& f = src ? *n.onchip.embed[1].form : *n.onchip.keep.form;
  if (!k.MB) return fail("nsrw: internal error: a kept on-chip pass without a mask buffer");
  TrunkKeepArgs a{};
  TrunkArgs t = trunk_args(n, k, P, kH2, n.dTrunk, n.trunk_rows, src);
  t.C = k.H[n.d.D - 1];
  t.ED = n.d.use_viewdirs ? k.ED : nullptr; t.ldED = n.Cv;
  t.RAW = k.RAW;
  t.range_flag = cfg.d_range;
  a.HV = k.HV; a.ldHV = n.W2p;
  a.masks = keep_masks(n, k, P);
  hipLaunchKernelGGL(f.keep, trunk_grid(cfg, f, P), dim3(kTrunkThreads), 0, st, t, a);
  if (cfg.keep_passes) ++*cfg.keep_passes;
  return 0;
}

// The kernels that read or write the kept activations k.H[0 .. D - 2] address them as one array of matrices, layer l at k.H[0] +
// l * ldH: carve_chunk lays them out at one stride
int kept_stride(const Net& n, const Chunk& k, long long* ldH) {
  *ldH = k.H[1] - k.H[0];
  for (int i = 0; i + 1 < n.d.D; ++i)
    if (k.H[i] != k.H[0] + i * *ldH) return fail("nsrw: internal error: the kept activations are not equally spaced");
  return 0;
}

// kw_mask_pack / kw_mask_unpack over the masks of a kept pass, conditional on the range flag like the bf16x3 chain's launches
int mask_launch(const GemmCfg& cfg, hipStream_t st, const Net& n, const Chunk& k, long long P, bool pack) {
  long long ldH;
  if (kept_stride(n, k, &ldH)) return 1;
  MaskArgs g{};
  g.H0 = k.H[0]; g.ldH = ldH; g.Wp = n.Wp; g.M = P;
  g.masks = keep_masks(n, k, P);
  g.run_if = cfg.d_range;
  const long long words = g.masks.ld * g.masks.n_layers;
  hipLaunchKernelGGL(pack ? kw_mask_pack : kw_mask_unpack, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, g);
  return 0;
}
// whether the kept passes of `n` over P points run on chip: the forward's f16x2 pass in keep_launch, the backward's reading bits
bool keep_pass(const Net& n, long long P) { return onchip_pass(Run{kH2, nullptr}, n.onchip.keep.form, P); }

// RH:99-122 over P points whose encodings are in k.E / k.ED: leaves the rgb logits in k.RAW (ld 32; all output_linear rows
// without view directions) and the density at sigma / ld_sigma.  keep: every pts layer's activation stays (k.H[i]).
// src: nullptr, or the pass's points where its on-chip launch computes the encodings itself (net_forward decides; f16x2 pass only).
int net_forward_chain(const GemmCfg& cfg, Run run, hipStream_t st, const Net& n, const Chunk& k, long long P, bool keep, const float** sigma,
                      int* ld_sigma, const EmbedArgs* src = nullptr) {
  const float* h = nullptr;
  // f16x2 pass of an eligible network on an on-chip handle: the one trunk launch where no activation is kept, the one kept launch
  // where the network has that form (the conditional bf16x3 re-run and every other pass that keeps its activations for a backward
  // stay layer by layer)
  const bool kept = keep && onchip_pass(run, n.onchip.keep.form, P);
  const bool onchip = kept || (!keep && onchip_pass(run, n.onchip.forward(), P));
  if (onchip) {
    if (kept) { if (keep_launch(cfg, st, n, k, P, src)) return 1; }
    else trunk_launch(cfg, st, n, k, P, src);
    if (n.onchip.heads.form) {        // the heads ran behind the trunk: k.FA is not written (kept: k.H[D - 1], k.HV and the masks are)
      *sigma = k.RAW + 3; *ld_sigma = n.ldraw;
      return 0;
    }
    h = k.H[kept ? n.d.D - 1 : (n.d.D - 1) & 1];
  }
  // the conditional bf16x3 re-run of a pass that keeps nothing, on a network with the re-run form: one launch instead of the layer
  // loop; its heads stay the launches below
  const bool rerun = !keep && rerun_pass(run, n, P);
  if (rerun) {
    rerun_launch(cfg, run, st, n, k, P);
    h = k.H[(n.d.D - 1) & 1];
  }
  for (int i = 0; i < n.d.D && !onchip && !rerun; ++i) {
    float* out = k.H[keep ? i : (i & 1)];
    int rc;
    if (i == 0) rc = gemm(cfg, run, st, n, n.fwd[0], k.E, n.Ci, nullptr, 0, out, n.Wp, n.Wp, P, kRelu);
    else if (n.skip_in[i]) rc = gemm(cfg, run, st, n, n.fwd[i], k.E, n.Ci, h, n.Wp, out, n.Wp, n.Wp, P, kRelu);
    else rc = gemm(cfg, run, st, n, n.fwd[i], h, n.Wp, nullptr, 0, out, n.Wp, n.Wp, P, kRelu);
    if (rc) return rc;
    h = out;
  }
  if (!n.d.use_viewdirs) {
    if (gemm(cfg, run, st, n, n.out, h, n.Wp, nullptr, 0, k.RAW, 32, n.d.output_ch, P, 0)) return 1;
    *sigma = k.RAW + 3; *ld_sigma = 32;
    return 0;
  }
  // the raw outputs of a point are FOUR dense floats [r g b sigma] (r06: rows of 32 with 3 + 1 useful values made every per-ray
  // kernel fetch two 128-byte lines per point): alpha_linear writes column 3, rgb_linear columns 0..2
  if (gemm(cfg, run, st, n, n.fa, h, n.Wp, nullptr, 0, k.FA, n.ldfa, n.ldfa, P, 0)) return 1;
  if (gemm(cfg, run, st, n, n.al, h, n.Wp, nullptr, 0, k.RAW + 3, n.ldraw, 1, P, 0)) return 1;
  if (gemm(cfg, run, st, n, n.hv, k.FA, n.ldfa, k.ED, n.Cv, k.HV, n.W2p, n.W2p, P, kRelu)) return 1;
  if (gemm(cfg, run, st, n, n.rgb, k.HV, n.W2p, nullptr, 0, k.RAW, n.ldraw, 3, P, 0)) return 1;
  *sigma = k.RAW + 3; *ld_sigma = n.ldraw;
  return 0;
}

// the bookkeeping of one f16x2 network pass: counts it, counts its re-run, clears the flag for the next pass
__global__ void kw_range_tally(unsigned* r) {
  if (threadIdx.x == 0) {
    r[1] += 1u;
    if (r[0]) { r[2] += 1u; r[0] = 0u; }
  }
}

// ---- the row-granular re-run (NSRW_FLAG_RERUN_ROWS) between the f16x2 chain and the bf16x3 chain of a pass over M rows.
// kw_rows_list, one thread per M-block of tile_rows rows: a block with a flagged row (bits of rows >= M do not count) appends itself
// to list[1 ..] at the position the wave's one atomicAdd on list[0] hands out -- the blocks of a list stand in no fixed order, which
// no result depends on (a tile's sums do not know its neighbours).  The launch with `tally` set -- one per pass -- also sets
// range[0] = (count > 0), so that every run_if consumer and kw_rows_tally see what the per-pass form would show them, and adds to the two
// 64-bit counters behind range[4]: rows seen, rows flagged.  nsrw_rerun_rows_plan is its host restatement.
struct RowsListArgs {
  const unsigned* words; long long M; int n_words, tile_rows;
  int* list; int list_max;
  unsigned* range; int tally;
};
__global__ void __launch_bounds__(256) kw_rows_list(const RowsListArgs a) {
  const long long mb = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long mblocks = (a.M + a.tile_rows - 1) / a.tile_rows;
  const int wpb = a.tile_rows >> 5, lane = threadIdx.x & 63;
  unsigned n = 0u;
  if (mb < mblocks)
    for (int q = 0; q < wpb; ++q) {
      const long long wi = mb * wpb + q;
      if (wi >= a.n_words) break;
      NSRW_CHECK(wi >= 0 && wi < a.n_words && wi * 32 < a.M);
      unsigned w = a.words[wi];
      const long long left = a.M - wi * 32;
      if (left < 32) w &= (1u << (int)left) - 1u;
      n += (unsigned)__builtin_popcount(w);
    }
  const unsigned long long any = __builtin_amdgcn_ballot_w64(n != 0u);
  if (any == 0ull) {
    if (a.tally && mb == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.range + 4), (unsigned long long)a.M);
    return;
  }
  const int leader = __builtin_ctzll(any);
  int base = 0;
  if (lane == leader) base = atomicAdd(a.list, __builtin_popcountll(any));
  base = __shfl(base, leader, 64);
  if (n != 0u) {
    const int pos = base + __builtin_popcountll(any & ((1ull << lane) - 1ull));
    NSRW_CHECK(pos >= 0 && pos < a.list_max && mb * a.tile_rows < a.M);
    if (pos < a.list_max) a.list[1 + pos] = (int)mb;
  }
  if (a.tally) {
    unsigned sum = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == leader) {
      atomicAdd(reinterpret_cast<unsigned long long*>(a.range + 4) + 1, (unsigned long long)sum);
      atomicOr(a.range, 1u);
    }
    if (mb == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.range + 4), (unsigned long long)a.M);
  }
}

// kw_range_tally's sibling behind such a pass: the same bookkeeping, and the row words and both list counts cleared for the next pass
__global__ void __launch_bounds__(256) kw_rows_tally(unsigned* r, unsigned* words, int n_words, int* count128, int* count256) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n_words) words[i] = 0u;
  if (i == 0) {
    r[1] += 1u;
    if (r[0]) { r[2] += 1u; r[0] = 0u; }
    *count128 = 0;
    *count256 = 0;
  }
}

RowsListArgs rows_list_args(const GemmCfg& cfg, const RowsRun& rr, long long M, int which) {
  RowsListArgs a{};
  a.words = rr.words; a.M = M; a.n_words = (int)((M + 31) / 32); a.tile_rows = which ? 256 : 128;
  a.list = rr.list[which]; a.list_max = rr.list_max[which];
  a.range = cfg.d_range; a.tally = which == 0;
  return a;
}
// the two lists of a pass over M rows (the 128-row one serves the 64-column forms on every handle, and every form under NSRW_B3_WM = 2)
void rows_list_launch(const GemmCfg& cfg, hipStream_t st, const RowsRun& rr, long long M) {
  for (int which = 0; which < 2; ++which) {
    const RowsListArgs a = rows_list_args(cfg, rr, M, which);
    const long long mblocks = (M + a.tile_rows - 1) / a.tile_rows;
    hipLaunchKernelGGL(kw_rows_list, dim3((unsigned)((mblocks + 255) / 256)), dim3(256), 0, st, a);
  }
}
void rows_tally_launch(const GemmCfg& cfg, hipStream_t st, const RowsRun& rr, long long M) {
  const int n_words = (int)((M + 31) / 32);
  hipLaunchKernelGGL(kw_rows_tally, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, cfg.d_range, rr.words, n_words, rr.list[0], rr.list[1]);
}

// kw_embed over the points of `src` (EmbedArgs::E / ED are set here): E nullable -- the direction rows alone; run_if nullable
void embed_launch(const GemmCfg& cfg, hipStream_t st, EmbedArgs a, float* E, float* ED, const unsigned* run_if) {
  a.E = E; a.ED = ED; a.run_if = run_if;
  if (!ED) a.Lv = -1;                 // the position rows alone: kw_embed takes Lv >= 0 as "write ED"
  hipLaunchKernelGGL(kw_embed, dim3((unsigned)((a.P * 16 + 255) / 256)), dim3(256), 0, st, a);
  if (cfg.embed_counts) ++cfg.embed_counts[run_if ? 2 : 1];
}

// One network pass over the P points of `src` (EmbedArgs without E / ED: where the points come from, the bands, the row lengths): the
// encodings, then the chain.  On a handle with NSRW_FLAG_EMBED_ONCHIP the f16x2 launch of a pass that runs on chip computes the
// position encodings itself (n.onchip.embed; the direction encodings too in a heads form, else kw_embed writes k.ED alone), and
// kw_embed for k.E (and k.ED) stands conditional on the range word in front of the bf16x3 chain, which reads them from memory.
int net_forward(const GemmCfg& cfg, hipStream_t st, const Net& n, const Chunk& k, const EmbedArgs& src, long long P, bool keep,
                const float** sigma, int* ld_sigma) {
  if (P <= 0) return net_forward_chain(cfg, Run{cfg.arith, nullptr}, st, n, k, P, keep, sigma, ld_sigma);
  const EmbedOn& eo = n.onchip.embed[keep ? 1 : 0];
  // (the conditions under which net_forward_chain's f16x2 pass is the one launch of the form eo.form is the twin of)
  const bool enc = cfg.arith == kH2 && eo.form && onchip_pass(Run{kH2, nullptr}, keep ? n.onchip.keep.form : n.onchip.forward(), P);
  float* ED = src.Lv >= 0 ? k.ED : nullptr;
  if (!enc) embed_launch(cfg, st, src, k.E, ED, nullptr);
  else if (ED && !eo.dirs) embed_launch(cfg, st, src, nullptr, ED, nullptr);
  if (cfg.arith != kH2) return net_forward_chain(cfg, Run{cfg.arith, nullptr}, st, n, k, P, keep, sigma, ld_sigma);
  // f16x2: the pass on fp16 MFMAs; then the same pass on bf16x3 in launches that are empty unless an activation left fp16's
  // range (its inputs -- the encodings -- are untouched, every buffer it writes is written again); then the tally
  if (cfg.rows) {
    // row-granular: the f16x2 chain sets a bit per row that leaves the range, the lists name the blocks that hold one, and the bf16x3
    // chain stores those rows alone (every launch of it reads its count on the device: nothing listed, nothing done)
    if (net_forward_chain(cfg, Run{kH2, nullptr, k.rows}, st, n, k, P, keep, sigma, ld_sigma)) return 1;
    rows_list_launch(cfg, st, k.rows, P);
    if (net_forward_chain(cfg, Run{kB3, cfg.d_range, k.rows}, st, n, k, P, keep, sigma, ld_sigma)) return 1;
    rows_tally_launch(cfg, st, k.rows, P);
    return 0;
  }
  if (net_forward_chain(cfg, Run{kH2, nullptr}, st, n, k, P, keep, sigma, ld_sigma, enc ? &src : nullptr)) return 1;
  if (enc) {
    embed_launch(cfg, st, src, k.E, eo.dirs ? ED : nullptr, cfg.d_range);
    if (cfg.embed_counts) ++cfg.embed_counts[0];
  }
  if (net_forward_chain(cfg, Run{kB3, cfg.d_range}, st, n, k, P, keep, sigma, ld_sigma)) return 1;
  // a kept on-chip pass that was re-run: the re-run has rewritten every fp32 H, the backward reads bits
  if (keep && keep_pass(n, P) && mask_launch(cfg, st, n, k, P, true)) return 1;
  hipLaunchKernelGGL(kw_range_tally, dim3(1), dim3(64), 0, st, cfg.d_range);
  return 0;
}

// net_backward_chain's layer loop over P points in ONE launch: k.G0 (what b_head left there) and the kept k.H[0 .. D - 2] -> k.GEP
int trunk_bwd_launch(const GemmCfg& cfg, hipStream_t st, const Net& n, const Chunk& k, long long P) {
  const int D = n.d.D;
  const TrunkForm& f = *n.onchip.bwd.form;
  long long ldH;
  if (kept_stride(n, k, &ldH)) return 1;
  TrunkBwdArgs t{};
  t.G = k.G0; t.Wp = n.Wp;
  t.img = n.dImg[kH2]; t.img_bytes = (unsigned)n.img_bytes[kH2];
  t.rows = n.dTrunk + n.trunk_rows; t.R = n.trunk_bwd_rows;
  t.H0 = k.H[0]; t.ldH = ldH; t.n_masks = D - 1;
  t.GEP = k.GEP; t.Ci = n.Ci;
  t.M = P;
  t.range_flag = cfg.d_range;
  if (n.onchip.keep.form) {           // the forward was kept on chip: the masks are bits (k.H[0 .. D - 2] is not read)
    hipLaunchKernelGGL(n.onchip.keep_bwd->keep_bwd, trunk_grid(cfg, *n.onchip.keep_bwd, P), dim3(kTrunkThreads), 0, st, t, keep_masks(n, k, P));
    return 0;
  }
  hipLaunchKernelGGL(f.bwd, trunk_grid(cfg, f, P), dim3(kTrunkThreads), 0, st, t);
  return 0;
}

// Input-side backward of net_forward (activations kept): k.DRAW [P,32] = dL/d(rgb logits, sigma) -> k.GEP [P,Ci], k.GED [P,Cv].
int net_backward_chain(const GemmCfg& cfg, Run run, hipStream_t st, const Net& n, const Chunk& k, long long P) {
  float* g = k.G0;
  float* g2 = k.G1;
  const int D = n.d.D;
  if (n.d.use_viewdirs) {
    if (gemm(cfg, run, st, n, n.b_rgb, k.DRAW, 32, nullptr, 0, k.GV, n.W2p, n.W2p, P, 0, k.HV, n.W2p)) return 1;   // (g W_rgb) relu'(views)
    if (gemm(cfg, run, st, n, n.b_feat, k.GV, n.W2p, nullptr, 0, g2, n.Wp, n.Wp, P, 0)) return 1;                  // dL/d feature
    if (gemm(cfg, run, st, n, n.b_ed, k.GV, n.W2p, nullptr, 0, k.GED, n.Cv, n.Cv, P, 0)) return 1;                 // dL/d direction encoding
    if (gemm(cfg, run, st, n, n.b_head, g2, n.Wp, k.DRAW, 32, g, n.Wp, n.Wp, P, 0, k.H[D - 1], n.Wp)) return 1;    // feature, alpha -> h_{D-1}
  } else {
    if (gemm(cfg, run, st, n, n.b_head, k.DRAW, 32, nullptr, 0, g, n.Wp, n.Wp, P, 0, k.H[D - 1], n.Wp)) return 1;
  }
  // f16x2 pass of a network whose backward trunk is on chip: the one launch instead of the layer loop
  if (onchip_pass(run, n.onchip.bwd.form, P)) return trunk_bwd_launch(cfg, st, n, k, P);
  bool first_e = true;
  for (int i = D - 1; i >= 0; --i) {          // g = dL/d pre-activation of layer i
    if (i == 0 || n.skip_in[i]) {
      if (gemm(cfg, run, st, n, n.bwd_e[i], g, n.Wp, nullptr, 0, k.GEP, n.Ci, n.Ci, P, first_e ? 0 : kAccum)) return 1;
      first_e = false;
    }
    if (i > 0) {
      if (gemm(cfg, run, st, n, n.bwd_h[i], g, n.Wp, nullptr, 0, g2, n.Wp, n.Wp, P, 0, k.H[i - 1], n.Wp)) return 1;
      std::swap(g, g2);
    }
  }
  return 0;
}

// f16x2: the chain on fp16 MFMAs over the per-point NORMALISED gradients (kw_composite_bwd), then -- in launches that are empty
// unless a gradient left fp16's range -- once more on bf16x3 from the same inputs (k.DRAW and the stored activations are read
// only; the first write of k.GEP does not accumulate), then the tally
int net_backward(const GemmCfg& cfg, hipStream_t st, const Net& n, const Chunk& k, long long P) {
  if (cfg.arith != kH2 || P <= 0) return net_backward_chain(cfg, Run{cfg.arith, nullptr}, st, n, k, P);
  if (cfg.rows) {                     // row-granular, as in net_forward: the bits are this backward's own (the tally cleared the forward's)
    if (net_backward_chain(cfg, Run{kH2, nullptr, k.rows}, st, n, k, P)) return 1;
    rows_list_launch(cfg, st, k.rows, P);
    if (net_backward_chain(cfg, Run{kB3, cfg.d_range, k.rows}, st, n, k, P)) return 1;
    rows_tally_launch(cfg, st, k.rows, P);
    return 0;
  }
  if (net_backward_chain(cfg, Run{kH2, nullptr}, st, n, k, P)) return 1;
  // a forward kept on chip left bits: the re-run masks by fp32 H > 0, so H[0 .. D - 2] = 1 / 0 from the bits first
  if (keep_pass(n, P) && mask_launch(cfg, st, n, k, P, false)) return 1;
  if (net_backward_chain(cfg, Run{kB3, cfg.d_range}, st, n, k, P)) return 1;
  hipLaunchKernelGGL(kw_range_tally, dim3(1), dim3(64), 0, st, cfg.d_range);
  return 0;
}

// How a handle created with `flags` runs one per-ray stage of a pass with `samples` samples per ray (SAMPLE_PDF: the coarse pass's,
// and n_importance samples to draw) -- pure host arithmetic, no HIP call (nsrw_stage_plan exposes it).  Without
// NSRW_FLAG_STAGES_WAVE: the thread-per-ray kernel.  With it: the wave-per-ray kernel of nsr_wide_stages.inc, the LDS one ray takes
// there (stage_lds_*), and as many rays per workgroup -- 4, 2 or 1 -- as 64 KiB hold; a ray that does not fit stays on the thread
// kernel.  ("Per-ray stages".)
NsrwStagePlan stage_plan(int stage, int samples, int n_importance, int flags) {
  NsrwStagePlan p{};
  auto thread_form = [&](const char* why) { p = NsrwStagePlan{}; snprintf(p.reason, sizeof p.reason, "%s", why); };
  if (!(flags & NSRW_FLAG_STAGES_WAVE)) { thread_form("NSRW_FLAG_STAGES_WAVE not set"); return p; }
  const long long lds = stage == NSRW_STAGE_COMPOSITE    ? (long long)stage_lds_composite(samples)
                        : stage == NSRW_STAGE_SAMPLE_PDF ? (long long)stage_lds_sample_pdf(samples, n_importance)
                                                         : (long long)stage_lds_composite_bwd(samples);
  for (int rays : {4, 2, 1})
    if (lds * rays <= kStageLdsMax) {
      p.wave = 1; p.rays_per_group = rays; p.lds_bytes = (int)lds;
      return p;
    }
  thread_form("one ray's samples do not fit 64 KiB of LDS");
  return p;
}

// One stage launch over Rc rays: the kernel, the grid and the LDS from the plan
template <typename Args>
void stage_launch(Handle* h, int stage, void (*threads)(Args), void (*wave)(Args), const Args& args, int Rc, int samples, hipStream_t st) {
  const NsrwStagePlan p = stage_plan(stage, samples, h->cfg.n_importance, h->cfg.flags);
  if (!p.wave) {
    hipLaunchKernelGGL(threads, dim3((unsigned)((Rc + 255) / 256)), dim3(256), 0, st, args);
    return;
  }
  const int rpg = p.rays_per_group;
  hipLaunchKernelGGL(wave, dim3((unsigned)((Rc + rpg - 1) / rpg)), dim3(64 * rpg), (size_t)p.lds_bytes * rpg, st, args);
  ++h->stage_launches;
}

// the timing events are skipped while the stream is being captured into a hipGraph (an event recorded under capture cannot be
// waited on by nsrw_last_ms); everything else a launch call does -- kernels, memset / memcpy nodes -- is capturable
bool capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

int check_common(Handle* h, const float* ro, const float* rd, long long n, const NsrwExtras* ex) {
  if (!h) return fail("nsrw: null handle");
  if (n < 0) return fail("nsrw: n_rays < 0");
  if (n > 0 && (!ro || !rd)) return fail("nsrw: null rays");
  if (!h->net[0].loaded) return fail("nsrw: network 0 not uploaded");
  if (!h->tables) return fail("nsrw: nsrw_upload_tables not called");
  if (ex && (ex->d_u || ex->d_z_fine) && h->cfg.n_importance == 0) return fail("nsrw: u draws / fine depths without N_importance");
  return 0;
}

long long chunk_rays(Handle* h, size_t bytes, int grad, long long n) {
  // largest R (multiple of 64, <= n rounded up) whose chunk fits `bytes`; 0 if not even 64 rays fit
  auto need = [&](long long R) { Carve c(nullptr); Chunk k; carve_chunk(*h, R, grad, c, k); return c.off; };
  if (need(64) > bytes) return 0;
  long long lo = 64, hi = std::max<long long>(64, (n + 63) / 64 * 64);
  if (need(hi) <= bytes) return hi;
  while (hi - lo > 64) {
    const long long mid = (lo + hi) / 2 / 64 * 64;
    if (need(mid) <= bytes) lo = mid; else hi = mid;
  }
  return lo;
}

int render_impl(Handle* h, const float* ro, const float* rd, long long n, float near_, float far_, const NsrwExtras* ex,
                const NsrwCotangents* cot, const NsrwOut* out, float* grad_o, float* grad_d, float* grad_v, void* ws,
                size_t ws_bytes, hipStream_t st) {
  const int S0 = h->cfg.n_samples, NI = h->cfg.n_importance, S1 = NI > 0 ? S0 + NI : 0, SL = NI > 0 ? S1 : S0;
  // the last pass's backward runs for a cotangent on rgb / disp / acc, the coarse pass's (N_importance > 0) for one on
  // rgb0 / disp0 / acc0 -- after the last pass's, into the same gradients; no cotangent at all: zero gradients
  const bool grad_last = cot && (cot->d_rgb || cot->d_disp || cot->d_acc);
  const bool grad_c = cot && NI > 0 && (cot->d_rgb0 || cot->d_disp0 || cot->d_acc0);
  const bool grad = grad_last || grad_c;
  const int mode = grad_c ? 2 : grad ? 1 : 0;
  const Net& n0 = h->net[0];
  const Net& n1 = (NI > 0 && h->net[1].loaded) ? h->net[1] : h->net[0];
  const Net& last = NI > 0 ? n1 : n0;
  NsrwExtras e{};
  if (ex) e = *ex;
  NsrwOut o{};
  if (out) o = *out;
  if (n == 0) return 0;
  if (!ws) return fail("nsrw: null workspace");
  if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return fail("nsrw: workspace must be 256-byte aligned");
  const long long R = chunk_rays(h, ws_bytes, mode, n);
  if (R == 0) return fail("nsrw: workspace too small for a chunk of 64 rays (nsrw_workspace_bytes)");
  if ((size_t)S1 * sizeof(float) > 64 * 1024) return fail("nsrw: too many samples per ray for the sort kernel");
  h->chunks = 0;
  const bool cap = capturing(st);
  if (!cap) NSRW_HIP(hipEventRecord(h->ev0, st));
  for (long long r0 = 0; r0 < n; r0 += R) {
    const int Rc = (int)std::min<long long>(R, n - r0);
    Carve c(ws);
    Chunk k;
    carve_chunk(*h, R, mode, c, k);
    if (c.off > ws_bytes) return fail("nsrw: internal error: the chunk's carve exceeds the workspace");      // (chunk_rays sized it)
    // (the workspace is the caller's memory: whatever it holds, the first pass starts from clear bits and empty lists; kw_rows_tally keeps them so)
    if (k.rows.words) NSRW_HIP(hipMemsetAsync(k.rows.words, 0, rows_bytes(R * std::max(S0, S1)), st));
    const unsigned rb = (Rc + 255) / 256;
    RayArgs ra{};
    ra.rays_o = ro + r0 * 3; ra.rays_d = rd + r0 * 3;
    ra.viewdirs_in = e.d_viewdirs ? e.d_viewdirs + r0 * 3 : nullptr;
    ra.near_in = e.d_near ? e.d_near + r0 : nullptr; ra.far_in = e.d_far ? e.d_far + r0 : nullptr;
    ra.near_ = near_; ra.far_ = far_; ra.R = Rc; ra.S0 = S0; ra.NI = NI; ra.flags = h->cfg.flags;
    ra.t_tab = h->d_tab; ra.u_tab = h->d_tab + S0;
    ra.t_rand = e.d_t_rand ? e.d_t_rand + r0 * S0 : nullptr;
    ra.vd = k.vd; ra.nrm = k.nrm; ra.z0 = k.z0;
    hipLaunchKernelGGL(kw_ray_setup, dim3(rb), dim3(256), 0, st, ra);

    // the points of a pass of `nn` at the depths z (net_forward encodes them, in kw_embed or in the pass's own launch)
    auto points = [&](const Net& nn, const float* z, int S) {
      EmbedArgs ea{};
      ea.rays_o = ra.rays_o; ea.rays_d = ra.rays_d; ea.z = z; ea.vd = k.vd; ea.P = (long long)Rc * S; ea.S = S;
      ea.L = nn.d.multires; ea.Lv = nn.d.use_viewdirs ? nn.d.multires_views : -1;
      ea.ldE = nn.Ci; ea.ldED = nn.Cv;
      return ea;
    };
    // ---- coarse pass (RN:463-467) ----
    const float* sigma; int ld_sigma;
    const bool grad_coarse = grad_last && NI == 0;
    if (net_forward(h->gemm_cfg, st, n0, k, points(n0, k.z0, S0), (long long)Rc * S0, grad_coarse, &sigma, &ld_sigma)) return 1;
    CompositeArgs ca{};
    ca.R = Rc; ca.S = S0; ca.flags = h->cfg.flags; ca.rgb = k.RAW; ca.ld_rgb = n0.ldraw; ca.sigma = sigma; ca.ld_sigma = ld_sigma;
    ca.z = k.z0; ca.nrm = k.nrm; ca.noise = e.d_noise0 ? e.d_noise0 + r0 * S0 : nullptr; ca.weights = k.w0;
    float* rgb0 = NI > 0 ? o.d_rgb0 : o.d_rgb;
    float* disp0 = NI > 0 ? o.d_disp0 : o.d_disp;
    float* acc0 = NI > 0 ? o.d_acc0 : o.d_acc;
    ca.rgb_map = rgb0 ? rgb0 + r0 * 3 : nullptr; ca.disp = disp0 ? disp0 + r0 : nullptr; ca.acc = acc0 ? acc0 + r0 : nullptr;
    float* raw_c = NI == 0 ? o.d_raw : o.d_raw0;
    if (raw_c) {
      ca.raw_out = raw_c + r0 * S0 * n0.raw_ch; ca.raw_ch = n0.raw_ch;
      if (!n0.d.use_viewdirs) { ca.raw_src = k.RAW; ca.ld_raw = 32; }
    }
    if (ca.rgb_map && !(ca.disp && ca.acc)) return fail("nsrw: rgb / disp / acc outputs of a pass must be given together");
    stage_launch<CompositeArgs>(h, NSRW_STAGE_COMPOSITE, kw_composite, kw_composite_wave, ca, Rc, S0, st);
    if (o.d_weights0) NSRW_HIP(hipMemcpyAsync(o.d_weights0 + r0 * S0, k.w0, (size_t)Rc * S0 * 4, hipMemcpyDeviceToDevice, st));
    const float* z_last = k.z0;
    const float* noise_last = ca.noise;
    if (NI > 0) {
      // ---- resampling (RN:473-477) ----
      PdfArgs pa{};
      pa.R = Rc; pa.S0 = S0; pa.NI = NI; pa.z0 = k.z0; pa.w0 = k.w0; pa.u_tab = h->d_tab + S0;
      pa.u_rays = e.d_u ? e.d_u + r0 * NI : nullptr; pa.pdf = k.pdf; pa.cdf = k.cdf; pa.zs = k.zs;
      pa.inds = o.d_inds ? o.d_inds + r0 * NI : nullptr; pa.z_std = o.d_z_std ? o.d_z_std + r0 : nullptr;
      stage_launch<PdfArgs>(h, NSRW_STAGE_SAMPLE_PDF, kw_sample_pdf, kw_sample_pdf_wave, pa, Rc, S0, st);
      if (o.d_z_samples) NSRW_HIP(hipMemcpyAsync(o.d_z_samples + r0 * NI, k.zs, (size_t)Rc * NI * 4, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(kw_sort, dim3((unsigned)Rc), dim3(64), (size_t)S1 * sizeof(float), st, k.z0, k.zs, S0, NI, k.zf);
      if (e.d_z_fine)          // given depths (constants of the gradient, RN:475) replace the resampled ones for the fine pass
        NSRW_HIP(hipMemcpyAsync(k.zf, e.d_z_fine + r0 * S1, (size_t)Rc * S1 * 4, hipMemcpyDeviceToDevice, st));
      // ---- fine pass (RN:478-485) ----
      if (net_forward(h->gemm_cfg, st, n1, k, points(n1, k.zf, S1), (long long)Rc * S1, grad_last, &sigma, &ld_sigma)) return 1;
      CompositeArgs cf = ca;
      cf.S = S1; cf.ld_rgb = n1.ldraw; cf.sigma = sigma; cf.ld_sigma = ld_sigma; cf.z = k.zf; cf.noise = e.d_noise1 ? e.d_noise1 + r0 * S1 : nullptr;
      cf.weights = k.wf;
      cf.rgb_map = o.d_rgb ? o.d_rgb + r0 * 3 : nullptr; cf.disp = o.d_disp ? o.d_disp + r0 : nullptr;
      cf.acc = o.d_acc ? o.d_acc + r0 : nullptr;
      cf.raw_out = nullptr; cf.raw_src = nullptr;
      if (o.d_raw) {
        cf.raw_out = o.d_raw + r0 * S1 * last.raw_ch; cf.raw_ch = last.raw_ch;
        if (!last.d.use_viewdirs) { cf.raw_src = k.RAW; cf.ld_raw = 32; }
      }
      if (cf.rgb_map && !(cf.disp && cf.acc)) return fail("nsrw: rgb / disp / acc outputs of a pass must be given together");
      stage_launch<CompositeArgs>(h, NSRW_STAGE_COMPOSITE, kw_composite, kw_composite_wave, cf, Rc, S1, st);
      z_last = k.zf;
      noise_last = cf.noise;
    }
    if (o.d_z_vals) NSRW_HIP(hipMemcpyAsync(o.d_z_vals + r0 * SL, z_last, (size_t)Rc * SL * 4, hipMemcpyDeviceToDevice, st));
    // one pass's backward: raw2outputs (the pass's cotangents, offset to the chunk inside) -> network -> encodings and rays
    auto backward = [&](const Net& nn, const float* z, int S, const float* noise, const float* sg, int ld_sg, const float* g_rgb,
                        const float* g_disp, const float* g_acc, int accumulate) -> int {
      const long long P = (long long)Rc * S;
      NSRW_HIP(hipMemsetAsync(k.DRAW, 0, (size_t)P * 32 * 4, st));
      CompositeBwdArgs cb{};
      cb.R = Rc; cb.S = S; cb.flags = h->cfg.flags; cb.rgb = k.RAW; cb.ld_rgb = nn.ldraw; cb.sigma = sg; cb.ld_sigma = ld_sg;
      cb.z = z; cb.nrm = k.nrm; cb.noise = noise; cb.draw = k.DRAW; cb.gnorm = k.gnorm;
      cb.grad_rgb = g_rgb ? g_rgb + r0 * 3 : nullptr; cb.grad_disp = g_disp ? g_disp + r0 : nullptr;
      cb.grad_acc = g_acc ? g_acc + r0 : nullptr;
      cb.scr_a = k.scr_a; cb.scr_t = k.scr_t; cb.gscale = h->gemm_cfg.arith == kH2 ? k.gscale : nullptr;
      stage_launch<CompositeBwdArgs>(h, NSRW_STAGE_COMPOSITE_BWD, kw_composite_bwd, kw_composite_bwd_wave, cb, Rc, S, st);
      if (net_backward(h->gemm_cfg, st, nn, k, P)) return 1;
      EmbedBwdArgs eb{};
      eb.R = Rc; eb.S = S; eb.L = nn.d.multires; eb.Lv = nn.d.multires_views;
      eb.rays_o = ra.rays_o; eb.rays_d = ra.rays_d; eb.z = z; eb.vd = k.vd; eb.nrm = k.nrm; eb.gnorm = k.gnorm;
      eb.GE = k.GEP; eb.ldE = nn.Ci; eb.GED = nn.d.use_viewdirs ? k.GED : nullptr; eb.ldED = nn.Cv;
      eb.given_viewdirs = e.d_viewdirs != nullptr; eb.gscale = cb.gscale; eb.accumulate = accumulate;
      eb.grad_o = grad_o + r0 * 3; eb.grad_d = grad_d + r0 * 3; eb.grad_v = grad_v ? grad_v + r0 * 3 : nullptr;
      hipLaunchKernelGGL(kw_embed_bwd, dim3((unsigned)Rc), dim3(64), 0, st, eb);
      return 0;
    };
    if (grad_last && backward(last, z_last, SL, noise_last, sigma, ld_sigma, cot->d_rgb, cot->d_disp, cot->d_acc, 0)) return 1;
    if (grad_c) {
      // ---- the coarse pass's backward (RN:463-467 with rgb0 / disp0 / acc0, RN:492-494): its forward again, activations kept
      // (the buffers the last pass's backward is done with), then the same three stages, adding into the rays' gradients
      if (net_forward(h->gemm_cfg, st, n0, k, points(n0, k.z0, S0), (long long)Rc * S0, true, &sigma, &ld_sigma)) return 1;
      if (backward(n0, k.z0, S0, ca.noise, sigma, ld_sigma, cot->d_rgb0, cot->d_disp0, cot->d_acc0, grad_last ? 1 : 0)) return 1;
    }
    if (cot && !grad) {       // cotangents given, all NULL: the gradient of nothing
      NSRW_HIP(hipMemsetAsync(grad_o + r0 * 3, 0, (size_t)Rc * 3 * 4, st));
      NSRW_HIP(hipMemsetAsync(grad_d + r0 * 3, 0, (size_t)Rc * 3 * 4, st));
      if (grad_v) NSRW_HIP(hipMemsetAsync(grad_v + r0 * 3, 0, (size_t)Rc * 3 * 4, st));
    }
    ++h->chunks;
  }
  if (!cap) NSRW_HIP(hipEventRecord(h->ev1, st));
  h->timed = !cap;
  NSRW_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------------------
extern "C" {

const char* nsrw_last_error(void) { return g_err.c_str(); }

size_t nsrw_network_floats(const NsrwNet* net) {
  if (!net) { fail("nsrw_network_floats: null description"); return 0; }
  const std::string why = check_net(*net);
  if (!why.empty()) { fail("nsrw: " + why); return 0; }
  return net_floats(*net);
}

int nsrw_create(const NsrwConfig* cfg, nsrw_handle* out) {
  if (!cfg || !out) return fail("nsrw_create: null argument");
  if (cfg->n_samples < 3 || cfg->n_samples > NSRW_MAX_SAMPLES) return fail("nsrw_create: N_samples must be 3.." + std::to_string(NSRW_MAX_SAMPLES));
  if (cfg->n_importance < 0 || cfg->n_importance > NSRW_MAX_SAMPLES) return fail("nsrw_create: N_importance must be 0.." + std::to_string(NSRW_MAX_SAMPLES));
  int count = 0;
  NSRW_HIP(hipGetDeviceCount(&count));
  if (cfg->device < 0 || cfg->device >= count) return fail("nsrw_create: no such device");
  if (const char* refusal = flags_refusal(cfg->flags)) return fail(refusal);
  GemmCfg gc;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) gc.cus = prop.multiProcessorCount;
  }
  gc.flags = cfg->flags;
  gc.rows = (cfg->flags & NSRW_FLAG_RERUN_ROWS) != 0;
  gc.arith = (cfg->flags & NSRW_FLAG_MLP_F16X2) ? kH2 : (cfg->flags & NSRW_FLAG_MLP_BF16X3) ? kB3 : kF32;
  if (const char* wm = getenv("NSRW_B3_WM")) gc.tile_wm = atoi(wm) == 2 ? 2 : 4;
  Handle* h = new Handle();
  h->cfg = *cfg;
  h->gemm_cfg = gc;
  DeviceGuard guard(cfg->device);
  if (guard.err != hipSuccess) { delete h; return fail("nsrw_create: hipSetDevice failed"); }
  if (hipMalloc(&h->d_tab, (size_t)(cfg->n_samples + std::max(cfg->n_importance, 1)) * 4) != hipSuccess ||
      hipMalloc(&h->d_range, 8 * sizeof(unsigned)) != hipSuccess || hipMemset(h->d_range, 0, 8 * sizeof(unsigned)) != hipSuccess ||
      hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
    if (h->d_tab) (void)hipFree(h->d_tab);
    if (h->d_range) (void)hipFree(h->d_range);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    delete h;
    return fail("nsrw_create: out of device memory");
  }
  h->gemm_cfg.d_range = h->d_range;
  h->gemm_cfg.keep_passes = &h->keep_passes;
  h->gemm_cfg.rerun_launches = &h->rerun_launches;
  h->gemm_cfg.embed_counts = h->embed_counts;
  *out = reinterpret_cast<nsrw_handle>(h);
  return 0;
}

int nsrw_range_status(nsrw_handle hh, unsigned long long* passes, unsigned long long* passes_rerun) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h) return fail("nsrw_range_status: null handle");
  NSRW_DEVICE(h);
  unsigned r[4] = {0, 0, 0, 0};
  NSRW_HIP(hipDeviceSynchronize());
  NSRW_HIP(hipMemcpy(r, h->d_range, sizeof r, hipMemcpyDeviceToHost));
  if (passes) *passes = r[1];
  if (passes_rerun) *passes_rerun = r[2];
  return 0;
}

int nsrw_range_rows_status(nsrw_handle hh, unsigned long long* rows, unsigned long long* rows_rerun) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h) return fail("nsrw_range_rows_status: null handle");
  NSRW_DEVICE(h);
  unsigned long long r[2] = {0, 0};
  NSRW_HIP(hipDeviceSynchronize());
  NSRW_HIP(hipMemcpy(r, h->d_range + 4, sizeof r, hipMemcpyDeviceToHost));
  if (rows) *rows = r[0];
  if (rows_rerun) *rows_rerun = r[1];
  return 0;
}

int nsrw_rerun_rows_plan(const uint32_t* words, int64_t n_words, int64_t M, int tile_rows, int32_t* list_out, int64_t max) {
  if (n_words < 0 || (n_words > 0 && !words) || M < 0 || (tile_rows != 128 && tile_rows != 256) || max < 0 || (max > 0 && !list_out)) {
    fail("nsrw_rerun_rows_plan: n_words, M, max >= 0 with their buffers, tile_rows 128 or 256");
    return -1;
  }
  const int64_t mblocks = (M + tile_rows - 1) / tile_rows, wpb = tile_rows / 32;
  if (mblocks > 0x7fffffff) { fail("nsrw_rerun_rows_plan: more tile blocks than an int32 names"); return -1; }
  int64_t count = 0;
  for (int64_t mb = 0; mb < mblocks; ++mb) {
    bool any = false;
    for (int64_t q = 0; q < wpb && !any; ++q) {
      const int64_t wi = mb * wpb + q;
      if (wi >= n_words || wi * 32 >= M) break;
      uint32_t w = words[wi];
      const int64_t left = M - wi * 32;
      if (left < 32) w &= (1u << (int)left) - 1u;
      any = w != 0u;
    }
    if (any) {
      if (count < max) list_out[count] = (int32_t)mb;
      ++count;
    }
  }
  return (int)count;
}

int nsrw_destroy(nsrw_handle hh) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h) return 0;
  DeviceGuard guard(h->cfg.device);
  for (Net& n : h->net) free_net(n);
  if (h->d_tab) (void)hipFree(h->d_tab);
  if (h->d_range) (void)hipFree(h->d_range);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  delete h;
  return 0;
}

int nsrw_upload_tables(nsrw_handle hh, const float* t_coarse, int n_coarse, const float* u_fine, int n_fine) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !t_coarse) return fail("nsrw_upload_tables: null argument");
  if (n_coarse != h->cfg.n_samples || n_fine != h->cfg.n_importance || (n_fine > 0 && !u_fine))
    return fail("nsrw_upload_tables: table sizes must be the handle's N_samples / N_importance");
  NSRW_DEVICE(h);
  NSRW_HIP(hipMemcpy(h->d_tab, t_coarse, (size_t)n_coarse * 4, hipMemcpyHostToDevice));
  if (n_fine > 0) NSRW_HIP(hipMemcpy(h->d_tab + n_coarse, u_fine, (size_t)n_fine * 4, hipMemcpyHostToDevice));
  h->tables = true;
  return 0;
}

int nsrw_upload_network(nsrw_handle hh, int net_id, const NsrwNet* desc, const float* wts, size_t n_floats) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !desc || !wts) return fail("nsrw_upload_network: null argument");
  if (net_id < 0 || net_id > 1) return fail("nsrw_upload_network: net_id must be 0 or 1");
  const std::string why = check_net(*desc);
  if (!why.empty()) return fail("nsrw_upload_network: " + why);
  if (n_floats != net_floats(*desc)) return fail("nsrw_upload_network: expected " + std::to_string(net_floats(*desc)) + " floats, got " + std::to_string(n_floats));
  Net n;
  n.d = *desc;
  const int D = desc->D, W = desc->W;
  n.in_ch = 3 + 6 * desc->multires; n.in_v = 3 + 6 * desc->multires_views;
  n.Ci = pad32(n.in_ch); n.Cv = desc->use_viewdirs ? pad32(n.in_v) : 32; n.Wp = pad32(W); n.W2 = W / 2; n.W2p = pad32(std::max(n.W2, 1));
  n.ldfa = n.Wp;
  n.ldraw = desc->use_viewdirs ? 4 : 32;
  n.raw_ch = desc->use_viewdirs ? 4 : desc->output_ch;
  n.skip_in.assign(D, 0);
  for (int i = 1; i < D; ++i) n.skip_in[i] = is_skip(*desc, i - 1);
  // views of the parameter block
  std::vector<const float*> Wl(D), Bl(D);
  std::vector<int> Kin(D);
  const float* p = wts;
  for (int i = 0; i < D; ++i) {
    Kin[i] = i == 0 ? n.in_ch : (n.skip_in[i] ? n.in_ch + W : W);
    Wl[i] = p; p += (size_t)W * Kin[i];
    Bl[i] = p; p += W;
  }
  const float *Wf = nullptr, *Bf = nullptr, *Wa = nullptr, *Ba = nullptr, *Wv = nullptr, *Bv = nullptr, *Wr = nullptr, *Br = nullptr,
              *Wo = nullptr, *Bo = nullptr;
  const int Kv = W + n.in_v;
  if (desc->use_viewdirs) {
    Wf = p; p += (size_t)W * W; Bf = p; p += W;
    Wa = p; p += W; Ba = p; p += 1;
    Wv = p; p += (size_t)n.W2 * Kv; Bv = p; p += n.W2;
    Wr = p; p += (size_t)3 * n.W2; Br = p; p += 3;
  } else {
    Wo = p; p += (size_t)desc->output_ch * W; Bo = p; p += desc->output_ch;
  }
  std::vector<float> img, bias;        // the plain fp32 packing of every matrix (host only: input of the images) and the biases
  n.fwd.resize(D); n.bwd_h.resize(D); n.bwd_e.resize(D);
  const int in_ch = n.in_ch, Ci = n.Ci, Wp = n.Wp;
  for (int i = 0; i < D; ++i) {
    Mat& m = n.fwd[i];
    const float* w = Wl[i];
    const int K = Kin[i];
    m.Np = Wp;
    if (i == 0) {
      m.K1p = Ci;
      m.w = pack(img, Wp, Ci, [&](int nn, int kk) { return (nn < W && kk < in_ch) ? w[(size_t)nn * K + kk] : 0.0f; });
    } else if (n.skip_in[i]) {                      // cat[input_pts, h]: encoding columns first (RH:106)
      m.K1p = Ci; m.K2p = Wp;
      m.w = pack(img, Wp, Ci + Wp, [&](int nn, int kk) {
        if (nn >= W) return 0.0f;
        if (kk < Ci) return kk < in_ch ? w[(size_t)nn * K + kk] : 0.0f;
        const int c = kk - Ci;
        return c < W ? w[(size_t)nn * K + in_ch + c] : 0.0f;
      });
    } else {
      m.K1p = Wp;
      m.w = pack(img, Wp, Wp, [&](int nn, int kk) { return (nn < W && kk < W) ? w[(size_t)nn * K + kk] : 0.0f; });
    }
    m.b = pack_bias(bias, Wp, Bl[i], W);
    // transposed pieces for the backward: out[n'] = sum_k g[k] W_i[k][col(n')]
    const int hoff = (i > 0 && n.skip_in[i]) ? in_ch : 0;
    if (i > 0) {
      Mat& bh = n.bwd_h[i];
      bh.Np = Wp; bh.K1p = Wp;
      bh.w = pack(img, Wp, Wp, [&](int nn, int kk) { return (nn < W && kk < W) ? w[(size_t)kk * K + hoff + nn] : 0.0f; });
    }
    if (i == 0 || n.skip_in[i]) {
      Mat& be = n.bwd_e[i];
      be.Np = Ci; be.K1p = Wp;
      be.w = pack(img, Ci, Wp, [&](int nn, int kk) { return (nn < in_ch && kk < W) ? w[(size_t)kk * K + nn] : 0.0f; });
    }
  }
  if (desc->use_viewdirs) {
    const int W2 = n.W2, W2p = n.W2p, Cv = n.Cv, in_v = n.in_v;
    // feature_linear, and alpha_linear as a matrix of its own (row 0; its one output column goes to the raw block, net_forward)
    n.fa.Np = Wp; n.fa.K1p = Wp;
    n.fa.w = pack(img, Wp, Wp, [&](int nn, int kk) { return (nn < W && kk < W) ? Wf[(size_t)nn * W + kk] : 0.0f; });
    n.fa.b = pack_bias(bias, Wp, Bf, W);
    n.al.Np = 32; n.al.K1p = Wp;
    n.al.w = pack(img, 32, Wp, [&](int nn, int kk) { return (nn == 0 && kk < W) ? Wa[kk] : 0.0f; });
    n.al.b = pack_bias(bias, 32, Ba, 1);
    // views_linears.0 on cat[feature, input_views] (RH:113): A1 = FA's feature columns, A2 = direction encoding
    n.hv.Np = W2p; n.hv.K1p = Wp; n.hv.K2p = Cv;
    n.hv.w = pack(img, W2p, Wp + Cv, [&](int nn, int kk) {
      if (nn >= W2) return 0.0f;
      if (kk < Wp) return kk < W ? Wv[(size_t)nn * Kv + kk] : 0.0f;
      const int c = kk - Wp;
      return c < in_v ? Wv[(size_t)nn * Kv + W + c] : 0.0f;
    });
    n.hv.b = pack_bias(bias, W2p, Bv, W2);
    n.rgb.Np = 32; n.rgb.K1p = W2p;
    n.rgb.w = pack(img, 32, W2p, [&](int nn, int kk) { return (nn < 3 && kk < W2) ? Wr[(size_t)nn * W2 + kk] : 0.0f; });
    n.rgb.b = pack_bias(bias, 32, Br, 3);
    // backward heads
    n.b_rgb.Np = W2p; n.b_rgb.K1p = 32;
    n.b_rgb.w = pack(img, W2p, 32, [&](int nn, int kk) { return (nn < W2 && kk < 3) ? Wr[(size_t)kk * W2 + nn] : 0.0f; });
    n.b_feat.Np = Wp; n.b_feat.K1p = W2p;
    n.b_feat.w = pack(img, Wp, W2p, [&](int nn, int kk) { return (nn < W && kk < W2) ? Wv[(size_t)kk * Kv + nn] : 0.0f; });
    n.b_ed.Np = Cv; n.b_ed.K1p = W2p;
    n.b_ed.w = pack(img, Cv, W2p, [&](int nn, int kk) { return (nn < in_v && kk < W2) ? Wv[(size_t)kk * Kv + W + nn] : 0.0f; });
    n.b_head.Np = Wp; n.b_head.K1p = Wp; n.b_head.K2p = 32;       // [dL/dfeature | dL/draw]: feature_linear^T, alpha_linear^T at column 3
    n.b_head.w = pack(img, Wp, Wp + 32, [&](int nn, int kk) {
      if (nn >= W) return 0.0f;
      if (kk < Wp) return kk < W ? Wf[(size_t)kk * W + nn] : 0.0f;
      return kk - Wp == 3 ? Wa[nn] : 0.0f;
    });
  } else {
    const int oc = desc->output_ch;
    n.out.Np = 32; n.out.K1p = Wp;
    n.out.w = pack(img, 32, Wp, [&](int nn, int kk) { return (nn < oc && kk < W) ? Wo[(size_t)nn * W + kk] : 0.0f; });
    n.out.b = pack_bias(bias, 32, Bo, oc);
    n.b_head.Np = Wp; n.b_head.K1p = 32;                            // render_rays reads rows 0..3 of output_linear (RN:363-374)
    n.b_head.w = pack(img, Wp, 32, [&](int nn, int kk) { return (nn < W && kk < 4) ? Wo[(size_t)kk * W + nn] : 0.0f; });
  }
  // the weight images: per arithmetic the handle launches, every matrix in the layout that arithmetic's kernel moves into LDS
  std::vector<char> image[kArithSlots];
  for (Arith a : kAriths) {
    if (!has_image(h->gemm_cfg.arith, a)) continue;
    for_each_mat(n, [&](Mat& m) {
      if (m.Np <= 0) return;
      m.ncb = col_blocks(m.Np);
      m.img[a] = pack_image(image[a], a, img.data() + m.w, m.Np, m.K1p + m.K2p, &m.cscale);
    });
    if (image[a].size() >= 0x7fffffffull) return fail(std::string("nsrw_upload_network: network too large for the ") + arith_name(a) + " image");
  }
  n.onchip = onchip_plan(*desc, h->gemm_cfg.flags);
  const std::vector<TrunkLayer> trunk = trunk_table(n, &n.trunk_rows, &n.trunk_bwd_rows, &n.trunk_rerun_rows);
  n.bias_floats = (unsigned)bias.size();
  NSRW_DEVICE(h);
  // (every failure path below frees what this call allocated: ADVICE r05)
  hipError_t e = hipMalloc(&n.dBias, bias.size() * sizeof(float));
  if (e == hipSuccess && !trunk.empty()) e = hipMalloc(&n.dTrunk, trunk.size() * sizeof(TrunkLayer));
  if (e == hipSuccess && !trunk.empty()) e = hipMemcpy(n.dTrunk, trunk.data(), trunk.size() * sizeof(TrunkLayer), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(n.dBias, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice);
  for (Arith a : kAriths) {
    if (e != hipSuccess || image[a].empty()) continue;
    n.img_bytes[a] = image[a].size();
    e = hipMalloc(&n.dImg[a], n.img_bytes[a]);
    if (e == hipSuccess) e = hipMemcpy(n.dImg[a], image[a].data(), n.img_bytes[a], hipMemcpyHostToDevice);
  }
  Net& slot = h->net[net_id];
  if (e == hipSuccess && slot.loaded) e = hipDeviceSynchronize();      // a launch may still read the images being replaced
  if (e != hipSuccess) {
    free_net(n);
    return fail(std::string("nsrw_upload_network: ") + hipGetErrorString(e));
  }
  free_net(slot);
  slot = n;
  slot.loaded = true;
  return 0;
}

int nsrw_workspace_bytes(nsrw_handle hh, int64_t rays, int with_grad, size_t* bytes) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !bytes) return fail("nsrw_workspace_bytes: null argument");
  if (!h->net[0].loaded) return fail("nsrw_workspace_bytes: network 0 not uploaded");
  if (rays < 1) rays = 1;
  const long long R = (rays + 63) / 64 * 64;
  Carve c(nullptr);
  Chunk k;
  carve_chunk(*h, R, with_grad >= 2 ? 2 : with_grad != 0 ? 1 : 0, c, k);
  *bytes = c.off;
  return 0;
}

int nsrw_render_rays(nsrw_handle hh, const float* d_rays_o, const float* d_rays_d, int64_t n_rays, float near_, float far_,
                     const NsrwExtras* ex, const NsrwOut* out, void* ws, size_t ws_bytes, void* stream) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (check_common(h, d_rays_o, d_rays_d, n_rays, ex)) return 1;
  NSRW_DEVICE(h);
  return render_impl(h, d_rays_o, d_rays_d, n_rays, near_, far_, ex, nullptr, out, nullptr, nullptr, nullptr, ws, ws_bytes,
                     static_cast<hipStream_t>(stream));
}

int nsrw_render_rays_vjp(nsrw_handle hh, const float* d_rays_o, const float* d_rays_d, int64_t n_rays, float near_, float far_,
                         const NsrwExtras* ex, const float* d_grad_rgb, const NsrwOut* out, float* d_grad_o, float* d_grad_d,
                         float* d_grad_viewdirs, void* ws, size_t ws_bytes, void* stream) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (check_common(h, d_rays_o, d_rays_d, n_rays, ex)) return 1;
  if (n_rays > 0 && (!d_grad_rgb || !d_grad_o || !d_grad_d)) return fail("nsrw_render_rays_vjp: null gradient buffer");
  if (d_grad_viewdirs && !(ex && ex->d_viewdirs)) return fail("nsrw_render_rays_vjp: grad_viewdirs without given view directions");
  NSRW_DEVICE(h);
  NsrwCotangents cot{};
  cot.d_rgb = d_grad_rgb;
  return render_impl(h, d_rays_o, d_rays_d, n_rays, near_, far_, ex, &cot, out, d_grad_o, d_grad_d, d_grad_viewdirs, ws,
                     ws_bytes, static_cast<hipStream_t>(stream));
}

int nsrw_render_rays_vjp_cot(nsrw_handle hh, const float* d_rays_o, const float* d_rays_d, int64_t n_rays, float near_, float far_,
                             const NsrwExtras* ex, const NsrwCotangents* cot, const NsrwOut* out, float* d_grad_o, float* d_grad_d,
                             float* d_grad_viewdirs, void* ws, size_t ws_bytes, void* stream) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (check_common(h, d_rays_o, d_rays_d, n_rays, ex)) return 1;
  if (!cot) return fail("nsrw_render_rays_vjp_cot: null cotangents");
  if (n_rays > 0 && (!d_grad_o || !d_grad_d)) return fail("nsrw_render_rays_vjp_cot: null gradient buffer");
  if (h->cfg.n_importance == 0 && (cot->d_rgb0 || cot->d_disp0 || cot->d_acc0))
    return fail("nsrw_render_rays_vjp_cot: rgb0 / disp0 / acc0 cotangents without N_importance (the coarse pass IS the last one)");
  if (d_grad_viewdirs && !(ex && ex->d_viewdirs)) return fail("nsrw_render_rays_vjp_cot: grad_viewdirs without given view directions");
  NSRW_DEVICE(h);
  return render_impl(h, d_rays_o, d_rays_d, n_rays, near_, far_, ex, cot, out, d_grad_o, d_grad_d, d_grad_viewdirs, ws,
                     ws_bytes, static_cast<hipStream_t>(stream));
}

int nsrw_run_network(nsrw_handle hh, int net_id, const float* d_pts, const float* d_viewdirs, int64_t n_pts, float* d_raw,
                     void* ws, size_t ws_bytes, void* stream) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h) return fail("nsrw_run_network: null handle");
  if (net_id < 0 || net_id > 1 || !h->net[net_id].loaded) return fail("nsrw_run_network: network not uploaded");
  if (n_pts < 0 || (n_pts > 0 && (!d_pts || !d_raw))) return fail("nsrw_run_network: null argument");
  const Net& n = h->net[net_id];
  if (n.d.use_viewdirs && n_pts > 0 && !d_viewdirs) return fail("nsrw_run_network: this network takes view directions");
  if (n_pts == 0) return 0;
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255) != 0) return fail("nsrw_run_network: workspace must be 256-byte aligned");
  NSRW_DEVICE(h);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // points per pass: what the workspace holds of [E | ED | FA | HV | RAW | H0 | H1]
  // (+ 1 byte a point on a handle with NSRW_FLAG_RERUN_ROWS: rows_bytes is 4 (1 / 32 + 1 / 128 + 1 / 256) = 0.18 bytes a point and 20
  // bytes; the 4096 below cover the eight 256-byte roundings of the carve)
  const size_t per_pt = (size_t)(n.Ci + n.Cv + n.ldfa + n.W2p + 32 + 2 * n.Wp) * 4 + 64 + ((h->cfg.flags & NSRW_FLAG_RERUN_ROWS) ? 1 : 0);
  long long PB = (long long)((ws_bytes > 4096 ? ws_bytes - 4096 : 0) / per_pt) / 128 * 128;
  if (PB < 128) return fail("nsrw_run_network: workspace too small");
  PB = std::min<long long>(PB, (n_pts + 127) / 128 * 128);
  Carve c(ws);
  Chunk k;
  k.E = c.f(PB * n.Ci); k.ED = c.f(PB * n.Cv); k.FA = c.f(PB * n.ldfa); k.HV = c.f(PB * n.W2p); k.RAW = c.f(PB * 32);
  k.H = {c.f(PB * n.Wp), c.f(PB * n.Wp)};
  carve_rows(h->cfg.flags, PB, c, k);       // (per_pt counts it)
  if (c.off > ws_bytes) return fail("nsrw_run_network: workspace too small");
  if (k.rows.words) NSRW_HIP(hipMemsetAsync(k.rows.words, 0, rows_bytes(PB), st));
  const bool cap = capturing(st);
  if (!cap) NSRW_HIP(hipEventRecord(h->ev0, st));
  h->chunks = 0;
  for (long long p0 = 0; p0 < n_pts; p0 += PB) {
    const long long P = std::min<long long>(PB, n_pts - p0);
    EmbedArgs ea{};
    ea.pts = d_pts + p0 * 3; ea.dirs = d_viewdirs ? d_viewdirs + p0 * 3 : nullptr; ea.P = P; ea.S = 1;
    ea.L = n.d.multires; ea.Lv = n.d.use_viewdirs ? n.d.multires_views : -1;
    ea.ldE = n.Ci; ea.ldED = n.Cv;
    const float* sigma; int ld_sigma;
    if (net_forward(h->gemm_cfg, st, n, k, ea, P, false, &sigma, &ld_sigma)) return 1;
    const int C = n.raw_ch;
    if (n.d.use_viewdirs) {          // the raw block IS [P, 4] = [r g b sigma]
      NSRW_HIP(hipMemcpyAsync(d_raw + p0 * 4, k.RAW, (size_t)P * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
      hipLaunchKernelGGL(kw_copy_rows, dim3((unsigned)((P * C + 255) / 256)), dim3(256), 0, st, k.RAW, 32, d_raw + p0 * C, C, P, C);
    }
    ++h->chunks;
  }
  if (!cap) NSRW_HIP(hipEventRecord(h->ev1, st));
  h->timed = !cap;
  NSRW_HIP(hipGetLastError());
  return 0;
}

int nsrw_gemm_plan(int n_packed_rows, int n_stored_columns, int tile_wm, NsrwGemmPart* parts_out, int max_parts) {
  if (n_packed_rows < 1 || n_packed_rows > NSRW_MAX_WIDTH || (tile_wm != 2 && tile_wm != 4) || max_parts < 0 || (max_parts > 0 && !parts_out)) {
    fail("nsrw_gemm_plan: 1..NSRW_MAX_WIDTH packed rows, tile_wm 2 or 4, max_parts >= 0 with a buffer");
    return -1;
  }
  NsrwGemmPart parts[kMaxGemmParts];
  const int count = gemm_plan(col_blocks(n_packed_rows), n_stored_columns, tile_wm, parts);
  for (int i = 0; i < std::min(count, max_parts); ++i) parts_out[i] = parts[i];
  return count;
}

const char* nsrw_flags_refusal(int flags) { return flags_refusal(flags); }

// the views of onchip_plan: 0 and the decision, or -1 for an invalid description (nsrw_last_error says why)
static int plan_entry(const char* name, const NsrwNet* net, const void* plan_out, int flags, OnchipPlan* p) {
  if (!net || !plan_out) { fail(std::string(name) + ": null argument"); return -1; }
  const std::string why = check_net(*net);
  if (!why.empty()) { fail(std::string(name) + ": " + why); return -1; }
  *p = onchip_plan(*net, flags);
  return 0;
}

int nsrw_trunk_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out) {
  OnchipPlan p;
  if (plan_entry("nsrw_trunk_plan", net, plan_out, flags, &p)) return -1;
  *plan_out = as_trunk_plan(p.trunk);
  return 0;
}

int nsrw_heads_plan(const NsrwNet* net, int flags, NsrwHeadsPlan* plan_out) {
  OnchipPlan p;
  if (plan_entry("nsrw_heads_plan", net, plan_out, flags, &p)) return -1;
  *plan_out = as_heads_plan(p.heads);
  return 0;
}

int nsrw_trunk_bwd_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out) {
  OnchipPlan p;
  if (plan_entry("nsrw_trunk_bwd_plan", net, plan_out, flags, &p)) return -1;
  *plan_out = as_trunk_plan(p.bwd);
  return 0;
}

int nsrw_trunk_keep_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out) {
  OnchipPlan p;
  const int rc = plan_entry("nsrw_trunk_keep_plan", net, plan_out, flags, &p);
  if (rc == 0) *plan_out = as_trunk_plan(p.keep);
  return rc;
}

int nsrw_keep_status(nsrw_handle hh, unsigned long long* passes_onchip) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !passes_onchip) return fail("nsrw_keep_status: null argument");
  *passes_onchip = h->keep_passes;
  return 0;
}

int nsrw_trunk_rerun_plan(const NsrwNet* net, int flags, NsrwTrunkPlan* plan_out) {
  OnchipPlan p;
  if (plan_entry("nsrw_trunk_rerun_plan", net, plan_out, flags, &p)) return -1;
  *plan_out = as_trunk_plan(p.rerun);
  return 0;
}

int nsrw_rerun_status(nsrw_handle hh, unsigned long long* launches_onchip) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !launches_onchip) return fail("nsrw_rerun_status: null argument");
  *launches_onchip = h->rerun_launches;
  return 0;
}

int nsrw_embed_plan(const NsrwNet* net, int flags, int kept, NsrwEmbedPlan* plan_out) {
  OnchipPlan p;
  if (plan_entry("nsrw_embed_plan", net, plan_out, flags, &p)) return -1;
  const EmbedOn& e = p.embed[kept ? 1 : 0];
  NsrwEmbedPlan o{};
  o.positions_onchip = e.form ? 1 : 0;
  o.directions_onchip = e.dirs ? 1 : 0;
  snprintf(o.positions_reason, sizeof o.positions_reason, "%s", e.why);
  snprintf(o.directions_reason, sizeof o.directions_reason, "%s", e.why_dirs);
  *plan_out = o;
  return 0;
}

int nsrw_embed_status(nsrw_handle hh, unsigned long long* passes_onchip, unsigned long long* embed_launches,
                      unsigned long long* embed_launches_conditional) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !passes_onchip || !embed_launches || !embed_launches_conditional) return fail("nsrw_embed_status: null argument");
  *passes_onchip = h->embed_counts[0];
  *embed_launches = h->embed_counts[1];
  *embed_launches_conditional = h->embed_counts[2];
  return 0;
}

int nsrw_stage_plan(int stage, int samples, int n_importance, int flags, NsrwStagePlan* plan_out) {
  if (!plan_out) { fail("nsrw_stage_plan: null argument"); return -1; }
  const bool pdf = stage == NSRW_STAGE_SAMPLE_PDF;
  if (stage != NSRW_STAGE_COMPOSITE && !pdf && stage != NSRW_STAGE_COMPOSITE_BWD) { fail("nsrw_stage_plan: no such stage"); return -1; }
  if (samples < 3 || samples > (pdf ? NSRW_MAX_SAMPLES : 2 * NSRW_MAX_SAMPLES) || (pdf && (n_importance < 1 || n_importance > NSRW_MAX_SAMPLES))) {
    fail("nsrw_stage_plan: 3.." + std::to_string(2 * NSRW_MAX_SAMPLES) + " samples of a pass (NSRW_STAGE_SAMPLE_PDF: 3.." +
         std::to_string(NSRW_MAX_SAMPLES) + " coarse samples and 1.." + std::to_string(NSRW_MAX_SAMPLES) + " to draw)");
    return -1;
  }
  *plan_out = stage_plan(stage, samples, pdf ? n_importance : 0, flags);
  return 0;
}

int nsrw_stages_status(nsrw_handle hh, unsigned long long* launches_wave) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !launches_wave) return fail("nsrw_stages_status: null argument");
  *launches_wave = h->stage_launches;
  return 0;
}

int nsrw_debug_bounds_status(int* built_with_checks, unsigned* first_bad_line) {
  if (!built_with_checks || !first_bad_line) return fail("nsrw_debug_bounds_status: null argument");
  *first_bad_line = 0;
#ifdef NSR_DEBUG_BOUNDS
  *built_with_checks = 1;
  NSRW_HIP(hipDeviceSynchronize());
  NSRW_HIP(hipMemcpyFromSymbol(first_bad_line, HIP_SYMBOL(nsrw::g_wide_violation), sizeof(unsigned)));
#else
  *built_with_checks = 0;
#endif
  return 0;
}

int nsrw_sample_pdf(int device, const float* d_bins, const float* d_weights, int64_t n_rows, int n_bins, const float* d_u,
                    int u_per_row, int n_samples, float* d_samples, int64_t* d_inds, float* d_scratch, void* stream) {
  if (!d_bins || !d_weights || !d_u || !d_samples || !d_scratch) return fail("nsrw_sample_pdf: null argument");
  if (n_rows < 0 || n_rows > 0x7fffffffll) return fail("nsrw_sample_pdf: 0 .. 2^31 - 1 rows");
  if (n_bins < 2 || n_bins > NSRW_MAX_SAMPLES || n_samples < 1 || n_samples > NSRW_MAX_SAMPLES)
    return fail("nsrw_sample_pdf: 2.." + std::to_string(NSRW_MAX_SAMPLES) + " bins, 1.." + std::to_string(NSRW_MAX_SAMPLES) + " samples");
  if (n_rows == 0) return 0;
  DeviceGuard guard_(device);
  NSRW_HIP(guard_.err);
  PdfArgs pa{};
  pa.R = (int)n_rows; pa.S0 = n_bins + 1; pa.NI = n_samples; pa.z0 = d_bins; pa.w0 = d_weights; pa.bins = d_bins;
  pa.u_tab = u_per_row ? nullptr : d_u; pa.u_rays = u_per_row ? d_u : nullptr;
  pa.pdf = d_scratch; pa.cdf = d_scratch + (size_t)n_rows * (n_bins + 1);
  pa.zs = d_samples; pa.inds = d_inds; pa.z_std = nullptr;
  hipLaunchKernelGGL(kw_sample_pdf, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pa);
  NSRW_HIP(hipGetLastError());
  return 0;
}

int nsrw_embed_vjp(int device, const float* d_x, const float* d_grad_out, int64_t n_points, int multires, float* d_grad_x, void* stream) {
  if (!d_x || !d_grad_out || !d_grad_x) return fail("nsrw_embed_vjp: null argument");
  if (n_points < 0 || multires < 0 || multires > 15) return fail("nsrw_embed_vjp: n_points >= 0, multires 0..15");
  if (n_points == 0) return 0;
  DeviceGuard guard_(device);
  NSRW_HIP(guard_.err);
  hipLaunchKernelGGL(kw_embed_vjp, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_x, d_grad_out,
                     (long long)n_points, multires, d_grad_x);
  NSRW_HIP(hipGetLastError());
  return 0;
}

int nsrw_rerun_rows_list(int device, const uint32_t* d_words, int64_t M, int tile_rows, int32_t* d_list, int64_t max, uint32_t* d_range,
                         void* stream) {
  if (!d_words || !d_list) return fail("nsrw_rerun_rows_list: null argument");
  if (M < 1 || (tile_rows != 128 && tile_rows != 256) || M / tile_rows >= 0x7fffffffll || max < (M + tile_rows - 1) / tile_rows)
    return fail("nsrw_rerun_rows_list: M >= 1, tile_rows 128 or 256, and room for every block of the pass in the list");
  DeviceGuard guard_(device);
  NSRW_HIP(guard_.err);
  RowsListArgs a{};
  a.words = d_words; a.M = M; a.n_words = (int)((M + 31) / 32); a.tile_rows = tile_rows;
  a.list = d_list; a.list_max = (int)std::min<int64_t>(max, 0x7fffffff);
  a.range = d_range; a.tally = d_range != nullptr;
  const long long mblocks = (M + tile_rows - 1) / tile_rows;
  hipLaunchKernelGGL(kw_rows_list, dim3((unsigned)((mblocks + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  NSRW_HIP(hipGetLastError());
  return 0;
}

int nsrw_last_ms(nsrw_handle hh, float* ms, int* chunks) {
  Handle* h = reinterpret_cast<Handle*>(hh);
  if (!h || !ms) return fail("nsrw_last_ms: null argument");
  if (!h->timed) return fail("nsrw_last_ms: no timed launch yet (launches captured into a hipGraph are not timed)");
  NSRW_DEVICE(h);
  NSRW_HIP(hipEventSynchronize(h->ev1));
  NSRW_HIP(hipEventElapsedTime(ms, h->ev0, h->ev1));
  if (chunks) *chunks = h->chunks;
  return 0;
}

}  // extern "C"
