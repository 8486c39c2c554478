// nsr_wide_stages.inc -- the per-ray stages of the layered renderer with ONE WAVE PER RAY (NSRW_FLAG_STAGES_WAVE): kw_composite_wave,
// kw_sample_pdf_wave and kw_composite_bwd_wave, held bit for bit to kw_composite, kw_sample_pdf and kw_composite_bwd (nsr_wide.hip),
// whose argument structs they take unchanged.  Included by nsr_wide.hip behind those kernels.
//
// The thread-per-ray kernels walk a ray's samples in one thread: every load of a wave touches 64 rows a whole ray apart, and the
// whole stage runs at the latency of those loads.  Here a workgroup is rays_per_group waves (4, 2 or 1: stage_plan) and wave w of
// group g owns ray g * rays_per_group + w, with its own slice of the dynamic LDS; nothing is shared between the waves of a group,
// so there is no workgroup barrier and a ray's bits cannot depend on its neighbours.  Within a wave:
//   * everything ELEMENTWISE in the sample index -- the loads, dists, alpha, the sigmoids, the products w * c, pdf, the importance
//     samples, the gradient rows -- belongs to lane i % 64: consecutive lanes read and write consecutive samples;
//   * every CHAIN -- a sum or product whose association order the thread kernel fixes -- runs on ONE lane in that order over
//     operands that the elementwise step left in LDS.  Independent chains (the five weighted sums, ATen's eight vector lanes) run
//     side by side on one lane each.
// The unit is compiled -ffp-contract=off: `x = x + w * c` is a rounded product and a rounded sum in either kernel, so the product
// may be taken by lane i % 64 and the sum by the chain's lane -- the same IEEE operations on the same values in the same order, hence
// the same bits.  expf, sigmoidf_, relu_nan and grad_norm_scale are the thread kernels' own functions.
// The only synchronisation is wave_lds_sync: LDS written by one lane of the wave, read by another.
#undef NSRW_FILE_TAG
#define NSRW_FILE_TAG 300000        /* a failed NSRW_CHECK of this file reports 300000 + its line (nsrw_debug_bounds_status) */

constexpr int kStageLdsMax = 64 * 1024;       // what a workgroup takes without raising the kernel's LDS attribute

// LDS bytes ONE ray of a stage kernel needs (stage_plan: the one statement of it; the kernels below carve exactly this).
//   composite      5 floats per sample: [om -> T -> w z] [alpha -> w] [w c0] [w c1] [w c2]
//   sample_pdf     x / pdf [S0], cdf [S0], z0 [S0] and zs [NI] floats
//   composite_bwd  16 bytes per sample: one fp64 [(w z, w) -> A w -> suffix -> dn's term] and two floats [alpha] [om -> T]
__host__ __device__ constexpr int stage_lds_composite(int S) { return 20 * S; }
__host__ __device__ constexpr int stage_lds_sample_pdf(int S0, int NI) { return 4 * (3 * S0 + NI); }
__host__ __device__ constexpr int stage_lds_composite_bwd(int S) { return 16 * S; }

// LDS written by some lanes of this wave is read by others: a release / acquire pair at wavefront scope around a wave barrier
// (the lanes of a wave run in lockstep; this orders the LDS operations and keeps the compiler from moving them across)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// alpha of sample i of ray r, as kw_composite computes it (RN:356-361, RN:374)
__device__ __forceinline__ float stage_alpha(const float* z, int i, int S, float nrm, float sg_raw, const float* noise, long long p) {
  float dist = (i < S - 1) ? (z[i + 1] - z[i]) : 1e10f;
  dist = dist * nrm;
  float sg = sg_raw;
  if (noise) sg = sg + noise[p];
  return 1.0f - expf(-relu_nan(sg) * dist);
}

// chain 1, on the calling lane: t[i] = (float)T_i, T_{i+1} = T_i * (double)om[i] -- the exclusive fp64 product, every prefix rounded
// to fp32 before its multiply.  In place: t[i] holds om[i] on entry.
__device__ __forceinline__ void stage_transmittance(float* t, int S) {
  double T = 1.0;
  int i = 0;
  for (; i + 8 <= S; i += 8) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = t[i + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      t[i + k] = (float)T;
      T = T * (double)f[k];
    }
  }
  for (; i < S; ++i) {
    const float f = t[i];
    t[i] = (float)T;
    T = T * (double)f;
  }
}

// a sequential fp32 sum in index order, on the calling lane: x = x + v[i]
__device__ __forceinline__ float stage_sum_f32(const float* v, int stride, int S) {
  float x = 0.f;
  int i = 0;
  for (; i + 8 <= S; i += 8) {
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = v[(i + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) x = x + f[k];
  }
  for (; i < S; ++i) x = x + v[i * stride];
  return x;
}

// raw2outputs (RN:343-387) of one ray per wave.  Grid: ceil(R / rays_per_group) groups of 64 * rays_per_group threads.
__global__ void __launch_bounds__(256) kw_composite_wave(const CompositeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stage_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.R) return;
  const int S = a.S;
  NSRW_CHECK((wave + 1) * stage_lds_composite(S) <= kStageLdsMax);
  float* s_t = reinterpret_cast<float*>(stage_lds + (size_t)wave * stage_lds_composite(S));      // om -> T -> w z
  float* s_w = s_t + S;                                                                           // alpha -> w
  float* s_c0 = s_w + S;
  float* s_c1 = s_c0 + S;
  float* s_c2 = s_c1 + S;
  const float* z = a.z + r * S;
  const float nrm = a.nrm[r];
  // elementwise: alpha, om, the three sigmoids; the raw copy
  for (int i = lane; i < S; i += 64) {
    const long long p = r * S + i;
    const float al = stage_alpha(z, i, S, nrm, a.sigma[p * a.ld_sigma], a.noise, p);
    s_w[i] = al;
    s_t[i] = (1.0f - al) + 1e-10f;
    const float* q = a.rgb + p * a.ld_rgb;
    s_c0[i] = sigmoidf_(q[0]);                                             // RN:363
    s_c1[i] = sigmoidf_(q[1]);
    s_c2[i] = sigmoidf_(q[2]);
  }
  if (a.raw_out) {
    const int C = a.raw_ch;
    float* o = a.raw_out + r * S * C;
    if (a.raw_src) {
      for (int e = lane; e < S * C; e += 64) {
        const int i = e / C, c = e - i * C;
        o[e] = a.raw_src[(r * S + i) * a.ld_raw + c];
      }
    } else {
      for (int e = lane; e < S * 4; e += 64) {
        const int i = e >> 2, c = e & 3;
        const long long p = r * S + i;
        o[e] = c < 3 ? a.rgb[p * a.ld_rgb + c] : a.sigma[p * a.ld_sigma];
      }
    }
  }
  wave_lds_sync();
  if (lane == 0) stage_transmittance(s_t, S);                              // chain 1
  wave_lds_sync();
  // elementwise: w = alpha * (float)T_i (RN:376), its store, and the five products the chains add up
  float* wout = a.weights + r * S;
  for (int i = lane; i < S; i += 64) {
    const float w = s_w[i] * s_t[i];
    wout[i] = w;
    s_w[i] = w;
    s_c0[i] = w * s_c0[i];                                                 // RN:378
    s_c1[i] = w * s_c1[i];
    s_c2[i] = w * s_c2[i];
    s_t[i] = w * z[i];                                                     // RN:380
  }
  wave_lds_sync();
  if (!a.rgb_map) return;
  // chains 2-6 on lanes 0..4: cr, cg, cb, depth, acc as sequential fp32 sums in sample order
  float x = 0.f;
  if (lane < 5) x = stage_sum_f32(lane == 0 ? s_c0 : lane == 1 ? s_c1 : lane == 2 ? s_c2 : lane == 3 ? s_t : s_w, 1, S);
  float cr = __shfl(x, 0), cg = __shfl(x, 1), cb = __shfl(x, 2);
  const float depth = __shfl(x, 3), acc = __shfl(x, 4);
  if (lane != 0) return;
  const float qd = depth / acc;
  const float disp = (qd != qd) ? qd : 1.0f / fmaxf(1e-10f, qd);           // RN:381: 0/0 -> NaN propagates through torch.max
  if (a.flags & NSRW_FLAG_WHITE_BKGD) {                                     // RN:384-385
    const float bg = 1.0f - acc;
    cr = cr + bg; cg = cg + bg; cb = cb + bg;
  }
  a.rgb_map[r * 3 + 0] = cr; a.rgb_map[r * 3 + 1] = cg; a.rgb_map[r * 3 + 2] = cb;
  a.disp[r] = disp; a.acc[r] = acc;
}

// sample_pdf (RH:199-243) for bins = mid-points of the coarse depths and z_std (RN:495) of one ray per wave; kw_sample_pdf's
// arithmetic (its comment has ATen's sum order).  The `bins` form of the stage entry is not taken: it stays on kw_sample_pdf.
__global__ void __launch_bounds__(256) kw_sample_pdf_wave(const PdfArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stage_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.R) return;
  const int S0 = a.S0, NI = a.NI, NW = S0 - 2, NC = S0 - 1;
  NSRW_CHECK(!a.bins && (wave + 1) * stage_lds_sample_pdf(S0, NI) <= kStageLdsMax);
  float* x = reinterpret_cast<float*>(stage_lds + (size_t)wave * stage_lds_sample_pdf(S0, NI));      // [S0]: weights + 1e-5 -> pdf
  float* cdf = x + S0;                                                                                // [S0]: entries 0 .. NW
  float* sz = cdf + S0;                                                                               // [S0]: the coarse depths
  float* szs = sz + S0;                                                                               // [NI]: the samples, for z_std
  const float* z = a.z0 + r * S0;
  const float* w = a.w0 + r * S0 + 1;
  for (int i = lane; i < S0; i += 64) {
    sz[i] = z[i];
    if (i < NW) x[i] = w[i] + 1e-5f;                                       // RH:201
  }
  wave_lds_sync();
  // torch.sum: lane jj < 8 runs the four partial accumulators of vector lane jj, the left-over whole vectors into partial 0
  const int nvec = NW / 8, silp = nvec / 4;
  float lj = 0.0f;
  if (lane < 8) {
    float ps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < silp; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) ps[k] = ps[k] + x[(i * 4 + k) * 8 + lane];
    for (int v = silp * 4; v < nvec; ++v) ps[0] = ps[0] + x[v * 8 + lane];
    lj = ((ps[0] + ps[1]) + ps[2]) + ps[3];
  }
  float total = 0.0f;                                                      // (every lane: the scalar tail, then the eight lanes in order)
  for (int i = nvec * 8; i < NW; ++i) total = total + x[i];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) total = total + __shfl(lj, jj);
  wave_lds_sync();
  for (int i = lane; i < NW; i += 64) x[i] = x[i] / total;                 // RH:202
  wave_lds_sync();
  if (lane == 0) {                                                         // RH:203-204: sequential fp64 sum, rounded per prefix
    double run = 0.0;
    cdf[0] = 0.0f;
    int i = 0;
    for (; i + 8 <= NW; i += 8) {
      float f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = x[i + k];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        run = run + (double)f[k];
        cdf[i + k + 1] = (float)run;
      }
    }
    for (; i < NW; ++i) {
      run = run + (double)x[i];
      cdf[i + 1] = (float)run;
    }
  }
  wave_lds_sync();
  float* zs = a.zs + r * NI;
  for (int k = lane; k < NI; k += 64) {
    const float u = a.u_rays ? a.u_rays[r * NI + k] : a.u_tab[k];
    int lo = 0, hi = NC;                                                   // RH:227: first index with cdf > u
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      NSRW_CHECK(mid >= 0 && mid < NC);
      if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
    }
    const int below = max(lo - 1, 0), above = min(lo, NC - 1);             // RH:228-229
    NSRW_CHECK(lo >= 0 && lo <= NC && below >= 0 && above >= 0 && above + 1 < S0 && below + 1 < S0 && NC < S0);
    const float c0 = cdf[below], c1 = cdf[above];
    const float b0 = 0.5f * (sz[below + 1] + sz[below]);                   // RN:473
    const float b1 = 0.5f * (sz[above + 1] + sz[above]);
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.0f;                                       // RH:238-239
    const float t = (u - c0) / denom;
    const float s = b0 + t * (b1 - b0);                                    // RH:241
    zs[k] = s;
    szs[k] = s;
    if (a.inds) a.inds[r * NI + k] = (int64_t)lo;
  }
  if (!a.z_std) return;
  wave_lds_sync();
  if (lane == 0) {                                                         // RN:495: fp64 two-pass over the fp32 samples, in order
    double sum = 0.0;
    for (int k = 0; k < NI; ++k) sum += (double)szs[k];
    const double mean = sum / NI;
    double var = 0.0;
    for (int k = 0; k < NI; ++k) { const double d = (double)szs[k] - mean; var += d * d; }
    a.z_std[r] = (float)sqrt(var / NI);
  }
}

// Backward of one pass's raw2outputs of one ray per wave; kw_composite_bwd's arithmetic (its comment has the derivation).  scr_a / scr_t
// are not touched: alpha_i and T_i stay in LDS.
__global__ void __launch_bounds__(256) kw_composite_bwd_wave(const CompositeBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char stage_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.R) return;
  const int S = a.S;
  NSRW_CHECK((wave + 1) * stage_lds_composite_bwd(S) <= kStageLdsMax);
  double* s_d = reinterpret_cast<double*>(stage_lds + (size_t)wave * stage_lds_composite_bwd(S));     // (w z, w) -> A w -> suffix -> dn's term
  float* s_al = reinterpret_cast<float*>(s_d + S);                                                    // alpha
  float* s_t = s_al + S;                                                                              // om -> T
  const float* z = a.z + r * S;
  const float nrm = a.nrm[r];
  for (int i = lane; i < S; i += 64) {
    const long long p = r * S + i;
    const float al = stage_alpha(z, i, S, nrm, a.sigma[p * a.ld_sigma], a.noise, p);
    s_al[i] = al;
    s_t[i] = (1.0f - al) + 1e-10f;
  }
  wave_lds_sync();
  if (lane == 0) stage_transmittance(s_t, S);
  wave_lds_sync();
  float depth = 0.f, acc = 0.f;       // the forward's sequential fp32 sums (RN:380, RN:382), for disp only
  if (a.grad_disp) {
    float* s_f = reinterpret_cast<float*>(s_d);                            // [S][2]: w z, w
    for (int i = lane; i < S; i += 64) {
      const float w = s_al[i] * s_t[i];
      s_f[2 * i + 0] = w * z[i];
      s_f[2 * i + 1] = w;
    }
    wave_lds_sync();
    float x = 0.f;
    if (lane < 2) x = stage_sum_f32(s_f + lane, 2, S);
    depth = __shfl(x, 0); acc = __shfl(x, 1);
    wave_lds_sync();
  }
  // the per-ray scalars (every lane holds them)
  const double g0 = a.grad_rgb ? a.grad_rgb[r * 3 + 0] : 0.0, g1 = a.grad_rgb ? a.grad_rgb[r * 3 + 1] : 0.0,
               g2 = a.grad_rgb ? a.grad_rgb[r * 3 + 2] : 0.0;
  const double gsum = (a.flags & NSRW_FLAG_WHITE_BKGD) ? (g0 + g1 + g2) : 0.0;
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
  // elementwise: A_i and w_i, their product for the suffix chain
  for (int i = lane; i < S; i += 64) {
    const long long p = r * S + i;
    const float* q = a.rgb + p * a.ld_rgb;
    const double c0 = sigmoidf_(q[0]), c1 = sigmoidf_(q[1]), c2 = sigmoidf_(q[2]);
    const double w = (double)(s_al[i] * s_t[i]);
    double A = g0 * c0 + g1 * c1 + g2 * c2 - gsum;
    if (extra) A += g_w + g_z * (double)z[i];
    s_d[i] = A * w;
  }
  wave_lds_sync();
  if (lane == 0) {                    // suffix: from the last sample to the first; s_d[i] <- the value BEFORE sample i's add
    double suffix = 0.0;
    for (int i = S - 1; i >= 0; --i) {
      const double aw = s_d[i];
      s_d[i] = suffix;
      suffix += aw;
    }
  }
  wave_lds_sync();
  for (int i = lane; i < S; i += 64) {
    const long long p = r * S + i;
    const float* q = a.rgb + p * a.ld_rgb;
    const double c0 = sigmoidf_(q[0]), c1 = sigmoidf_(q[1]), c2 = sigmoidf_(q[2]);
    const double al = s_al[i], Ti = s_t[i];
    const double w = (double)(s_al[i] * s_t[i]);
    double A = g0 * c0 + g1 * c1 + g2 * c2 - gsum;
    if (extra) A += g_w + g_z * (double)z[i];
    const double om = (double)((1.0f - s_al[i]) + 1e-10f);
    const double suffix = s_d[i];
    const double d_alpha = A * Ti - suffix / om;
    float sg = a.sigma[p * a.ld_sigma];
    if (a.noise) sg = sg + a.noise[p];
    const double dz = (i < S - 1) ? (double)(z[i + 1] - z[i]) : 1e10;
    const double e = 1.0 - al;
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
    *reinterpret_cast<f32x4*>(a.draw + p * 32) = f32x4{o0, o1, o2, o3};
    s_d[i] = d_alpha * (double)relu_nan(sg) * e * dz;                      // d(dz |d|) / d|d| = dz
  }
  wave_lds_sync();
  if (lane == 0) {                    // dn: from the last sample to the first
    double dn = 0.0;
    for (int i = S - 1; i >= 0; --i) dn += s_d[i];
    a.gnorm[r] = (float)dn;
  }
}
