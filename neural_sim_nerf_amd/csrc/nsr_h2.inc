// nsr_h2.inc -- the layer GEMMs on v_mfma_f32_32x32x16_f16 with fp32 operands split into TWO fp16 pieces ("f16x2").
// Included inside namespace nsr, after the ring, the fp32 segments and nsr_b3.inc (nsr_kernels.hip).
//
// x = x0 + x1 with x0 = fp16(x) (round to nearest even) and x1 = fp16(x - x0): 11 + 11 significand bits, |x - x0 - x1| <=
// 2^-23 |x| as long as x1 is a normal fp16 (|x| >= 2^-2), else <= 2^-25 absolute (fp16 subnormal spacing 2^-24; the MFMA
// honours fp16 subnormal inputs, tools/probe_f16_mfma.hip).  Of the four piece products of a*b the three of weight >=
// 2^-11 are kept -- a0b0, a0b1, a1b0, each exact in the MFMA's fp32 product stage (11 + 11 bits) -- and a1b1 <= 2^-22 |a||b|
// is dropped.  Per 32x32x16 block of products three fp16 MFMAs of 32 matrix-pipe cycles replace eight fp32 32x32x2 MFMAs
// of 64 (96 against 512 cycles) or the six of bf16x3 (192).  What keeps the result fp32-grade is RANGE MANAGEMENT, all of
// it by exact powers of two decided by the packer (pack.pack_network_h2):
//   * every weight matrix is scaled by 2^sw so that its largest entry sits just below 2^15: the low pieces of the weights
//     are then far above the fp16 subnormal range; biases are scaled by 2^(sw + ca) and the accumulators carry that scale;
//   * the activations handed to a GEMM are scaled by m = 2^(ca - P) on the fly (P = the scale the registers carry from the
//     previous layer; ca = 0 unless the packer was told to calibrate), i.e. the un-scaling of one layer and the scaling for
//     the next are ONE multiplication, done lazily right before the conversion, in the shadow of the previous MFMAs;
//   * |scaled activation| must stay below 65504 (fp16 max): the running maximum is tracked (one v_max3 per pair) and a
//     point that exceeds it gets NaN outputs -- loud, like the encoder's domain check -- instead of an inf/NaN soup.
// Measured on the 8x256 MLP (tests/test_host_logic.py::test_f16x2_split_is_fp32_grade): error against fp64 0.5-0.7x
// that of a numpy fp32 GEMM chain.
//
// Stream: the SAME size and segment order as the fp32 x32 stream (145 slabs per pass: 2 fp16 pieces = 4 bytes per weight).
// A chunk (1 KiB, one ds_read_b128 per lane) is the A fragment -- 32 rows x 16 k -- of ONE piece of ONE (k16 block, output
// block) pair; step s of a k16 block = 4 chunks = [hi(2s), hi(2s+1), lo(2(s^1)), lo(2(s^1)+1)] = 6 MFMAs on four different
// accumulators; a k16 block of an 8-block layer is 4 steps = one slab, of the 4-block views layer 2 steps.  K order as in nsr_b3.inc: slot i
// of k16 block kb is k-step 8 kb + i of the fp32 x32 layout for both lane halves (kappa / eps tables shared).
// slabs of a backward pass (transposed fine network): views^T enc 2 + 8 | feature^T 16 | L7^T L6^T 32 | L5^T enc 4 + 16 |
// L4^T..L1^T 64 | L0^T enc 4.  The encoding rows of the fp32 stream's 9-, 10- and 2-block segments are 2-block GEMMs here.
constexpr int kStreamSlabsH2Bwd = 146;


typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct H2 { u32x4 hi, lo; };          // this lane's 8 k-slots of one k16 block: packed fp16 pairs

constexpr float kH2Max = 65504.0f * (1.0f - 1.0f / 4096.0f);     // largest |scaled value| that still rounds to a finite fp16

// The split of one packed pair (slots 2j, 2j+1 of a block): scale, round to fp16 (RNE), residual (exact in fp32), round
// again -- as FOUR STAGES of one or two instructions each, so that the caller can put one stage into each MFMA gap.
// In-order issue is why: a dependent chain of five VALU instructions between two MFMAs holds the wave's issue slot for
// about as long as the matrix pipe needs for one MFMA, one or two independent instructions per gap do not (measured: +1 %
// over the same instructions as one block per step; the kernel is power-bound, most of a cycle saving returns as clock).
// The mixed-precision FMAs do scale + convert (v_fma_mixlo/hi_f16: fp16(x * m + 0) into one half of the destination) and
// scale + residual (v_fma_mix_f32: x * m - float(half), a single exact operation) in one instruction each -- four
// instructions where plain C compiles to eight (2 v_mul, v_cvt_pk, 2 v_cvt_f32_f16, 2 v_sub; there is no builtin for them).
// amax: running max of the UNSCALED magnitudes (one v_max3_f32); the caller multiplies by the scale once per GEMM.
struct H2Job {
  float xa, xb, m;
  unsigned hi;
  float ra, rb;
};
__device__ __forceinline__ void h2_stage0(H2Job& q) {
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(q.hi) : "v"(q.xa), "v"(q.m));
}
__device__ __forceinline__ void h2_stage1(H2Job& q, float& amax) {
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(q.hi) : "v"(q.xb), "v"(q.m));
  asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(q.xa), "v"(q.xb));
}
__device__ __forceinline__ void h2_stage2(H2Job& q) {
  asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(q.ra) : "v"(q.xa), "v"(q.m), "v"(q.hi));
  asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(q.rb) : "v"(q.xb), "v"(q.m), "v"(q.hi));
}
__device__ __forceinline__ void h2_stage3(const H2Job& q, int j, H2& r) {
  const f16x2 lo = __builtin_convertvector(f32x2{q.ra, q.rb}, f16x2);                            // v_cvt_pk_f16_f32 (RNE)
  r.hi[j] = q.hi;
  r.lo[j] = __builtin_bit_cast(unsigned, lo);
}
// all four stages back to back (the first block of a GEMM, split before its first MFMA)
__device__ __forceinline__ void split_pair_h2(float xa, float xb, float m, int j, H2& r, float& amax) {
  H2Job q{xa, xb, m, 0u, 0.0f, 0.0f};
  h2_stage0(q); h2_stage1(q, amax); h2_stage2(q); h2_stage3(q, j, r);
}

__device__ __forceinline__ f32x16 mfma_h2(f32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// the pieces of ring_issue, so that the DMA issue of a slab change can be spread over MFMA gaps
template <int C0>
__device__ __forceinline__ void ring_issue_dma(Ring& rg) {          // chunks C0, C0 + 1 of the slab being issued
  char* l = rg.smem + rg.pslot * kSlabBytes + rg.wave_lds;
  const int soff = rg.pnet_off + rg.pslab * kSlabBytes;
#ifndef NSR_EXP_NODMA
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rg.rsrc, (__attribute__((address_space(3))) void*)l, 16, rg.lane_off, soff,
                                           C0 * 1024, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rg.rsrc, (__attribute__((address_space(3))) void*)l, 16, rg.lane_off, soff,
                                           (C0 + 1) * 1024, 0);
#endif
}
template <int C>
__device__ __forceinline__ void ring_issue_dma1(Ring& rg) {         // chunk C alone
  char* l = rg.smem + rg.pslot * kSlabBytes + rg.wave_lds;
  const int soff = rg.pnet_off + rg.pslab * kSlabBytes;
#ifndef NSR_EXP_NODMA
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rg.rsrc, (__attribute__((address_space(3))) void*)l, 16, rg.lane_off, soff,
                                           C * 1024, 0);
#endif
}
template <int NS, int SLABS, int SLABS_BWD>
__device__ __forceinline__ void ring_issue_advance(Ring& rg) {
  rg.pslot = (rg.pslot + 1 == NS) ? 0 : rg.pslot + 1;
  const int nslab = rg.pslab + 1;
  const bool wrap = nslab == ((SLABS_BWD != SLABS && rg.pphase >= rg.pn1) ? SLABS_BWD : SLABS);
  rg.pslab = wrap ? 0 : nslab;
  const int nphase = (rg.pphase + 1 == rg.ppi) ? 0 : rg.pphase + 1;
  rg.pphase = wrap ? nphase : rg.pphase;
  const int net = rg.pphase < rg.pn0 ? 0 : (rg.pphase < rg.pn1 ? 1 : 2);
  rg.pnet_off = net * (int)rg.stride;
}

// ring_issue_advance in two halves (about eight scalar instructions each), for two different MFMA gaps
template <int NS, int SLABS, int SLABS_BWD>
__device__ __forceinline__ bool ring_issue_advance_a(Ring& rg) {
  rg.pslot = (rg.pslot + 1 == NS) ? 0 : rg.pslot + 1;
  const int nslab = rg.pslab + 1;
  const bool wrap = nslab == ((SLABS_BWD != SLABS && rg.pphase >= rg.pn1) ? SLABS_BWD : SLABS);
  rg.pslab = wrap ? 0 : nslab;
  return wrap;
}
__device__ __forceinline__ void ring_issue_advance_b(Ring& rg, bool wrap) {
  const int nphase = (rg.pphase + 1 == rg.ppi) ? 0 : rg.pphase + 1;
  rg.pphase = wrap ? nphase : rg.pphase;
  const int net = rg.pphase < rg.pn0 ? 0 : (rg.pphase < rg.pn1 ? 1 : 2);
  rg.pnet_off = net * (int)rg.stride;
}

// One step: fragments A[0..3] = hi(HB), hi(HB+1), lo(LB), lo(LB+1) -- the hi pieces of one pair of output blocks and the
// lo pieces of ANOTHER pair (step s of a k16 block: HB = 2s, LB = 2(s^1); the partner step has them the other way round) --
// six MFMAs in the order hi(HB) bl, hi(HB+1) bl, lo(LB) bh, lo(LB+1) bh, hi(HB) bh, hi(HB+1) bh: an accumulator recurs no
// sooner than three MFMAs later, within a step and across steps (GEMM cycles -4 % against two accumulators alternating --
// given back as clock: DESIGN.md 4).  The instruction order is written out BY HAND -- every statement group is pinned (sched_barrier) -- one
// MFMA, then at most one LDS fragment read for the next step and one stage of the split of NP packed pairs of the NEXT
// k16 block (jobs).  G = the step's index within its slab; in the slab's last step (G = 3) the counted wait + barrier,
// the next slab's first fragment reads and the LDS-DMA issue of slab n + NS take the places of the fragment reads.
template <int NS, int G, int NP, bool ACT_, bool ZH = false, bool ZL = false, int NACC>
__device__ __forceinline__ void step_h2(Ring& rg, f32x4 (&Acur)[4], f32x4 (&Anxt)[4], const H2& b, f32x16 (&acc)[NACC],
                                        int HB, int LB /* constants after unrolling */, int lane, H2Job (&job)[NP], int j0,
                                        H2& bn, float& amax) {
  const char* p = rg.smem + rg.cslot * kSlabBytes + (G + 1) * kStepBytes + lane * 16;      // next step's fragments (G < 3)
#ifdef NSR_EXP_H2_NOSPLIT      // timing experiments only (results are wrong)
  constexpr bool ACT = false;
  if (ACT_) { bn = b; }
#else
  constexpr bool ACT = ACT_;
#endif
#ifdef NSR_EXP_H2_NOFRAG
#define NSR_H2_FRAG(i, off) do { } while (0)
#else
#define NSR_H2_FRAG(i, off) Anxt[i] = *(const f32x4*)(p + (off))
#endif
  // slab change (G == 3): nothing but the counted wait and the barrier sits between two MFMAs -- the matrix pipe holds one
  // MFMA, so every instruction in that window is an idle pipe (measured: the window cost ~100 of a slab's 768 cycles
  // when the next slab's four fragment reads, the DMA address arithmetic and two DMA issues sat in it)
#ifdef NSR_EXP_NODMA
#define NSR_H2_DMA(C) do { } while (0)
#define NSR_H2_DMA1(C) do { } while (0)
#else
#define NSR_H2_DMA(C) ring_issue_dma<C>(rg)
#define NSR_H2_DMA1(C) ring_issue_dma1<C>(rg)
#endif
  const char* pn = nullptr;                    // G == 3: the next slab's first fragments
  NSR_PIN();
  acc[HB] = mfma_h2(Acur[0], b.lo, ZH ? f32x16{0} : acc[HB]);       // ZH / ZL: first touch of a zero-initialised accumulator
  NSR_PIN();
  if (G != 3) NSR_H2_FRAG(0, 0);
#if NSR_H2_SCHED == 3
  // r05: ONE LDS-DMA piece per step, in a gap that carries no fragment read (an LDS-DMA issue holds the wave's issue port
  // for about as long as an MFMA holds the matrix pipe: two in one gap -- r03 / r04 -- leave the pipe idle for most of the
  // second one), and the ring's scalar bookkeeping in two halves.  The ring starts one slab short (ring_start<.., LAG = 1>),
  // so the slab whose pieces are issued during slab n is n + NS - 1, into the slot the barrier at the end of slab n - 1
  // freed; piece 3 goes out before this slab's counted wait, which therefore still allows 4 (NS - 2) younger pieces.
  // Measured (profiles/r05/extra/sched_ab.txt): GEMM cycles -6.3 %, clock -3.7 % (the kernel runs at the power limit: part
  // of every cycle saving is handed back as clock), kernel time -2.0 %, results bit-identical.
  else NSR_H2_DMA1(3);
#endif
  if (ACT) for (int u = 0; u < NP; ++u) h2_stage0(job[u]);
  NSR_PIN();
  acc[HB + 1] = mfma_h2(Acur[1], b.lo, ZH ? f32x16{0} : acc[HB + 1]);
  NSR_PIN();
  if (G != 3) NSR_H2_FRAG(1, 1024);
  if (ACT) for (int u = 0; u < NP; ++u) h2_stage1(job[u], amax);
  if (G == 3) {
    NSR_PIN();
    // all of this wave's reads of the current slab are complete after lgkmcnt(0); my share of the next slab has landed
    // after the counted vmcnt; the barrier makes both true for the whole workgroup
#ifdef NSR_EXP_NOVMWAIT         // timing experiment (results may be wrong): what the counted vmcnt wait costs
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(4 * (NS - 2)) : "memory");
#endif
#ifdef NSR_EXP_H2_HALFBARRIER      // timing experiment (results may be wrong): a barrier at every other slab change only =
    if (rg.cslot & 1)              // what 32 KiB slabs would leave of the barriers, with the DMA issue unchanged
#endif
#ifndef NSR_EXP_NOBARRIER
    __builtin_amdgcn_s_barrier();
#endif
    rg.cslot = (rg.cslot + 1 == NS) ? 0 : rg.cslot + 1;
    pn = rg.smem + rg.cslot * kSlabBytes + lane * 16;
  }
  NSR_PIN();
  acc[LB] = mfma_h2(Acur[2], b.hi, ZL ? f32x16{0} : acc[LB]);
  NSR_PIN();
  if (G != 3) NSR_H2_FRAG(2, 2048);
  else { Anxt[0] = *(const f32x4*)(pn); if (NSR_H2_SCHED != 3) NSR_H2_DMA(0); }
  if (ACT) for (int u = 0; u < NP; ++u) h2_stage2(job[u]);
  NSR_PIN();
  acc[LB + 1] = mfma_h2(Acur[3], b.hi, ZL ? f32x16{0} : acc[LB + 1]);
  NSR_PIN();
  if (G != 3) NSR_H2_FRAG(3, 3072);
  else { Anxt[1] = *(const f32x4*)(pn + 1024); if (NSR_H2_SCHED != 3) NSR_H2_DMA(2); }
  if (ACT) for (int u = 0; u < NP; ++u) h2_stage3(job[u], j0 + u, bn);
  NSR_PIN();
  acc[HB] = mfma_h2(Acur[0], b.hi, acc[HB]);
  NSR_PIN();
#if NSR_H2_SCHED == 3
  if (G == 0) NSR_H2_DMA1(0);
  if (G == 1) NSR_H2_DMA1(1);
  if (G == 2) NSR_H2_DMA1(2);
#endif
#if NSR_H2_SCHED == 3
  bool wrapped = false;
  if (G == 3) { Anxt[2] = *(const f32x4*)(pn + 2048); wrapped = ring_issue_advance_a<NS, kStreamSlabs, kStreamSlabsH2Bwd>(rg); }
#else
  if (G == 3) { Anxt[2] = *(const f32x4*)(pn + 2048); ring_issue_advance<NS, kStreamSlabs, kStreamSlabsH2Bwd>(rg); }
#endif
  NSR_PIN();
  acc[HB + 1] = mfma_h2(Acur[1], b.hi, acc[HB + 1]);
  NSR_PIN();
  if (G == 3) Anxt[3] = *(const f32x4*)(pn + 3072);
#if NSR_H2_SCHED == 3
  if (G == 3) ring_issue_advance_b(rg, wrapped);
#endif
#undef NSR_H2_DMA
#undef NSR_H2_DMA1
#undef NSR_H2_FRAG
}

// ---- the tail of a layer GEMM: the LAST k16 block with the layer's epilogue in its MFMA gaps ----------------------------
// Between two layer GEMMs sit the epilogue in = clamp(acc) (the accumulators live in AGPRs: one v_accvgpr_read and one
// v_max_i32 per value, 256 instructions) and the next layer's bias load (32 ds_read_b128).  With one wave per SIMD nothing
// covers them: the matrix pipe idles for every one of their issue cycles, while the gaps between the last 24 MFMAs of the
// GEMM are empty (the last block has no next block to split).  So the last block of an 8-output-block GEMM -- always one
// whole slab, steps g = 0..3 -- gets an order of its own in which accumulators become FINAL one after another,
//     MFMA  0  1  2  3  4  5  6* 7* 8* 9 10 11 12 13 14 15* 16* 17 18 19 20 21* 22* 23*        (* = last MFMA of that
//     acc   0  1  2  0  1  2  0  1  2  3  4  5  3  4  6  3   4   7  5  6  7  5   6   7          accumulator)
// and whatever is final is clamped into in[] (dead by now: the last block was split during the one before) and re-loaded
// with the next layer's bias in the gaps that follow.  What the order keeps:
//   * per accumulator the three MFMAs of the block come in the order they have in step_h2 (even pairs: hi.bl, hi.bh, lo.bh;
//     odd pairs: lo.bh, hi.bl, hi.bh) -- the fp32 accumulation order, hence every bit of the result;
//   * an accumulator recurs no sooner than three MFMAs later (which is also why no order retires much earlier: any three
//     consecutive MFMAs go to three different accumulators, so the last three end at 21, 22, 23 whatever one does);
//   * the slab's chunk layout (chunk c of the slab = step c / 4, fragment c % 4 of step_h2) -- only the read order differs;
//   * the slab-change duties of step G = 3 at the MFMAs they had: one LDS-DMA piece after MFMA 4, 10, 16, 18, the counted
//     wait + barrier after MFMA 19 (every read of this slab has been issued by then: the chunks of the last four MFMAs
//     sit in A1), the next slab's first fragments into A0 after MFMA 20..23;
//   * a gap carries a fragment read or a DMA piece or bias reads, never two of them.
// The accumulators 0..4 are clamped inside the block (160 instructions) and 0 and half of 1 re-loaded; accumulators 5, 6, 7
// retire with the last three MFMAs: their 96 clamp instructions and the 26 bias reads that are left stay behind the last MFMA
// (137 instructions with the ring's scalar bookkeeping) and the split of the next layer's first block before the next first
// MFMA (35) -- 172 per layer where 482 stood (tools/isa_mix.py; measured -2.6 % kernel time, profiles/r07/ab_epilogue.txt).
struct H2Tail {
  f32x16 (&acc)[8];
  f32x16 (&in)[8];
  int thr;                 // clamp_bits16 threshold of this layer: 0 = relu, INT_MIN = none
  unsigned bias;           // LDS byte address of this lane's half of the NEXT layer's bias (aux layout, load_bias)
  __device__ __forceinline__ void clamp(int k, int q) const {           // a quarter of accumulator k
#pragma unroll
    for (int r = 4 * q; r < 4 * q + 4; ++r) in[k][r] = __int_as_float(max(__float_as_int(acc[k][r]), thr));
  }
  __device__ __forceinline__ void load(int k, int rq) const {            // a quarter of the next bias into accumulator k
    const f32x4 v = *(const __attribute__((address_space(3))) f32x4*)(bias + (k * 4 + rq) * 32);
    acc[k][rq * 4 + 0] = v[0];
    acc[k][rq * 4 + 1] = v[1];
    acc[k][rq * 4 + 2] = v[2];
    acc[k][rq * 4 + 3] = v[3];
  }
};
// the LDS address of p + h4 as ONE opaque per-lane register: every access through it is base + immediate offset (the aux
// block sits above 64 KiB, beyond the reach of a ds offset from the LDS base: without this each read gets a v_add of its own)
__device__ __forceinline__ unsigned h2_lds_base(const float* p, int h4) {
  return (unsigned)opaque_v((int)(unsigned)(size_t)(const __attribute__((address_space(3))) float*)(p + h4));
}

template <int NS, typename Tail>
__device__ __forceinline__ void tail_h2(Ring& rg, f32x4 (&A0)[4], f32x4 (&A1)[4], const H2& b, f32x16 (&acc)[8], int lane,
                                        const Tail& t) {
  const char* p = rg.smem + rg.cslot * kSlabBytes + lane * 16;          // A0 holds chunks 0..3 of this slab
#define NSR_T_MFMA(k, frag, bop) NSR_PIN(); acc[k] = mfma_h2(frag, b.bop, acc[k]); NSR_PIN()
#define NSR_T_READ(dst, c) dst = *(const f32x4*)(p + (c) * 1024)
  // chunks: 0 hi0, 1 hi1, 2 lo2, 3 lo3 | 4 hi2, 5 hi3, 6 lo0, 7 lo1 | 8 hi4, 9 hi5, 10 lo6, 11 lo7 | 12 hi6, 13 hi7, 14 lo4, 15 lo5
  NSR_T_MFMA(0, A0[0], lo); NSR_T_READ(A1[0], 4);
  NSR_T_MFMA(1, A0[1], lo); NSR_T_READ(A1[1], 6);
  NSR_T_MFMA(2, A0[2], hi); NSR_T_READ(A1[2], 7);
  NSR_T_MFMA(0, A0[0], hi); NSR_T_READ(A1[3], 8);
  NSR_T_MFMA(1, A0[1], hi); ring_issue_dma1<0>(rg);
  NSR_T_MFMA(2, A1[0], lo); NSR_T_READ(A0[2], 9);
  NSR_T_MFMA(0, A1[1], hi); NSR_T_READ(A0[0], 5);                                     // 0 final
  NSR_T_MFMA(1, A1[2], hi); NSR_T_READ(A0[1], 10);                                    // 1 final
  NSR_T_MFMA(2, A1[0], hi); NSR_T_READ(A1[1], 14); t.clamp(0, 0); t.clamp(0, 1);      // 2 final
  NSR_T_MFMA(3, A0[3], hi); NSR_T_READ(A1[2], 11); t.clamp(0, 2); t.clamp(0, 3);
  NSR_T_MFMA(4, A1[3], lo); ring_issue_dma1<1>(rg); t.clamp(1, 0); t.clamp(1, 1);
  NSR_T_MFMA(5, A0[2], lo); NSR_T_READ(A1[0], 12); t.clamp(1, 2); t.clamp(1, 3);
  NSR_T_MFMA(3, A0[0], lo); t.clamp(2, 0); t.clamp(2, 1); t.load(0, 0); t.load(0, 1);
  NSR_T_MFMA(4, A1[3], hi); t.clamp(2, 2); t.clamp(2, 3); t.load(0, 2); t.load(0, 3);
  NSR_T_MFMA(6, A0[1], hi); t.load(1, 0); t.load(1, 1);
  NSR_T_MFMA(3, A0[0], hi); NSR_T_READ(A1[3], 13);                                    // 3 final
  NSR_T_MFMA(4, A1[1], hi); ring_issue_dma1<2>(rg);                                   // 4 final
  NSR_T_MFMA(7, A1[2], hi); NSR_T_READ(A1[1], 15); t.clamp(3, 0); t.clamp(3, 1);
  NSR_T_MFMA(5, A0[2], hi); ring_issue_dma1<3>(rg); t.clamp(3, 2); t.clamp(3, 3);
  NSR_T_MFMA(6, A1[0], lo);
  // as in step_h2, G == 3: every read of this slab is complete, my share of the next slab has landed, for the whole workgroup
#ifdef NSR_EXP_NOVMWAIT
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(4 * (NS - 2)) : "memory");
#endif
#ifndef NSR_EXP_NOBARRIER
  __builtin_amdgcn_s_barrier();
#endif
  rg.cslot = (rg.cslot + 1 == NS) ? 0 : rg.cslot + 1;
  p = rg.smem + rg.cslot * kSlabBytes + lane * 16;
  NSR_T_MFMA(7, A1[3], lo); NSR_T_READ(A0[0], 0); t.clamp(4, 0); t.clamp(4, 1);
  NSR_T_MFMA(5, A1[1], hi); NSR_T_READ(A0[1], 1); t.clamp(4, 2); t.clamp(4, 3);      // 5 final
  NSR_T_MFMA(6, A1[0], hi); NSR_T_READ(A0[2], 2);                                     // 6 final
  const bool wrapped = ring_issue_advance_a<NS, kStreamSlabs, kStreamSlabsH2Bwd>(rg);
  NSR_T_MFMA(7, A1[3], hi); NSR_T_READ(A0[3], 3);                                     // 7 final
  ring_issue_advance_b(rg, wrapped);
  NSR_PIN();
  // what does not fit: the rest of the bias of 1, the bias of 2, 3, 4 and all of 5, 6, 7
  t.load(1, 2); t.load(1, 3);
#pragma unroll
  for (int k = 2; k < 8; ++k) {
    if (k >= 5) { t.clamp(k, 0); t.clamp(k, 1); t.clamp(k, 2); t.clamp(k, 3); }
    t.load(k, 0); t.load(k, 1); t.load(k, 2); t.load(k, 3);
  }
#undef NSR_T_READ
#undef NSR_T_MFMA
}

// The power of two a k16 block's values are multiplied with before the split: m[0] for blocks < split, m[1] from there on
// (the views layer reads 16 blocks of scaled registers and 2 of unscaled direction encoding); split >= NKB: one scale.
struct H2Scale {
  float m[2];
  int split;
  __device__ __forceinline__ float operator()(int kb) const { return kb < split ? m[0] : m[1]; }
};

// A whole GEMM over NKB k16 blocks.  src(kb, i) = this lane's fp32 value in slot i of k16 block kb (constant indices after
// unrolling).  Block 0 is split up front, every following block stage by stage in the MFMA gaps of the block before it (one
// packed pair per step for NMO = 8, two for NMO = 4, all four for NMO = 2).  ZERO: the accumulators start from 0 (the first
// MFMA that touches one takes the constant 0 as its C operand).  NMO = 2 (the encoding rows of the transposed network): a
// step is [hi(0), hi(1), lo(0), lo(1)], one step per k16 block, four k16 blocks per slab.
// amax: running max of |scaled value| over everything this lane has split.
template <int NMO, int NKB, bool ZERO = false, int NACC, typename Src>
__device__ __forceinline__ void gemm_h2(Ring& rg, f32x4 (&A0)[4], f32x4 (&A1)[4], Src src, const H2Scale scale,
                                        f32x16 (&acc)[NACC], int lane, float& amax) {
  static_assert(NMO == 8 || NMO == 4 || NMO == 2, "8, 4 or 2 output blocks");
  static_assert((NKB * NMO) % 8 == 0, "a GEMM is a whole number of slabs");
  constexpr int SPB = NMO / 2;                     // steps per k16 block
  constexpr int NP = 4 / SPB;                      // packed pairs split per step
  float am[2] = {0.0f, 0.0f};                      // per scale class, unscaled
  H2 b;
#pragma unroll
  for (int j = 0; j < 4; ++j) split_pair_h2(src(0, 2 * j), src(0, 2 * j + 1), scale(0), j, b, am[0 >= scale.split]);
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) {
    H2 bn;
    const bool more = kb + 1 < NKB;
    const int cls = more && (kb + 1 >= scale.split);
#pragma unroll
    for (int s = 0; s < SPB; ++s) {
      H2Job job[NP];
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        const int j = NP * s + u;
        job[u] = H2Job{more ? src(kb + 1, 2 * j) : 0.0f, more ? src(kb + 1, 2 * j + 1) : 0.0f, more ? scale(kb + 1) : 0.0f, 0u, 0.0f, 0.0f};
      }
      const int g = (kb * SPB + s) & 3;            // step index within the slab
      const int hb = 2 * s, lb = NMO == 2 ? 0 : 2 * (s ^ 1);
      // zero-initialised accumulators are first touched in the first k16 block: as hi blocks in even steps, as lo blocks
      // of their partner step (also even); with NMO = 2 the hi MFMAs of the only step come first
      const bool zh = ZERO && kb == 0 && (s & 1) == 0, zl = ZERO && kb == 0 && (s & 1) == 0 && NMO != 2;
#define NSR_H2_STEP(GG, AC, AN, ACTV, ZHV, ZLV) \
  step_h2<kRingSlots, GG, NP, ACTV, ZHV, ZLV>(rg, AC, AN, b, acc, hb, lb, lane, job, NP * s, bn, am[ACTV ? cls : 0])
#define NSR_H2_STEP_Z(GG, AC, AN, ACTV)                              \
  do {                                                               \
    if (zh && zl) NSR_H2_STEP(GG, AC, AN, ACTV, true, true);         \
    else if (zh) NSR_H2_STEP(GG, AC, AN, ACTV, true, false);         \
    else NSR_H2_STEP(GG, AC, AN, ACTV, false, false);                \
  } while (0)
      if (more) {
        if (g == 0) NSR_H2_STEP_Z(0, A0, A1, true);
        if (g == 1) NSR_H2_STEP_Z(1, A1, A0, true);
        if (g == 2) NSR_H2_STEP_Z(2, A0, A1, true);
        if (g == 3) NSR_H2_STEP_Z(3, A1, A0, true);
      } else {
        if (g == 0) NSR_H2_STEP_Z(0, A0, A1, false);
        if (g == 1) NSR_H2_STEP_Z(1, A1, A0, false);
        if (g == 2) NSR_H2_STEP_Z(2, A0, A1, false);
        if (g == 3) NSR_H2_STEP_Z(3, A1, A0, false);
      }
#undef NSR_H2_STEP_Z
#undef NSR_H2_STEP
    }
    if (more) b = bn;
  }
  NSR_PIN();
  amax = __builtin_fmaxf(amax, __builtin_fmaxf(am[0] * scale.m[0], am[1] * scale.m[1]));
}

// gemm_h2 for an 8-output-block layer whose LAST k16 block runs as tail_h2: the layer's epilogue and the next layer's bias
// load in its MFMA gaps (tail: H2Tail).  A function of its own, so that gemm_h2 -- the input-gradient kernels use nothing
// else -- stays the text it was.  Every k16 block is one whole slab (steps g = 0..3); the accumulators come with their bias.
template <int NKB, typename Src, typename Tail>
__device__ __forceinline__ void gemm_h2_tail(Ring& rg, f32x4 (&A0)[4], f32x4 (&A1)[4], Src src, const H2Scale scale,
                                             f32x16 (&acc)[8], int lane, float& amax, const Tail tail) {
  static_assert(NKB > 1, "the last block is not the first");
  float am[2] = {0.0f, 0.0f};                      // per scale class, unscaled
  H2 b;
#pragma unroll
  for (int j = 0; j < 4; ++j) split_pair_h2(src(0, 2 * j), src(0, 2 * j + 1), scale(0), j, b, am[0 >= scale.split]);
#pragma unroll
  for (int kb = 0; kb + 1 < NKB; ++kb) {
    H2 bn;
    const int cls = kb + 1 >= scale.split;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      H2Job job[1] = {H2Job{src(kb + 1, 2 * s), src(kb + 1, 2 * s + 1), scale(kb + 1), 0u, 0.0f, 0.0f}};
      const int hb = 2 * s, lb = 2 * (s ^ 1);
#define NSR_H2_STEP(GG, AC, AN) step_h2<kRingSlots, GG, 1, true, false, false>(rg, AC, AN, b, acc, hb, lb, lane, job, s, bn, am[cls])
      if (s == 0) NSR_H2_STEP(0, A0, A1);
      if (s == 1) NSR_H2_STEP(1, A1, A0);
      if (s == 2) NSR_H2_STEP(2, A0, A1);
      if (s == 3) NSR_H2_STEP(3, A1, A0);
#undef NSR_H2_STEP
    }
    b = bn;
  }
  tail_h2<kRingSlots>(rg, A0, A1, b, acc, lane, tail);
  NSR_PIN();
  amax = __builtin_fmaxf(amax, __builtin_fmaxf(am[0] * scale.m[0], am[1] * scale.m[1]));
}
