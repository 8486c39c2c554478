// nsr_wide_gemm.inc -- the layered renderer's GEMM: ONE kernel body, gemm_split_body<NJ, EPI, WM, NP>, for its three arithmetics
// -- kw_gemm_b3 (NP = 3, "bf16x3"), kw_gemm_h2 (NP = 2, "f16x2") and kw_gemm_f32 (NP = 1, strict fp32).  Included inside namespace
// nsrw (nsr_wide.hip), after the epilogue enums.  The bf16x3 form came first and is described first; what the other two change is
// said where they are defined below.
//
// C[m][n] = epi( sum_k A[m][k] W[n][k] + bias[n] ), fp32 in HBM on both sides.  bf16x3: the products run
// on v_mfma_f32_32x32x16_bf16: every fp32 value is the exact sum of three bf16 pieces x = x0 + x1 + x2; of the nine piece
// products of a * w the six of weight >= 2^-16 are kept (a0w0 a0w1 a0w2 a1w0 a1w1 a2w0, each exact in the MFMA's product
// stage, fp32 accumulate) and the three below 2^-24 |a||w| are dropped -- the arithmetic of csrc/nsr_b3.inc, whose error
// against fp64 equals an fp32 GEMM chain's (tests/test_host_logic.py::test_bf16x3_split_is_fp32_grade), with fp32's exponent
// range: nothing to scale, no failure domain.  Six MFMAs of 32 matrix-pipe cycles per 32x32x16 block of products replace
// eight fp32 MFMAs of 64: 2.67x at the pipe, i.e. a ceiling of 2500 / 6 = 417 TFLOP/s of algorithmic work.
//
//   * weights: split on the host at upload (round-to-nearest pieces) into an image that IS the LDS image --
//     [col-block n / 32][k16 block][piece][64 lanes][8 bf16], lane l <-> (column 32 cb + l % 32, k = 16 kb + 8 (l / 32) ..+7),
//     1 KiB per (col-block, k16 block, piece) = one B fragment -- and moved by LDS-DMA (buffer_load_dwordx4 ... lds): no
//     register round trip, no VALU, one scalar offset per instruction;
//   * activations: fp32 rows in HBM (4 bytes per value, what the producing epilogue wrote).  A workgroup's thread loads the
//     8 consecutive k of ONE row that are one lane's share of an A fragment, splits them (truncation pieces: two ANDs, two exact
//     SUBs and a V_PERM per packed pair, 44 VALU per thread and stage in the shadow of 48 MFMAs) and writes the three 16-byte
//     pieces lane-linearly: the staging writes and the fragment reads (ds_read_b128 at base + 16 lane) are conflict-free by
//     construction, no padding, no swizzle;
//   * tile 128 (M) x 64 NJ (N), NJ = 4 | 2 | 1; 256 threads = 4 waves as 2 x 2, a wave owns 64 x 32 NJ = 2 x NJ accumulator
//     blocks (128 registers at NJ = 4); K advances one k16 block per stage through double-buffered LDS (36 KiB per stage at
//     NJ = 4: two workgroups per CU, two waves per SIMD), ONE barrier per stage = per 12 NJ MFMAs of a wave.  Per stage a wave
//     reads 6 + 3 NJ fragments for 12 NJ MFMAs (384 B per MFMA at NJ = 4);
//   * persistent workgroups walk the tiles in an XCD-aware order (the N-tiles of one M-block go to ONE XCD back to back), K runs
//     over two segments ([A1 | A2], the skip concatenations), the rows of a ragged last M-block are clamped on the way in and
//     never stored.
#undef NSRW_FILE_TAG
#define NSRW_FILE_TAG 100000        /* a failed NSRW_CHECK of this file reports 100000 + its line (nsrw_debug_bounds_status) */
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct GemmArgs {
  const float* A1; const float* A2;
  const char* Wb;                          // weight image of the launch's arithmetic, from the first col-block of this launch on
  const float* bias; float* C; const float* mask;
  long long M;
  int lda1, lda2, K1, K2;                  // K extents, multiples of 32 (so of 16)
  int ldc, N, ldm, n_tiles;
  unsigned wb_bytes;                       // bytes of the image from Wb on (bounds of the DMA's buffer descriptor)
  float cscale;                            // f16x2: 2^-sw, the weight scale of this matrix undone in the epilogue (bf16x3: 1)
  unsigned* range_flag;                    // f16x2: set when an activation leaves fp16's range (the caller re-runs the pass on bf16x3)
  const unsigned* run_if;                  // nullable: the launch does nothing unless *run_if != 0 (the bf16x3 re-run of such a pass)
  // the row-granular re-run (NSRW_FLAG_RERUN_ROWS; the *_rows kernels below read these, the others never do):
  unsigned* row_words;                     // [n_words] one bit per row of the pass, word = row / 32, bit = row % 32: f16x2 sets, bf16x3 reads
  const int* row_list;                     // bf16x3: [0] how many M-blocks of this launch's tile height hold a flagged row, [1 ..] which (kw_rows_list)
  int n_words, list_max;                   // (M + 31) / 32; entries the list has room for
};

constexpr unsigned kPermHi16 = 0x07060302u;          // V_PERM_B32(y, x): {y.hi16, x.hi16}

#define NSRW_SGB(mask, n) __builtin_amdgcn_sched_group_barrier((mask), (n), 0)
#define NSRW_MASK_VALU 0x002
#define NSRW_MASK_MFMA 0x008
#define NSRW_MASK_DSRD 0x100
#define NSRW_MASK_DSWR 0x200

// the LDS-DMA of piece P of one fragment image chunk (1 KiB a piece: 64 lanes x 16 bytes): from byte `soff` (uniform) of the buffer
// behind `rsrc` to the LDS address `l`; the immediate offsets BOTH the source and the LDS address.  The weight stages of
// gemm_split_body and of the on-chip kernels (nsr_wide_trunk.inc) are made of it.
#define NSRW_DMA(rsrc, l, lane, soff, P)                                                                                  \
  __builtin_amdgcn_raw_ptr_buffer_load_lds((rsrc), (__attribute__((address_space(3))) void*)(l), 16, (lane) * 16, (soff), \
                                           (P) * 1024, 0)

// 8 fp32 -> three pieces of 8 bf16 (packed pairs, k ascending); exact: x == p0 + p1 + p2
__device__ __forceinline__ void split8_b3(const f32x4& lo, const f32x4& hi, u32x4 (&p)[3]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float xa = j < 2 ? lo[2 * j] : hi[2 * j - 4], xb = j < 2 ? lo[2 * j + 1] : hi[2 * j - 3];
    const unsigned a0 = __builtin_bit_cast(unsigned, xa), b0 = __builtin_bit_cast(unsigned, xb);
    const float ra = xa - __builtin_bit_cast(float, a0 & 0xffff0000u);       // exact: <= 16 significant bits
    const float rb = xb - __builtin_bit_cast(float, b0 & 0xffff0000u);
    const unsigned a1 = __builtin_bit_cast(unsigned, ra), b1 = __builtin_bit_cast(unsigned, rb);
    const float sa = ra - __builtin_bit_cast(float, a1 & 0xffff0000u);       // exact: <= 8 significant bits = a bf16
    const float sb = rb - __builtin_bit_cast(float, b1 & 0xffff0000u);
    p[0][j] = __builtin_amdgcn_perm(b0, a0, kPermHi16);
    p[1][j] = __builtin_amdgcn_perm(b1, a1, kPermHi16);
    p[2][j] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, sb), __builtin_bit_cast(unsigned, sa), kPermHi16);
  }
}

__device__ __forceinline__ f32x16 mfma_b3(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- f16x2 (r06): the same kernel with every fp32 operand as TWO fp16 pieces and three piece products (csrc/nsr_h2.inc has the
// arithmetic and its error analysis: x0 = fp16(x) RNE, x1 = fp16(x - x0), a0w0 + a0w1 + a1w0, |error| <= 2^-22 |a||w|; the fused
// default kernel k_render_h2 computes with it).  Half the MFMAs of bf16x3, two thirds of its LDS and LDS-DMA bytes.  The price is
// fp16's RANGE: weights are stored scaled by 2^sw (largest entry just below 2^15; undone by cscale in the epilogue), activations
// go in as they are, and one whose magnitude reaches 65504 sets *range_flag -- the host side then runs the same network pass
// again on bf16x3 (launches that return at once when the flag is clear: stream-ordered, capturable, no host round trip).
typedef _Float16 f16x8w __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2w __attribute__((ext_vector_type(2)));
typedef float f32x2w __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void split8_h2(const f32x4& lo, const f32x4& hi, u32x4 (&p)[2], float& amax) {
  const float one = 1.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float xa = j < 2 ? lo[2 * j] : hi[2 * j - 4], xb = j < 2 ? lo[2 * j + 1] : hi[2 * j - 3];
    const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2w{xa, xb}, f16x2w));       // v_cvt_pk_f16_f32 (RNE)
    float ra, rb;                                                                      // x - float(half): one exact operation each
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(ra) : "v"(xa), "v"(one), "v"(h));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(rb) : "v"(xb), "v"(one), "v"(h));
    asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(amax) : "v"(xa), "v"(xb));
    p[0][j] = h;
    p[1][j] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2w{ra, rb}, f16x2w));
  }
}

__device__ __forceinline__ f32x16 mfma_h2w(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8w, a), __builtin_bit_cast(f16x8w, b), c, 0, 0, 0);
}

// WM: wave rows of a workgroup.  2: 256 threads, tile 128 x 64 NJ, two (NJ = 4) to four workgroups per CU.  4: 512 threads, tile
// 256 x 64 NJ, ONE workgroup per CU (the same two waves per SIMD) -- the weights' L2 -> LDS traffic per FLOP halves, which is
// what the ablations of profiles/r06/extra/ab_wide.txt price highest (this kernel runs at the board's power limit; time is energy).
template <int NJ, int WM> constexpr int wgs_per_cu() { return WM == 4 ? (NJ >= 3 ? 1 : 2) : NJ == 4 ? 2 : NJ == 2 ? 3 : 4; }

// NP: pieces per operand -- 3: bf16x3 (six products), 2: f16x2 (three products), 1: the STRICT fp32 mode (r06: v_mfma_f32_32x32x2_f32 on
// the same tiles, staging, prefetch and epilogues -- a fragment is then the lane's 8 consecutive fp32 k of a k16 block in two 16-byte
// chunks, no split at all; MFMA i of a block takes k = i from the lanes 0..31 and k = 8 + i from the lanes 32..63, the same
// permutation of a block's sixteen k on both operands; exact fp32 products, fp32 accumulate).  NPC: 16-byte chunks per lane of a fragment.
template <int NP> constexpr int split_chunks() { return NP == 1 ? 2 : NP; }
template <int NJ, int WM, int NP> constexpr int split_lds_bytes() { return 2 * (2 * WM + 2 * NJ) * split_chunks<NP>() * 1024; }

// ROWS: the row-granular re-run (DESIGN.md 8).  The bodies without it are what they were.
//   f16x2 (kBits): a lane stages the SAME row in every k16 block of a tile (am below), so the magnitude it has seen is that row's.  Per
//     tile, one ballot folded to 32 bits (both k halves of a row sit on lanes l and l + 32) and one atomicOr by one lane into the word of
//     the wave's 32 aligned rows, when it is non-zero; clamped rows set no bit; *range_flag is not touched (kw_rows_list sets it).
//     The A prefetch and astore run across tile boundaries -- the odd stage of a tile's LAST k pair splits the NEXT tile's stage 0 before
//     this tile's epilogue -- so there are TWO accumulators, amax (this tile's rows) and amax_nxt (the next tile's), and that one astore
//     goes to amax_nxt by a select on `last` (two v_cndmask around the stage: the steady state stays branch-free); the epilogue
//     folds amax, then amax = amax_nxt, amax_nxt = 0.
//   bf16x3 (kList): the M-blocks come from row_list -- position p of the XCD-aware walk is M-block row_list[1 + p], p < row_list[0], read
//     on the device -- and the epilogue stores / accumulates only the rows whose bit is set in row_words.  The other rows of a listed
//     tile are computed (from whatever their input rows hold) and dropped: rows do not mix.  A stored element's sum is the one of the
//     whole-pass bf16x3 kernel: k16 blocks ascending, the six products in their order.
template <int NJ, int EPI, int WM, int NP, bool ROWS = false>
__device__ __forceinline__ void gemm_split_body(const GemmArgs& g, char* const smem) {
  constexpr bool kBits = ROWS && NP == 2, kList = ROWS && NP == 3;
  static_assert(!ROWS || NP == 2 || NP == 3, "the row-granular re-run is f16x2's (bits) and bf16x3's (list)");
  constexpr int TN = 64 * NJ, NCB = 2 * NJ;                        // columns / col-blocks of a tile
  constexpr int kTM = 64 * WM, NW = 2 * WM;                        // rows of a tile / waves
  constexpr int NPC = split_chunks<NP>();
  constexpr int kFrag = NPC * 1024;                                // bytes of one fragment's pieces
  constexpr int kABytes = NW * kFrag, kBBytes = NCB * kFrag, kStage = kABytes + kBBytes;
  if (g.run_if && *g.run_if == 0u) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int KB = (g.K1 + g.K2) >> 4, KB1 = g.K1 >> 4;
  const int lrow = lane & 31, lh = lane >> 5;
  long long mblocks = (g.M + kTM - 1) / kTM;
  if constexpr (kList) {
    NSRW_CHECK(g.row_list[0] >= 0 && g.row_list[0] <= g.list_max && g.row_list[0] <= mblocks);
    mblocks = g.row_list[0];
  }
  const long long total = ((mblocks + 7) / 8) * 8 * g.n_tiles;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.Wb, 0, (int)g.wb_bytes, 0x00020000);

  struct Tile { long long m0; int n0; const float* a1p; const float* a2p; int wsrc; };
  auto coords = [&](long long t, Tile& tl) -> bool {               // the XCD-aware walk
    const int xcd = (int)(t & 7);
    const long long j = t >> 3;
    long long mb = (j / g.n_tiles) * 8 + xcd;
    if constexpr (kList) {                                         // mb is a list position: the XCD-aware order runs over those
      if (mb >= mblocks) return false;
      NSRW_CHECK(mb < g.list_max);
      mb = g.row_list[1 + mb];
      NSRW_CHECK(mb >= 0 && mb * kTM < g.M);
    }
    tl.m0 = mb * kTM;
    if (tl.m0 >= g.M) return false;
    tl.n0 = (int)(j % g.n_tiles) * TN;
    long long am = tl.m0 + 32 * wave + lrow;                       // wave w stages row-block w: lane = (row, k half)
    if (am >= g.M) am = g.M - 1;                                   // clamped rows are computed and never stored
    NSRW_CHECK(am >= 0 && am < g.M);
    tl.a1p = g.A1 + am * g.lda1 + 8 * lh;
    tl.a2p = g.A2 ? g.A2 + am * g.lda2 + 8 * lh : nullptr;
    tl.wsrc = (tl.n0 >> 5) * KB * kFrag;                            // byte offset of (first col-block of the tile, kb = 0)
    return true;
  };
  // A prefetch runs TWO stages ahead of the MFMAs (HBM latency under load is longer than one stage of 48 MFMAs), the
  // weights' LDS-DMA ONE stage (L2-resident); both run across tile boundaries, so a tile's first stage is in LDS and its
  // second in flight before the previous tile's epilogue starts.  ra[s]: the A values of the stages of parity s.
  // The steady state is BRANCH-FREE: what a stage fetches is chosen with selects (this tile's stage kb + 2, or the next tile's
  // stage 0 / 1; behind the last tile the fetches re-read this tile's first stages into buffers nobody reads any more) --
  // a load inside a conditional block makes hipcc wait for it at the block's end (phi copies), i.e. no prefetch at all.
  f32x4 ra[2][2];
  auto gload = [&](const Tile& tl, int kb, f32x4 (&r)[2]) {
    NSRW_CHECK(kb >= 0 && kb < KB && (kb < KB1 || tl.a2p));
    const float* ap = kb < KB1 ? tl.a1p + kb * 16 : tl.a2p + (kb - KB1) * 16;
#ifdef NSRW_EXP_NOA          // (NSRW_EXP_*: timing ablations only -- tools/ab_wide.sh; the results are wrong)
    asm volatile("" : "+v"(r[0]), "+v"(r[1]) : "v"(ap));
#elif defined(NSRW_EXP_NTA) || defined(NSRW_EXP_NT)
    r[0] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ap));
    r[1] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ap + 4));
#else
    r[0] = *reinterpret_cast<const f32x4*>(ap);
    r[1] = *reinterpret_cast<const f32x4*>(ap + 4);
#endif
  };
  // weights of stage kb -> LDS buffer `buf`: 3 NCB chunks of 1 KiB, col-block cbl = wave, wave + NW, ... by wave `wave`
  // (fewer col-blocks than waves: the surplus waves re-fetch col-blocks 0, 1, ... -- the same bytes to the same place -- so
  // that every wave issues the same number of VMEM operations per stage and one counted wait serves all)
  auto dma = [&](const Tile& tl, int kb, int buf) {
#pragma unroll
    for (int q = 0; q < (NCB + NW - 1) / NW; ++q) {
      const int cbl = (wave + NW * q) % NCB;
      char* l = smem + buf * kStage + kABytes + cbl * kFrag;
      const int soff = __builtin_amdgcn_readfirstlane(tl.wsrc + (cbl * KB + kb) * kFrag);
      NSRW_CHECK(soff >= 0 && (unsigned)soff + (unsigned)kFrag <= g.wb_bytes);
#ifndef NSRW_EXP_NODMA
      NSRW_DMA(rsrc, l, lane, soff, 0); NSRW_DMA(rsrc, l, lane, soff, 1);
      if constexpr (NPC == 3) NSRW_DMA(rsrc, l, lane, soff, 2);
#endif
    }
  };
  float amax = 0.0f;                                               // f16x2: largest activation magnitude this lane has split
  [[maybe_unused]] float amax_nxt = 0.0f;                          // kBits: ... of the NEXT tile's rows (amax: of this tile's)
  auto astore = [&](int buf, const f32x4 (&r)[2], float& am) {
    u32x4 p[NPC];
#ifdef NSRW_EXP_NOSPLIT
    p[0] = __builtin_bit_cast(u32x4, r[0]); p[1] = __builtin_bit_cast(u32x4, r[1]);
    if constexpr (NPC == 3) p[2] = p[0];
#else
    if constexpr (NP == 3) split8_b3(r[0], r[1], p);
    else if constexpr (NP == 2) split8_h2(r[0], r[1], p, am);
    else { p[0] = __builtin_bit_cast(u32x4, r[0]); p[1] = __builtin_bit_cast(u32x4, r[1]); }
#endif
    char* l = smem + buf * kStage + wave * kFrag + lane * 16;
#pragma unroll
    for (int q = 0; q < NPC; ++q) *reinterpret_cast<u32x4*>(l + q * 1024) = p[q];
  };
  // One stage behind its fetches: the 12 NJ MFMAs on buffer `buf`, then the A pieces of the following stage (values `r`, landed
  // a stage ago) split and written to the other buffer.  The instruction order is given to the scheduler as a pattern
  // (sched_group_barrier): the B fragments of column block j + 1 are read behind the first MFMAs of block j, and the split's
  // 44 VALU instructions run four per MFMA in the shadow of the last block's twelve -- left alone, hipcc reads every fragment
  // just in time (an exposed LDS latency per column block) and runs the whole split behind the last MFMA with an idle pipe.
  auto stage = [&](int buf, f32x16 (&acc)[2][NJ], const f32x4 (&r)[2], float& am) {
    const char* pa = smem + buf * kStage + (wm * 2) * kFrag + lane * 16;
    const char* pb = smem + buf * kStage + kABytes + (wn * NJ) * kFrag + lane * 16;
    u32x4 fa[2][NPC], fb[2][NPC];
    constexpr int kMfmaPerBlock = NP == 3 ? 12 : NP == 2 ? 6 : 16;  // MFMAs of one column block: both row blocks x the kept products (fp32: x 8 k pairs)
#ifdef NSRW_EXP_NOFRAG
#define NSRW_FRAG(dst, src) asm volatile("" : "=v"(dst) : "v"(src))
#else
#define NSRW_FRAG(dst, src) dst = *reinterpret_cast<const u32x4*>(src)
#endif
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < NPC; ++q) NSRW_FRAG(fa[i][q], pa + (i * NPC + q) * 1024);
#pragma unroll
    for (int q = 0; q < NPC; ++q) NSRW_FRAG(fb[0][q], pb + q * 1024);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (j + 1 < NJ)
#pragma unroll
        for (int q = 0; q < NPC; ++q) NSRW_FRAG(fb[(j + 1) & 1][q], pb + ((j + 1) * NPC + q) * 1024);
      // smallest terms first; the two row-blocks alternate, so no MFMA waits for its predecessor's accumulator
      if constexpr (NP == 3) {
#define NSRW_PAIR(PA, PB)                                            \
  acc[0][j] = mfma_b3(fa[0][PA], fb[j & 1][PB], acc[0][j]);          \
  acc[1][j] = mfma_b3(fa[1][PA], fb[j & 1][PB], acc[1][j]);
        NSRW_PAIR(2, 0) NSRW_PAIR(1, 1) NSRW_PAIR(0, 2) NSRW_PAIR(1, 0) NSRW_PAIR(0, 1) NSRW_PAIR(0, 0)
#undef NSRW_PAIR
      } else if constexpr (NP == 2) {
#define NSRW_PAIR(PA, PB)                                            \
  acc[0][j] = mfma_h2w(fa[0][PA], fb[j & 1][PB], acc[0][j]);         \
  acc[1][j] = mfma_h2w(fa[1][PA], fb[j & 1][PB], acc[1][j]);
        NSRW_PAIR(1, 0) NSRW_PAIR(0, 1) NSRW_PAIR(0, 0)
#undef NSRW_PAIR
      } else {
        // (the chunks are cast as VECTORS first: __builtin_bit_cast(float, uvec[e]) of a single element makes hipcc 7.2 take element 0
        // for every e -- found on this kernel's first run, reproduced in ten lines; profiles/r06/README.md)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const f32x4 xb = __builtin_bit_cast(f32x4, fb[j & 1][c]);
          const f32x4 x0 = __builtin_bit_cast(f32x4, fa[0][c]), x1 = __builtin_bit_cast(f32x4, fa[1][c]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[e], xb[e], acc[0][j], 0, 0, 0);
            acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[e], xb[e], acc[1][j], 0, 0, 0);
          }
        }
      }
    }
#undef NSRW_FRAG
    astore(buf ^ 1, r, am);
#ifndef NSRW_EXP_NOFRAG
    NSRW_SGB(NSRW_MASK_DSRD, 3 * NPC);
#pragma unroll
    for (int j = 0; j + 1 < NJ; ++j) {
#pragma unroll
      for (int q = 0; q < NPC; ++q) { NSRW_SGB(NSRW_MASK_MFMA, 1); NSRW_SGB(NSRW_MASK_DSRD, 1); }
      NSRW_SGB(NSRW_MASK_MFMA, kMfmaPerBlock - NPC);
    }
#else
    NSRW_SGB(NSRW_MASK_MFMA, kMfmaPerBlock * (NJ - 1));
#endif
#pragma unroll
    for (int q = 0; q < kMfmaPerBlock; ++q) { NSRW_SGB(NSRW_MASK_MFMA, 1); NSRW_SGB(NSRW_MASK_VALU, 4); }
    NSRW_SGB(NSRW_MASK_DSWR, NPC);
  };
  // end of a stage: this wave's LDS reads are done, its share of the next stage's weights has landed (everything but the two
  // younger A loads issued behind the DMA), its A pieces are written; the barrier makes that true for the workgroup
  auto stage_end = [&]() {
#ifdef NSRW_EXP_NOA
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
#endif
#ifndef NSRW_EXP_NOBAR
    __builtin_amdgcn_s_barrier();
#endif
  };

  Tile cur, nxt;
  long long t = blockIdx.x;
  while (t < total && !coords(t, cur)) t += gridDim.x;
  if (t >= total) return;
#ifdef NSRW_EXP_STAGGER      // timing experiment: workgroups start j / 8 of a tile's time apart, so that their epilogues' store bursts do not coincide
  {
    const int j = (blockIdx.x >> 3) & 7;
    const int units = j * KB * (NJ * (NP == 3 ? 12 : 6) * 2 * 32 / 8 / 64);          // sleep units of 64 cycles
    for (int u = 0; u < units; u += 64) __builtin_amdgcn_s_sleep(64);
  }
#endif
  gload(cur, 0, ra[0]);
  dma(cur, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
  gload(cur, 1, ra[1]);
  __builtin_amdgcn_sched_barrier(0);
  astore(0, ra[0], amax);
  stage_end();
  while (true) {
    long long tn = t + gridDim.x;
    while (tn < total && !coords(tn, nxt)) tn += gridDim.x;
    const bool more = tn < total;
    if (!more) nxt = cur;                                          // (what the last stages fetch then is never read)
    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    for (int kb = 0; kb < KB; kb += 2) {                           // (KB is even: both K extents are multiples of 32)
      const bool last = kb + 2 >= KB;
      Tile nx;                                                     // the tile of stages kb + 2, kb + 3
      nx.a1p = last ? nxt.a1p : cur.a1p; nx.a2p = last ? nxt.a2p : cur.a2p; nx.wsrc = last ? nxt.wsrc : cur.wsrc;
      const int k2 = last ? 0 : kb + 2;
      // even stage: MFMAs on buffer 0; weights of stage kb + 1 -> buffer 1; A of stage kb + 2 -> ra[0]; A pieces of kb + 1 -> buffer 1
      dma(cur, kb + 1, 1);
      __builtin_amdgcn_sched_barrier(0);                           // the A loads are the stage's YOUNGEST two VMEM operations:
      gload(nx, k2, ra[0]);                                        // stage_end's vmcnt(2) leaves exactly them in flight
      __builtin_amdgcn_sched_barrier(0);                           // ... and the fetches stay at the head of the stage
      stage(0, acc, ra[1], amax);
      stage_end();
      // odd stage: MFMAs on buffer 1; weights of stage kb + 2 -> buffer 0; A of kb + 3 -> ra[1]; A pieces of kb + 2 -> buffer 0
      dma(nx, k2, 0);
      __builtin_amdgcn_sched_barrier(0);
      gload(nx, k2 + 1, ra[1]);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kBits) {                                       // this astore splits stage k2 of nx: the next tile's rows when `last`
        float am = last ? amax_nxt : amax;
        stage(1, acc, ra[0], am);
        amax_nxt = last ? am : amax_nxt;
        amax = last ? amax : am;
      } else {
        stage(1, acc, ra[0], amax);
      }
      stage_end();
    }

    // epilogue: lane owns column n, rows 8 (r / 4) + 4 (lane / 32) + r % 4 of each 32 x 32 block.  A tile that lies inside
    // the matrix -- all of them but the last M-block's and a ragged N edge -- takes the predicate-free form: 16 stores per
    // block back to back.  (Per-row predicates put every store into a conditional block of its own, and hipcc then waits
    // vmcnt(0) in front of each: the stores of a tile serialise on the memory round trip.)
    if constexpr (kBits) {
      // the rows of THIS tile that left fp16's range -> their word (N-tiles of one M-block set the same bits again: harmless)
      const unsigned long long out = __builtin_amdgcn_ballot_w64(!(amax < 65504.0f) && cur.m0 + 32 * wave + lrow < g.M);
      const unsigned w = (unsigned)out | (unsigned)(out >> 32);
      if (w != 0u && lane == 0) {
        const long long wi = (cur.m0 >> 5) + wave;
        NSRW_CHECK(wi >= 0 && wi < g.n_words);
        atomicOr(&g.row_words[wi], w);
      }
      amax = amax_nxt;
      amax_nxt = 0.0f;
    }
    const bool inside = !kList && cur.m0 + kTM <= g.M && cur.n0 + TN <= g.N;
    if (inside) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = cur.n0 + wn * (NJ * 32) + j * 32 + lrow;
        float b = 0.0f;
        if (g.bias) b = g.bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const long long mt = cur.m0 + wm * 64 + i * 32 + 4 * lh;
          float* cb = g.C + mt * g.ldc + n;
          NSRW_CHECK(mt + 27 < g.M && n < g.ldc && n < g.N);
          float aux[16];
          if constexpr (EPI == kMaskEpi) {
            const float* sb = g.mask + mt * g.ldm + n;
#pragma unroll
            for (int r = 0; r < 16; ++r) aux[r] = sb[(8 * (r >> 2) + (r & 3)) * g.ldm];
          }
          if constexpr (EPI == kAccum) {
#pragma unroll
            for (int r = 0; r < 16; ++r) aux[r] = cb[(8 * (r >> 2) + (r & 3)) * g.ldc];
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = (NP == 2 ? acc[i][j][r] * g.cscale : acc[i][j][r]) + b;
            if constexpr (EPI == kRelu) v = (v < 0.0f) ? 0.0f : v;               // NaN stays NaN, as through torch's relu
            if constexpr (EPI == kMaskEpi) v = (aux[r] > 0.0f) ? v : 0.0f;
            if constexpr (EPI == kAccum) v = aux[r] + v;
#ifdef NSRW_EXP_NOSTORE
            if (v == 123.456f)
#endif
#if defined(NSRW_EXP_NTC) || defined(NSRW_EXP_NT)
            __builtin_nontemporal_store(v, &cb[(8 * (r >> 2) + (r & 3)) * g.ldc]);
#else
            cb[(8 * (r >> 2) + (r & 3)) * g.ldc] = v;
#endif
          }
        }
      }
    } else {
      const bool full_rows = cur.m0 + kTM <= g.M;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int n = cur.n0 + wn * (NJ * 32) + j * 32 + lrow;
        const bool ncol = n < g.N;
        const float b = (g.bias && ncol) ? g.bias[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const long long mt = cur.m0 + wm * 64 + i * 32 + 4 * lh;
          float* cb = g.C + mt * g.ldc + n;
          const int rows_left = (int)(g.M - mt < 32 ? g.M - mt : 32);
          [[maybe_unused]] unsigned rowbits = 0u;                  // kList: the bits of this lane's 28 rows from mt on
          if constexpr (kList) {
            const long long wi = (cur.m0 >> 5) + wm * 2 + i;
            NSRW_CHECK(wi >= 0);
            rowbits = wi < g.n_words ? g.row_words[wi] >> (4 * lh) : 0u;    // (no word behind row M: no bit)
          }
          auto rowok = [&](int ro) { return !kList || ((rowbits >> ro) & 1u) != 0u; };
          float aux[16];
          if constexpr (EPI == kMaskEpi) {
            const float* sb = g.mask + mt * g.ldm + n;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int ro = 8 * (r >> 2) + (r & 3);
              aux[r] = (ncol && (full_rows || ro < rows_left) && rowok(ro)) ? sb[ro * g.ldm] : 0.0f;
            }
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ro = 8 * (r >> 2) + (r & 3);
            float v = (NP == 2 ? acc[i][j][r] * g.cscale : acc[i][j][r]) + b;
            if constexpr (EPI == kRelu) v = (v < 0.0f) ? 0.0f : v;
            if constexpr (EPI == kMaskEpi) v = (aux[r] > 0.0f) ? v : 0.0f;
            if (ncol && (full_rows || ro < rows_left) && rowok(ro)) {
              NSRW_CHECK(mt + ro < g.M && n < g.ldc);
              if constexpr (EPI == kAccum) v = cb[ro * g.ldc] + v;
              cb[ro * g.ldc] = v;
            }
          }
        }
      }
    }
    if (!more) break;
    t = tn;
    cur = nxt;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // no LDS-DMA may outlive the workgroup
  if constexpr (NP == 2 && !kBits) {
    // (NaN compares false on both sides and passes through the pieces as NaN, as through an fp32 GEMM; inf is out of range)
    if (__builtin_amdgcn_ballot_w64(!(amax < 65504.0f)) != 0ull && lane == 0) atomicOr(g.range_flag, 1u);
  }
}

template <int NJ, int EPI, int WM>
__global__ void __launch_bounds__(128 * WM, (wgs_per_cu<NJ, WM>())) kw_gemm_b3(const GemmArgs g) {
  __shared__ __attribute__((aligned(1024))) char smem[split_lds_bytes<NJ, WM, 3>()];
  gemm_split_body<NJ, EPI, WM, 3>(g, smem);
}

template <int NJ, int EPI, int WM>
__global__ void __launch_bounds__(128 * WM, (wgs_per_cu<NJ, WM>())) kw_gemm_f32(const GemmArgs g) {
  __shared__ __attribute__((aligned(1024))) char smem[split_lds_bytes<NJ, WM, 1>()];
  gemm_split_body<NJ, EPI, WM, 1>(g, smem);
}

template <int NJ, int EPI, int WM>
__global__ void __launch_bounds__(128 * WM, (wgs_per_cu<NJ, WM>())) kw_gemm_h2(const GemmArgs g) {
  __shared__ __attribute__((aligned(1024))) char smem[split_lds_bytes<NJ, WM, 2>()];
  gemm_split_body<NJ, EPI, WM, 2>(g, smem);
}

// the row-granular twins (GemmArgs::row_words / row_list): f16x2 sets a bit per row that leaves the range, bf16x3 walks the listed
// M-blocks and stores the flagged rows alone
template <int NJ, int EPI, int WM>
__global__ void __launch_bounds__(128 * WM, (wgs_per_cu<NJ, WM>())) kw_gemm_b3_rows(const GemmArgs g) {
  __shared__ __attribute__((aligned(1024))) char smem[split_lds_bytes<NJ, WM, 3>()];
  gemm_split_body<NJ, EPI, WM, 3, true>(g, smem);
}

template <int NJ, int EPI, int WM>
__global__ void __launch_bounds__(128 * WM, (wgs_per_cu<NJ, WM>())) kw_gemm_h2_rows(const GemmArgs g) {
  __shared__ __attribute__((aligned(1024))) char smem[split_lds_bytes<NJ, WM, 2>()];
  gemm_split_body<NJ, EPI, WM, 2, true>(g, smem);
}
