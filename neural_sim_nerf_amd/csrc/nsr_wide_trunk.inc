// nsr_wide_trunk.inc -- the ON-CHIP kernels of the layered renderer's f16x2 arithmetic: persistent launches that run a whole chain of
// layers on a block of points, with the value between two layers in LDS instead of HBM.  Included inside namespace nsrw
// (nsr_wide.hip), after nsr_wide_gemm.inc, whose arithmetic they restate per output element and must reproduce BIT FOR BIT
// (tests/test_gpu_wide_trunk.py, test_gpu_wide_heads.py, test_gpu_wide_trunk_bwd.py).  TWO f16x2 bodies made of ONE set of building
// blocks, each a prologue, the block loop, the row loop -- the next row's fields, the stages with trunk_dma one stage ahead, the
// epilogue, the barrier -- stated once: trunk_h2_body (forward), behind the kernels kw_trunk_h2<NJ, HEADS, WR>, kw_keep_h2<NJ, HEADS>
// and their kw_enc_ twins, and trunk_bwd_body (input-gradient backward), behind kw_trunk_bwd_h2<NJ> and kw_keep_bwd_h2<NJ>; what a
// kernel of a body has of its own stands behind an `if constexpr` of the body.  (At the end of the file: kw_rerun_b3<NJ, WR>, the
// forward trunk once more on the bf16x3 arithmetic, for the conditional re-run of a pass that left fp16's range: three pieces, no
// cscale, no amax -- a body of its own on the same blocks; the blocks that count pieces take NP = 2 or 3.)
//
// The building blocks (above the kernels, each stated once):
//   * the row table.  A launch walks a table of TrunkLayer rows (Net::dTrunk): per row the weight image, K as k16 blocks of the
//     encoding image and of the activation image, cscale, and two packed words, `form` and `store`, whose bit layout stands at the
//     struct with the functions that pack them and the accessors that read them.
//   * the shape (trunk_lds, TrunkCtx, trunk_rows / trunk_ncb / trunk_sh / trunk_wstage).  512 threads = 8 waves = two per SIMD, as WR (rows)
//     x 8 / WR (columns): wave w owns rows 32 (w % WR) .. + 31 of the block and NJ column blocks (NJ accumulators of 32 x 32).  The
//     accumulator has the column on the lane and the rows in registers (trunk_acc_row: register r = row 8 (r / 4) + 4 (lane / 32) +
//     r % 4 of the wave's 32), the A fragment the row on the lane and k in the register.  LDS: the weight double buffer, then the row-major piece
//     images [piece][row][k], whose row stride (2 K + 16 bytes: an odd number of 16-byte slots) spreads the 16 rows of a ds_read_b128
//     lane group over all 64 banks.
//   * trunk_dma: a stage of weights -- two k16 blocks of every column block (4 KiB a column block) -- into one half of the double
//     buffer, by the LDS-DMA and from the very image (Mat::img[kH2]) gemm_split_body's stages move.  Fetched one stage ahead ACROSS row
//     and block boundaries.
//   * trunk_stage: the arithmetic.  The accumulator of an output element starts at 0 and takes the k16 blocks of K in ascending
//     order, per block the piece products (1,0) (0,1) (0,0) on v_mfma_f32_32x32x16_f16, A operand = activation, B operand = weight:
//     the operands are the very fragments gemm_split_body feeds.  One stage = 6 NA MFMAs of a wave, closed by
//   * trunk_sync: the full wait and the barrier -- this wave's LDS-DMA and loads have landed, its LDS reads and writes are done, and
//     that for the workgroup.  Because every stage ends in it, the last read of a row's input is behind every wave before the first
//     epilogue write, so a row's output may overwrite its input IN PLACE;
//   * trunk_write_inplace: ... which is what the epilogue does with a value the next row reads: split by split8_h2's formulas (RNE
//     fp16, exact residual -> fp16) into the next row's A pieces and fed to amax, so the range flag rises exactly when the per-layer
//     chain's next launch would raise it (the split8_h2 call stands in the kernel's epilogue, next to the arithmetic that feeds it);
//     the transposition of accumulator rows into image rows is trunk_write_inplace's 16-bit LDS writes.  trunk_lds_barrier then puts
//     the writes in front of the next row's reads.
//   * trunk_rows_fetch / trunk_rows_store: a block's rows of an [M, ld] fp32 matrix -> a piece image (the encodings, the direction
//     encodings, the incoming gradient), rows behind M clamped on the way in, split and fed to amax as above.
//   * trunk_rows_encode (NSRW_FLAG_EMBED_ONCHIP; the kw_enc_ twins of the forward and kept kernels): the same registers as
//     trunk_rows_fetch, computed from the block's points by kw_embed's own functions instead of fetched -- kw_embed's bits, and
//     trunk_rows_store behind it as it was.
//   * NSRW_ROWS_OUT: the fp32 epilogue store of a lane's 16 accumulator rows to an [M, ld] matrix (C, the kept H[D - 1] and HV),
//     without a look at the row inside M, guarded in the last block.
//   * trunk_tail: no LDS-DMA outlives the workgroup; the range flag.
//
// kw_trunk_h2<NJ, HEADS, WR>: all D pts_linears layers (RH:99-107) of a network of packed width Wp <= 128 on a block of 128 points
// (WR = 2, below: Wp <= 256, 64 points), K = [encoding | h].  Epilogue acc * cscale + bias, relu with NaN kept.  HEADS = false: only
// the last layer's fp32 output goes to HBM (rows of Wp floats: what the heads read).
//
// HEADS = true (NSRW_FLAG_HEADS_ONCHIP): the last layer is split into LDS like every other and the SAME workgroup runs the heads
// (RH:109-122) on its 128 rows as further rows of the layer table -- alpha_linear (before h is overwritten), feature_linear (plain
// epilogue, in place), views_linears.0 on K = [feature | direction encoding] (the direction encodings of the block are split into
// the encoding image, which the trunk no longer reads), rgb_linear; or output_linear alone -- and stores nothing but the raw
// outputs, 16 bytes a point with view directions.  A row says its K order, how many column blocks its image has (what the LDS-DMA
// moves) and how many are computed (a wave whose column blocks hold zero weights only issues no MFMA), its epilogue and where
// its output goes; the two column halves of the workgroup take the column blocks in turn, so that a head of two column blocks
// occupies all eight waves.  Every value the per-layer chain would split as an A operand is split here and fed to amax: h, the feature,
// the direction encoding, the views layer's output.
//
// LDS (static, one workgroup per CU): weights 2 x 8 NJ KiB, activation 2 pieces x 128 x (128 NJ + 16) B, encoding 2 pieces x
// 128 x 208 B (Ci <= 96; heads form: Cv <= 96 too) -- 155 648 B at NJ = 2, 106 496 B at NJ = 1, in either form.
//
// WR = 2 (NSRW_FLAG_TRUNK_WIDE): the WIDE form, for 128 < Wp <= 256, trunk-only.  The same kernel on a block of 64 points: the eight
// waves are 2 (rows) x 4 (column quarters), wave w owns rows 32 (w % 2) .. + 31 and the two column blocks of quarter w / 2, so a wave
// still reads four A and eight B fragments per twelve MFMAs.  A stage is two k16 blocks of EIGHT column blocks (32 KiB; every wave
// moves both k16 blocks of column block w), the activation image has rows of 528 B (33 slots of 16 bytes: odd, as above).  The weight
// image of a padded width of 160 or 192 has six column blocks: the two behind them are not moved, and the waves of the last quarter
// issue no MFMA (their output would be dropped anyway: a column block behind Wp holds zero weights).  LDS: weights 2 x 32 KiB,
// activation 2 x 64 x 528 B, encoding 2 x 64 x 208 B = 159 744 B.  Per output element nothing differs from WR = 4, hence the same bits.
//
// kw_trunk_bwd_h2<NJ> (NSRW_FLAG_TRUNK_BWD; behind the forward, where its own rows and epilogue are described): the
// input-gradient chain of net_backward_chain in the shape of the heads form, the gradient in the activation image, no encoding image.
//
// kw_keep_h2<NJ, HEADS>, kw_keep_bwd_h2<NJ>, kw_mask_pack, kw_mask_unpack (NSRW_FLAG_TRUNK_KEEP; the bit layout of the masks stands
// in front of the forward body): the forward that KEEPS what a backward reads, as one launch -- the forward body with KEEP -- and the
// backward that reads it -- the backward body with BITS.
#undef NSRW_FILE_TAG
#define NSRW_FILE_TAG 200000        /* a failed NSRW_CHECK of this file reports 200000 + its line (nsrw_debug_bounds_status) */

enum { kTrunkToLds = 0, kTrunkToC = 1, kTrunkToRaw = 2, kTrunkToGep = 3 };      // where a row's output goes (trunk_form_dest)

struct TrunkLayer {                 // one row of a launch: a pts_linears layer, a head behind them, or a backward product (Net::dTrunk)
  unsigned img_off;                 // byte offset of the row's f16x2 weight image in Net::dImg[kH2]
  unsigned bias_off;                // its bias in Net::dBias (floats)
  int kbe, kbh;                     // k16 blocks of K taken from the encoding image / from the activation image
  float cscale;                     // Mat::cscale
  // the rest of a row in two packed words, so that a row stays eight scalar registers (the trunk-only forward form has most of it
  // fixed: encoding first, relu, the last layer to C).  THE bit layout; packed by trunk_form / trunk_bwd_form / trunk_store and read
  // through the accessors below, by nothing else:
  //   form   bits 0-3    col-blocks of the weight image (Mat::ncb): what the LDS-DMA moves                       trunk_form_ncb
  //          bits 4-7    col-blocks of output that are computed (the rest of the image holds zero weights)       trunk_form_ncbo
  //          bit 8       the matrix's K order: 0 = [encoding | hidden] (pts_linears), 1 = [hidden | encoding]    trunk_form_h_first
  //          bit 9       epilogue: relu behind acc * cscale + bias                                                trunk_form_relu
  //          bits 10-11  kTrunkToLds: split in place into the activation image; kTrunkToC: TrunkArgs::C;        trunk_form_dest
  //                      kTrunkToRaw: TrunkArgs::RAW; kTrunkToGep (backward): summed into TrunkBwdArgs::GEP
  //          bit 12      backward, kTrunkToGep: the row adds to the sum (the first such row sets it)              trunk_form_accum
  //   store  forward, kTrunkToRaw: columns 0 .. (bits 0-7) - 1 go to RAW[row * (bits 16-23) + (bits 8-15) + column]
  //                                                                           trunk_store_ncols, trunk_store_ld, trunk_store_col0
  //          backward: the whole word is the index of the layer whose kept activation is the row's relu mask
  int form, store;
  int pad_;
};
inline int trunk_form(int ncb, int ncbo, bool h_first, bool relu, int dest) { return ncb | ncbo << 4 | (int)h_first << 8 | (int)relu << 9 | dest << 10; }
inline int trunk_bwd_form(int ncbo, int dest, bool accum) { return trunk_form(ncbo, ncbo, false, false, dest) | (int)accum << 12; }
inline int trunk_store(int ncols, int col0, int ld) { return ncols | col0 << 8 | ld << 16; }
__host__ __device__ inline int trunk_form_ncb(int form) { return form & 15; }
__host__ __device__ inline int trunk_form_ncbo(int form) { return form >> 4 & 15; }
__host__ __device__ inline bool trunk_form_h_first(int form) { return form >> 8 & 1; }
__host__ __device__ inline bool trunk_form_relu(int form) { return form >> 9 & 1; }
__host__ __device__ inline int trunk_form_dest(int form) { return form >> 10 & 3; }
__host__ __device__ inline bool trunk_form_accum(int form) { return form >> 12 & 1; }
__host__ __device__ inline int trunk_store_ncols(int store) { return store & 255; }
__host__ __device__ inline int trunk_store_col0(int store) { return store >> 8 & 255; }
__host__ __device__ inline int trunk_store_ld(int store) { return store >> 16 & 255; }

// Where the points of a launch that computes its encodings itself come from (the ENC forms; what EmbedArgs carries of them): rays
// form -- point p lies on ray p / S at depth z[p] -- or, rays_o == nullptr, the points form of nsrw_run_network
struct TrunkPoints {
  const float* rays_o; const float* rays_d; const float* z; const float* vd;      // [R,3], [R,3], [M], [R,3]
  const float* pts; const float* dirs;                                            // [M,3] each
  int S;
  int L, Lv;                        // bands of the position / direction encoding
};

struct TrunkArgs {
  const float* E; int ldE;          // encodings [M, ldE], ldE = Ci <= kTrunkCiMax; nullptr in the ENC forms: encoded here, from `pts`
  const char* img; unsigned img_bytes;
  const float* bias; unsigned bias_floats;
  const TrunkLayer* layers; int D;  // rows of the table: the pts_linears (trunk-only form), and the heads behind them (heads form)
  float* C; int Wp;                 // trunk-only form: the last layer's output [M, Wp]
  int Dt;                           // heads form: the pts_linears among the D rows; the direction encodings [M, ldED], ldED = Cv <=
  const float* ED; int ldED;        // kTrunkCiMax (nullptr: a network without view directions); the raw outputs the kTrunkToRaw
  float* RAW;                       // rows store to
  long long M;
  unsigned* range_flag;
  TrunkPoints pts;                  // the ENC forms (behind everything else: the other forms read their arguments where they were)
};

// WR wave rows of 32 points by 8 / WR wave columns of NJ column blocks: WR = 4 the 128-row forms, WR = 2 the wide form
constexpr int kTrunkCiMax = 96;
constexpr int kTrunkSE = 2 * kTrunkCiMax + 16;                                  // row stride of an encoding piece image (bytes)
template <int WR = 4> constexpr int trunk_rows() { return 32 * WR; }             // points of a block
template <int NJ, int WR = 4> constexpr int trunk_ncb() { return 8 / WR * NJ; }  // col-blocks of a block's output
template <int NJ, int WR = 4> constexpr int trunk_sh() { return 64 * trunk_ncb<NJ, WR>() + 16; }          // ... of an activation piece image
// NP: pieces per operand -- 2: f16x2, 3: bf16x3 (kw_rerun_b3); a fragment is NP KiB, a piece image row has the same bytes in either
template <int NJ, int WR = 4, int NP = 2> constexpr int trunk_wstage() { return trunk_ncb<NJ, WR>() * 2 * NP * 1024; }     // one stage of weights: every col-block x 2 k16 blocks
template <int NJ, int WR = 4, int NP = 2> constexpr int trunk_lds_bytes() {
  return 2 * trunk_wstage<NJ, WR, NP>() + NP * trunk_rows<WR>() * trunk_sh<NJ, WR>() + NP * trunk_rows<WR>() * kTrunkSE;
}

typedef unsigned short __attribute__((may_alias)) u16a;
typedef u32x4 __attribute__((may_alias)) u32x4a;

// ---- the building blocks ------------------------------------------------------------------------------------------------------------

// The workgroup's LDS, LDS bytes of it: a kernel's one static array, at namespace scope so that the building blocks name it as the
// kernel does (a pointer handed down to them is the same address and costs instructions: the compiler then no longer folds the
// array's base into the offsets).  Kernels of one size name the same variable; each gets its own allocation.
template <int LDS> __shared__ __attribute__((aligned(1024))) char trunk_lds[LDS];

template <int LDS>
struct TrunkCtx {                   // the workgroup's LDS (LDS bytes) and who this lane is in it
  __device__ __forceinline__ static char* smem() { return trunk_lds<LDS>; }
  int lane, wave;                   // wave: uniform
  int wr, wc;                       // the wave's row / column among the WR x 8 / WR waves
  int lrow, lh;                     // lane % 32: the row of an A fragment, the column of an accumulator; lane / 32: the k half / row group
  // this lane's A fragment of k16 block 0, piece 0 of the piece image at `base` with rows of `stride` bytes
  __device__ __forceinline__ int frag0(int base, int stride) const { return base + (32 * wr + lrow) * stride + lh * 16; }
};
template <int WR, int LDS>
__device__ __forceinline__ TrunkCtx<LDS> trunk_ctx() {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  return {lane, wave, wave & (WR - 1), wave >> (WR == 4 ? 2 : 1), lane & 31, lane >> 5};
}

// THE register to row map: accumulator register r of a lane holds row first + 8 (r / 4) + group + r % 4, first = the wave's first
// row (32 wr), group = 4 (lane / 32); without the two, the row relative to theirs
__device__ __forceinline__ constexpr int trunk_acc_row(int r, int first = 0, int group = 0) { return first + 8 * (r >> 2) + group + (r & 3); }

// weights of the stage (k16 blocks kb0, kb0 + 1 of a row with KB blocks) -> LDS buffer `buf`: 2 NCB chunks of 2 KiB, each [piece 2][64
// lanes][8 fp16] as the image holds it; wave w moves chunk w % (2 NCB) (NCB = 2: every chunk twice, the same bytes to the same place,
// so that one wait serves all waves; NCB = 8: 16 chunks, wave w moves w and w + 8, the two k16 blocks of col-block w).  VARIES: the
// image of a row may have fewer than NCB col-blocks (`ncb`); the chunks behind them are not moved, and no MFMA reads them.
// NP = 3: chunks of 3 KiB, [piece 3][64 lanes][8 bf16], three LDS-DMAs each.
template <int NCB, bool VARIES, int NP = 2, int LDS>
__device__ __forceinline__ void trunk_dma(const TrunkCtx<LDS>& c, const __amdgpu_buffer_rsrc_t rsrc, unsigned img_bytes, unsigned img_off, int KB,
                                          int kb0, int buf, int ncb) {
  constexpr int kFrag = NP * 1024, kWStage = NCB * 2 * kFrag;
#pragma unroll
  for (int i = 0; i < (2 * NCB + 7) / 8; ++i) {
    const int u = (c.wave + 8 * i) % (2 * NCB), cb = u % NCB, kbl = u / NCB;
    if constexpr (VARIES) {
      NSRW_CHECK(ncb >= 1 && ncb <= NCB);
      if (cb >= ncb) continue;
    }
    char* l = c.smem() + buf * kWStage + (cb * 2 + kbl) * kFrag;
    const int soff = __builtin_amdgcn_readfirstlane((int)img_off + (cb * KB + kb0 + kbl) * kFrag);
    NSRW_CHECK(kb0 >= 0 && kb0 + kbl < KB && soff >= 0 && (unsigned)soff + (unsigned)kFrag <= img_bytes && (buf == 0 || buf == 1) &&
               buf * kWStage + (cb * 2 + kbl) * kFrag + kFrag <= 2 * kWStage);
    NSRW_DMA(rsrc, l, c.lane, soff, 0); NSRW_DMA(rsrc, l, c.lane, soff, 1);
    if constexpr (NP == 3) NSRW_DMA(rsrc, l, c.lane, soff, 2);
  }
}

// this wave's LDS-DMA and global loads have landed and its LDS reads and writes are done; the barrier makes that true for the workgroup
__device__ __forceinline__ void trunk_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// the LDS-only barrier behind an in-place epilogue: the next row reads what every wave of its rows has written
__device__ __forceinline__ void trunk_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// the end of a kernel: no LDS-DMA may outlive the workgroup; the range flag rises when a lane has split a value outside fp16's range
// (kw_rerun_b3, which splits nothing that has a range, takes the first half alone)
__device__ __forceinline__ void trunk_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
template <int LDS>
__device__ __forceinline__ void trunk_tail(const TrunkCtx<LDS>& c, float amax, unsigned* range_flag) {
  trunk_drain();
  if (__builtin_amdgcn_ballot_w64(!(amax < 65504.0f)) != 0ull && c.lane == 0) atomicOr(range_flag, 1u);
}

// one stage of this wave's first NA accumulators (accumulator j = column block cb_of(j)): the A fragments at aoff (pieces pstride
// apart), the weights of the buffer at wbuf
// NP = 3 (bf16x3): three pieces a fragment and the six products (2,0) (1,1) (0,2) (1,0) (0,1) (0,0) on v_mfma_f32_32x32x16_bf16, gemm_split_body's
// order at NP = 3; one stage = 12 NA MFMAs of a wave.
template <int NA, int NP = 2, int NJ, class CbOf, int LDS>
__device__ __forceinline__ void trunk_stage(const TrunkCtx<LDS>& c, const CbOf& cb_of, f32x16 (&acc)[NJ], int wbuf, int aoff, int pstride) {
  constexpr int kFrag = NP * 1024;
  const char* pb = c.smem() + wbuf + c.lane * 16;
  u32x4 fa[2][NP], fb[2][NA][NP];
#pragma unroll
  for (int kbl = 0; kbl < 2; ++kbl) {
#pragma unroll
    for (int q = 0; q < NP; ++q) fa[kbl][q] = *reinterpret_cast<const u32x4a*>(c.smem() + aoff + q * pstride + kbl * 32);
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int q = 0; q < NP; ++q) fb[kbl][j][q] = *reinterpret_cast<const u32x4a*>(pb + (cb_of(j) * 2 + kbl) * kFrag + q * 1024);
  }
  // per accumulator the order of gemm_split_body: k16 blocks ascending, per block (1,0) (0,1) (0,0); the column blocks alternate
#pragma unroll
  for (int kbl = 0; kbl < 2; ++kbl) {
    if constexpr (NP == 3) {
#define NSRW_B3_ROUND(PA, PB) \
  _Pragma("unroll") for (int j = 0; j < NA; ++j) acc[j] = mfma_b3(fa[kbl][PA], fb[kbl][j][PB], acc[j]);
      NSRW_B3_ROUND(2, 0) NSRW_B3_ROUND(1, 1) NSRW_B3_ROUND(0, 2) NSRW_B3_ROUND(1, 0) NSRW_B3_ROUND(0, 1) NSRW_B3_ROUND(0, 0)
#undef NSRW_B3_ROUND
    } else {
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][1], fb[kbl][j][0], acc[j]);
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][1], acc[j]);
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][0], acc[j]);
    }
  }
  NSRW_SGB(NSRW_MASK_DSRD, 2 * NP + 2 * NP * NA);                        // every fragment read of the stage ahead of its MFMAs
  NSRW_SGB(NSRW_MASK_MFMA, (NP == 3 ? 12 : 6) * NA);
}

// The rows of the block at m0 of X [M, ld] (KBX k16 blocks) -> a piece image, in two steps (a kernel may put a row's stages between
// them): lane = (row, k half) loads the 8 consecutive k of its fragment, as gemm_split_body's gload does, for the k16 blocks of its
// wave's column (kb % WC, IT of them); rows behind M are clamped on the way in and never stored.  (Branch-free loads: a block behind
// KBX re-reads the last one and is not written.)
template <int IT, int WC, int LDS>
__device__ __forceinline__ void trunk_rows_fetch(const TrunkCtx<LDS>& c, const float* X, int ld, int KBX, long long m0, long long M, f32x4 (&e)[IT][2]) {
  long long am = m0 + 32 * c.wr + c.lrow;
  if (am >= M) am = M - 1;
  NSRW_CHECK(am >= 0 && am < M);
  const float* xp = X + am * ld + 8 * c.lh;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int kb = WC * i + c.wc, kc = kb < KBX ? kb : KBX - 1;
    NSRW_CHECK(kc >= 0 && kc * 16 + 8 * c.lh + 8 <= ld);
    e[i][0] = *reinterpret_cast<const f32x4*>(xp + kc * 16);
    e[i][1] = *reinterpret_cast<const f32x4*>(xp + kc * 16 + 4);
  }
}
// The same registers from the block's POINTS instead of a matrix (the ENC forms): what trunk_rows_fetch would have loaded from the E
// (DIRS = false) or ED (DIRS = true) that kw_embed writes, computed by kw_embed's own functions -- embed_point, embed_col -- so that
// the bits are its bits, the exact zeros of the padding columns behind 3 + 6 L included.  Rows behind M are clamped to point M - 1
// before anything is read, as there.  Each lane computes the eight consecutive columns of its own fragments: no scratch, no barrier,
// and trunk_rows_store behind it is what it was.  (A block behind KBX is not computed: it is not written either.)  The unrolled path
// has sincos_enc's polynomial alone; a wave in which a lane met an argument for the fp64 library routine (|a| >= 2^24, inf, NaN:
// hostile rays) computes its columns once more, one by one through sincos_enc itself -- embed_col_hard, a CALL, so that the library
// routine's registers are its own and not the kernel's.  The scheduling barrier after every fourth column keeps four polynomial
// chains in flight, not twenty-four: the registers of the latter would not fit beside the kernel's.
__device__ __noinline__ float embed_col_hard(float x0, float x1, float x2, int i, int L) {
  const float x[3] = {x0, x1, x2};
  return embed_col(x, i, L, [](float a, float& sn, float& cs) { sincos_enc(a, sn, cs); });
}
template <int IT, int WC, bool DIRS, int LDS>
__device__ __forceinline__ void trunk_rows_encode(const TrunkCtx<LDS>& c, const TrunkPoints& s, int KBX, long long m0, long long M, f32x4 (&e)[IT][2]) {
  long long am = m0 + 32 * c.wr + c.lrow;
  if (am >= M) am = M - 1;
  NSRW_CHECK(am >= 0 && am < M && KBX >= 1 && (s.rays_o ? s.S >= 1 : true));
  float x[3];
  if (s.rays_o) {
    // ray am / S without a 64-bit division per lane: the block's first ray once (uniform), then a 32-bit one of the offset
    const long long r0 = m0 / s.S;
    const long long r = r0 + (int)(am - r0 * s.S) / s.S;
    NSRW_CHECK(am - r0 * s.S >= 0 && am - r0 * s.S < 0x7fffffffll && r * s.S <= am && am < (r + 1) * s.S);
    if constexpr (DIRS) {
#pragma unroll
      for (int q = 0; q < 3; ++q) x[q] = s.vd[r * 3 + q];
    } else {
      const float zz = s.z[am];
#pragma unroll
      for (int q = 0; q < 3; ++q) x[q] = embed_point(s.rays_o[r * 3 + q], s.rays_d[r * 3 + q], zz);
    }
  } else {
    const float* src = DIRS ? s.dirs : s.pts;
#pragma unroll
    for (int q = 0; q < 3; ++q) x[q] = src[am * 3 + q];
  }
  const int L = DIRS ? s.Lv : s.L;
  bool hard = false;
  auto poly = [&](float a, float& sn, float& cs) {
    if (sincos_enc_is_fast(a)) sincos_enc_fast(a, sn, cs);
    else { hard = true; sn = cs = 0.0f; }
  };
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int kb = WC * i + c.wc;
    if (kb < KBX) {
      // (opaque: which band and coordinate a column is does not change from block to block, and the compiler would otherwise keep
      // all of it -- a hundred registers -- across the row loop)
      int k0 = kb * 16 + 8 * c.lh;
      asm volatile("" : "+v"(k0));
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        e[i][t >> 2][t & 3] = embed_col(x, k0 + t, L, poly);
        if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      e[i][0] = e[i][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
  }
  if (__builtin_amdgcn_ballot_w64(hard) != 0ull) {
#pragma nounroll
    for (int u = 0; u < 8 * IT; ++u) {
      const int kb = WC * (u >> 3) + c.wc;
      if (kb >= KBX) continue;
      const float v = embed_col_hard(x[0], x[1], x[2], kb * 16 + 8 * c.lh + (u & 7), L);
#pragma unroll
      for (int w = 0; w < 8 * IT; ++w)
        if (w == u) e[w >> 3][(w >> 2) & 1][w & 3] = v;
    }
  }
}
// ... split by split8_h2 and written to the image whose fragment of this lane is at frag (TrunkCtx::frag0), pieces pstride apart,
// rows of `stride` bytes, inside the first lds_end bytes of LDS
// (NP = 3: by split8_b3, which has no range and leaves amax alone)
template <int IT, int WC, int NP = 2, int LDS>
__device__ __forceinline__ void trunk_rows_store(const TrunkCtx<LDS>& c, int KBX, const f32x4 (&e)[IT][2], int frag, int pstride, int stride, int lds_end,
                                                 float& amax) {
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int kb = WC * i + c.wc;
    if (kb < KBX) {
      u32x4 p[NP];
      if constexpr (NP == 3) split8_b3(e[i][0], e[i][1], p);
      else split8_h2(e[i][0], e[i][1], p, amax);
      NSRW_CHECK(kb * 32 + c.lh * 16 + 16 <= stride - 16 && frag + (NP - 1) * pstride + kb * 32 + 16 <= lds_end);
      *reinterpret_cast<u32x4a*>(c.smem() + frag + kb * 32) = p[0];
      *reinterpret_cast<u32x4a*>(c.smem() + frag + pstride + kb * 32) = p[1];
      if constexpr (NP == 3) *reinterpret_cast<u32x4a*>(c.smem() + frag + 2 * pstride + kb * 32) = p[2];
    }
  }
}

// The in-place epilogue write of half an accumulator column: p = split8_h2 of the lane's registers 8 hf .. 8 hf + 7 of column n, packed
// pairs (r, r + 1) -> the activation image of the <NJ, WR> layout, each half of a pair to its row as one 16-bit write (the
// transposition), inside the first lds_end bytes of LDS.  (The split8_h2 call itself stays with the kernel's epilogue arithmetic.)
// NP (the pieces of p: split8_b3's three) is read off the argument.
template <int NJ, int WR, int NP, int LDS>
__device__ __forceinline__ void trunk_write_inplace(const TrunkCtx<LDS>& c, const u32x4 (&p)[NP], int hf, int n, int lds_end) {
  constexpr int kRows = trunk_rows<WR>(), kSH = trunk_sh<NJ, WR>(), kHPiece = kRows * kSH, kHOff = 2 * trunk_wstage<NJ, WR, NP>();
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int row = trunk_acc_row(8 * hf + 2 * jj, 32 * c.wr, 4 * c.lh);
    const int off = kHOff + row * kSH + n * 2;
    NSRW_CHECK(row + 1 < kRows && n * 2 + 2 <= kSH - 16 && off + kSH + (NP - 1) * kHPiece + 2 <= lds_end);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      *reinterpret_cast<u16a*>(c.smem() + off + q * kHPiece) = (unsigned short)(p[q][jj] & 0xffffu);
      *reinterpret_cast<u16a*>(c.smem() + off + q * kHPiece + kSH) = (unsigned short)(p[q][jj] >> 16);
    }
  }
}

// The fp32 epilogue store of an accumulator column: v = the lane's 16 registers of column n -> rows m0 + trunk_acc_row(r, 32 wr,
// 4 (lane / 32)) of X [M, ld]; a block inside M (`inside`) stores without a look at the row, the last block row by row.
// A MACRO on purpose.  As a __forceinline__ function (tried: arguments by value and by reference, both paths in one function and
// one function per path) the kernels that use it no longer compile to the code they had (tools/kernel_asm_diff.py): with both
// paths in one function the two share their last store, otherwise the kept and the re-run kernels get another accumulator
// offset and other branches, and the forms of two column blocks another instruction order.
#define NSRW_ROWS_OUT(c, v, X, ld, n, m0, M, inside)                                                          \
  do {                                                                                                        \
    const long long mt = (m0) + 32 * (c).wr + 4 * (c).lh;                                                     \
    NSRW_CHECK((n) < (ld) && (!(inside) || mt + 27 < (M)));                                                   \
    float* xp = (X) + mt * (ld) + (n);                                                                        \
    if (inside) {                                                                                             \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) xp[trunk_acc_row(r) * (ld)] = (v)[r >> 2][r & 3];        \
    } else {                                                                                                  \
      _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                          \
        if (mt + trunk_acc_row(r) < (M)) xp[trunk_acc_row(r) * (ld)] = (v)[r >> 2][r & 3];                    \
    }                                                                                                         \
  } while (0)

// ---- the relu masks of a KEPT pass as bits (NSRW_FLAG_TRUNK_KEEP; written by the kept forward and kw_mask_pack, read by the kept
// backward and kw_mask_unpack, all below) ------------------------------------------------------------------------------------------
//
// THE bit layout of the masks (keep_mask_word): per kept layer l = 0 .. D - 2, block b of 128 points and column block cb = 0 ..
// Wp / 32 - 1 one 16-bit word per (wave row wr, lane) --
//   word ((l nblk + b) Wp / 32 + cb) 256 + 64 wr + lane,   bit r = (x > 0) of row 128 b + trunk_acc_row(r, 32 wr, 4 (lane / 32)),
//                                                                            column 32 cb + lane % 32
// (x behind relu, so a NaN gives 0): Wp / 8 bytes per point and layer, over whole blocks (nblk = ceil(M / 128): a row >= M has a bit,
// of its clamped input; the backward does not read it).  A word holds exactly the 16 accumulator registers of the lane that owns
// (row, column) in either kernel, whichever column blocks cb_of deals to its wave.
struct KeepMasks {
  unsigned short* bits;             // the words of every kept layer
  long long ld;                     // words per layer: nblk * (Wp / 32) * 256
  int nblk, n_layers;               // blocks of 128 points; kept layers (D - 1)
};
__device__ __forceinline__ long long keep_mask_word(const KeepMasks& m, int layer, int blk, int ncb, int cb, int wr, int lane) {
  NSRW_CHECK(layer >= 0 && layer < m.n_layers && blk >= 0 && blk < m.nblk && cb >= 0 && cb < ncb && wr >= 0 && wr < 4 && lane >= 0 &&
             lane < 64 && (long long)m.nblk * ncb * 256 == m.ld);
  return layer * m.ld + ((long long)blk * ncb + cb) * 256 + 64 * wr + lane;
}

// ---- the FORWARD trunk, and the heads behind it --------------------------------------------------------------------------------------

// ONE body, trunk_h2_body<NJ, HEADS, WR, ENC, KEEP>, behind four kernels: kw_trunk_h2<NJ, HEADS, WR> (ENC = KEEP = false), its twin
// kw_enc_trunk_h2 (ENC), and the kept pair kw_keep_h2<NJ, HEADS> / kw_enc_keep_h2 (KEEP; WR = 4).
//
// ENC (NSRW_FLAG_EMBED_ONCHIP): the block's encodings are computed from its points (trunk_rows_encode) where the other forms fetch
// g.E -- and, in the heads form, g.ED -- from memory; nothing else differs.
//
// KEEP (NSRW_FLAG_TRUNK_KEEP): a forward pass that keeps its activations for a backward, as ONE launch too.  Row for row the pass
// that keeps nothing -- the same cadence, the same epilogue arithmetic, the same values split in place and fed to amax -- and in the epilogue it
// leaves what the backward reads: of the pts_linears rows 0 .. Dt - 2 nothing but the SIGN of each activation, one bit (KeepMasks); of
// the last pts_linears row the fp32 output in H[D - 1] = g.C (b_head masks by it through a GEMM launch), in either form; in the heads
// form views_linears.0's fp32 output in HV (b_rgb masks by it).  FA is not written: no backward reads it.
//
// (The bodies of this file are compiled for the device only: the host pass of hipcc rejects a SECOND kernel's call of a trunk_dma
// specialization that another kernel already uses -- the buffer descriptor in its signature is a device type -- and needs nothing
// of a kernel but its name.)
struct TrunkKeepArgs {              // beside a kept launch's TrunkArgs, where C = H[D - 1] and Dt = the pts_linears among the rows in either form
  float* HV; int ldHV;              // heads form: views_linears.0's output [M, ldHV]
  KeepMasks masks;
};

#ifdef __HIP_DEVICE_COMPILE__
template <int NJ, bool HEADS, int WR, bool ENC, bool KEEP>
__device__ __forceinline__ void trunk_h2_body(const TrunkArgs g, const TrunkKeepArgs a) {
  static_assert(!KEEP || WR == 4, "the kept forms have blocks of 128 points: the layout of the masks");
  static_assert((WR == 4 || (WR == 2 && NJ == 2 && !HEADS)), "the wide form is trunk-only, two column blocks a wave");
  constexpr int WC = 8 / WR, NCB = trunk_ncb<NJ, WR>(), kTrunkRows = trunk_rows<WR>();
  constexpr int kWStage = trunk_wstage<NJ, WR>(), kSH = trunk_sh<NJ, WR>(), kHPiece = kTrunkRows * kSH, kEPiece = kTrunkRows * kTrunkSE;
  constexpr int kHOff = 2 * kWStage, kEOff = kHOff + 2 * kHPiece, kLds = trunk_lds_bytes<NJ, WR>();
  constexpr int kKbeMax = kTrunkCiMax / 16, kEncIt = (kKbeMax + WC - 1) / WC;
  constexpr bool kNcbVaries = HEADS || WR != 4;       // a row's weight image may have fewer than NCB col-blocks (trunk_form_ncb)
  const TrunkCtx<kLds> c = trunk_ctx<WR, kLds>();
  // accumulator j of this wave is column block cb_of(j).  Trunk-only form: the NJ blocks of the wave's half.  Heads form: the two
  // halves take the blocks in turn, so that a head of two column blocks (views_linears.0 of a wide network) occupies all eight waves
  auto cb_of = [&](int j) { return HEADS ? 2 * j + c.wc : c.wc * NJ + j; };
  static_assert(!HEADS || WC == 2, "the heads form deals the column blocks to two halves");
  const int mblocks = (int)((g.M + kTrunkRows - 1) / kTrunkRows);      // (the host refuses more than 2^31 - 1 blocks)
  if ((int)blockIdx.x >= mblocks) return;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.img, 0, (int)g.img_bytes, 0x00020000);
  const int KBE = g.ldE >> 4, KBH = g.Wp >> 4, ncbr = g.Wp >> 5;
  NSRW_CHECK(KBE >= 2 && KBE <= kKbeMax && KBH >= 2 && KBH <= 2 * NCB && g.D >= 1);
  if constexpr (HEADS) NSRW_CHECK(g.Dt >= 1 && g.Dt < g.D && (!g.ED || ((g.ldED >> 4) >= 2 && (g.ldED >> 4) <= kKbeMax)));
  if constexpr (ENC) NSRW_CHECK(!g.E && 3 + 6 * g.pts.L <= g.ldE && (!HEADS || !g.ED || 3 + 6 * g.pts.Lv <= g.ldED));
  if constexpr (KEEP) NSRW_CHECK(g.Dt >= 2 && (HEADS || g.Dt == g.D) && a.masks.nblk == mblocks && a.masks.n_layers == g.Dt - 1);
  auto dma = [&](unsigned img_off, int KB, int kb0, int b, int ncb) { trunk_dma<NCB, kNcbVaries>(c, rsrc, g.img_bytes, img_off, KB, kb0, b, ncb); };

  float amax = 0.0f;                // largest magnitude this lane has split (encodings and activations)
  int buf = 0;
  const int row_e = c.frag0(kEOff, kTrunkSE), row_h = c.frag0(kHOff, kSH);
  {
    const TrunkLayer l0 = g.layers[0];
    dma(l0.img_off, l0.kbe + l0.kbh, 0, 0, trunk_form_ncb(l0.form));
  }
  for (int mb = blockIdx.x; mb < mblocks; mb += gridDim.x) {
    const long long m0 = (long long)mb * kTrunkRows;
    {
      f32x4 e[kEncIt][2];
      if constexpr (ENC) trunk_rows_encode<kEncIt, WC, false>(c, g.pts, KBE, m0, g.M, e);
      else trunk_rows_fetch<kEncIt, WC>(c, g.E, g.ldE, KBE, m0, g.M, e);
      trunk_rows_store<kEncIt, WC>(c, KBE, e, row_e, kEPiece, kTrunkSE, kLds, amax);
    }
    trunk_sync();                   // the encodings are written (and, in the first block, the first stage of weights has landed)
    for (int li = 0; li < g.D; ++li) {
      const TrunkLayer L = g.layers[li];
      const int ln = li + 1 < g.D ? li + 1 : 0;                       // behind the last row: layer 0 of the next block
      const unsigned img_next = g.layers[ln].img_off;
      const int kb_next = g.layers[ln].kbe + g.layers[ln].kbh;
      const int ncb_next = kNcbVaries ? trunk_form_ncb(g.layers[ln].form) : NCB;
      const int KB = L.kbe + L.kbh, nst = KB >> 1;
      const int L_ncb = trunk_form_ncb(L.form), L_ncbo = trunk_form_ncbo(L.form);
      const bool L_h_first = trunk_form_h_first(L.form), L_relu = trunk_form_relu(L.form);
      if constexpr (HEADS)
        NSRW_CHECK(L.kbe >= 0 && L.kbe <= kKbeMax && (L.kbe & 1) == 0 && L.kbh >= 0 && L.kbh <= KBH && (L.kbh & 1) == 0 && KB >= 2 &&
                   L_ncb >= 1 && L_ncb <= NCB && L_ncbo >= 1 && L_ncbo <= L_ncb);
      else
        NSRW_CHECK((L.kbe == 0 || L.kbe == KBE) && (L.kbh == 0 || L.kbh == KBH) && KB >= 2 && (KB & 1) == 0 &&
                   (!kNcbVaries || (L_ncb >= ncbr && L_ncb <= NCB && (L_ncb & 1) == 0)));
      // heads form: the accumulators of this wave that a column block of the row's output stands behind (cb_of(j) < ncbo: j < na)
      const int na = HEADS ? ((L_ncbo - c.wc + 1) >> 1 > NJ ? NJ : (L_ncbo - c.wc + 1) >> 1) : NJ;
      // heads form: the block's direction encodings are fetched in front of the last pts_linears layer and stored behind it
      f32x4 ed[kEncIt][2];
      const bool ed_here = HEADS && li + 1 == g.Dt && g.ED;
      if constexpr (HEADS) {
        if (ed_here) {
          if constexpr (ENC) trunk_rows_encode<kEncIt, WC, true>(c, g.pts, g.ldED >> 4, m0, g.M, ed);
          else trunk_rows_fetch<kEncIt, WC>(c, g.ED, g.ldED, g.ldED >> 4, m0, g.M, ed);
        }
      }
      f32x16 acc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
      for (int s = 0; s < nst; ++s) {
        const bool last = s + 1 >= nst;
        dma(last ? img_next : L.img_off, last ? kb_next : KB, last ? 0 : 2 * s + 2, buf ^ 1, last ? ncb_next : L_ncb);
        const int kb0 = 2 * s;
        bool from_e;
        int kbr;                                                         // kb0 within its image
        if (HEADS && L_h_first) { from_e = kb0 >= L.kbh; kbr = from_e ? kb0 - L.kbh : kb0; }
        else { from_e = kb0 < L.kbe; kbr = from_e ? kb0 : kb0 - L.kbe; }
        const int aoff = (from_e ? row_e : row_h) + kbr * 32;
        const int pstride = from_e ? kEPiece : kHPiece;
        if constexpr (HEADS) NSRW_CHECK(kbr >= 0 && kbr + 1 < (from_e ? L.kbe : L.kbh));
        else NSRW_CHECK(from_e ? (kb0 + 1 < KBE) : (kb0 - L.kbe >= 0 && kb0 - L.kbe + 1 < KBH));
        NSRW_CHECK(aoff >= kHOff && aoff + pstride + 32 + 16 <= kLds);
        if constexpr (HEADS) {
          if (na >= NJ) trunk_stage<NJ>(c, cb_of, acc, buf * kWStage, aoff, pstride);
          else if (NJ > 1 && na == 1) trunk_stage<1>(c, cb_of, acc, buf * kWStage, aoff, pstride);
        } else if constexpr (WR != 4) {
          if (c.wc * NJ < L_ncb) trunk_stage<NJ>(c, cb_of, acc, buf * kWStage, aoff, pstride);      // (the image holds both of the wave's col-blocks or neither)
        } else {
          trunk_stage<NJ>(c, cb_of, acc, buf * kWStage, aoff, pstride);
        }
        trunk_sync();
        buf ^= 1;
      }
      // epilogue: acc * cscale + bias, relu, to the row's destination.  Column blocks behind Wp hold zero weights and are dropped.
      const int dest = HEADS ? trunk_form_dest(L.form) : (li + 1 == g.D ? kTrunkToC : kTrunkToLds);
      const int ncbo = HEADS ? L_ncbo : ncbr;
      const bool inside = m0 + kTrunkRows <= g.M;
      // KEEP: what a kept pass leaves beside the raw outputs -- the bits of the pts_linears rows 0 .. Dt - 2, the fp32 rows of the last
      // one (H[D - 1]) and, in the heads form, of views_linears.0 (HV: the one row whose K is [hidden | encoding])
      const bool to_bits = li + 1 < g.Dt;
      float* keep_to = li + 1 == g.Dt ? g.C : (HEADS && L_h_first) ? a.HV : nullptr;
      const int keep_ld = li + 1 == g.Dt ? g.Wp : a.ldHV;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = cb_of(j);
        if (cb < ncbo) {
          const int n = cb * 32 + c.lrow;
          NSRW_CHECK(n < (HEADS ? 32 * ncbo : g.Wp) && L.bias_off + (unsigned)n < g.bias_floats);
          const float b = g.bias[L.bias_off + n];
          f32x4 v[4];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float x = acc[j][r] * L.cscale + b;
            if (!HEADS || L_relu) x = (x < 0.0f) ? 0.0f : x;             // NaN stays NaN, as through torch's relu
            v[r >> 2][r & 3] = x;
          }
          if constexpr (KEEP) {
            if (to_bits) {
              unsigned bits = 0u;
#pragma unroll
              for (int r = 0; r < 16; ++r) bits |= (v[r >> 2][r & 3] > 0.0f ? 1u : 0u) << r;
              NSRW_CHECK(cb < ncbr && dest == kTrunkToLds);
              a.masks.bits[keep_mask_word(a.masks, li, mb, ncbr, cb, c.wr, c.lane)] = (unsigned short)bits;
            }
            if (keep_to) NSRW_ROWS_OUT(c, v, keep_to, keep_ld, n, m0, g.M, inside);
          }
          if (dest == kTrunkToLds) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              u32x4 p[2];
              split8_h2(v[2 * hf], v[2 * hf + 1], p, amax);
              trunk_write_inplace<NJ, WR>(c, p, hf, n, kEOff);
            }
          } else if (!HEADS) {                                           // (a kept pass has stored its last row above)
            if constexpr (!KEEP) NSRW_ROWS_OUT(c, v, g.C, g.Wp, n, m0, g.M, inside);
          } else if (n < trunk_store_ncols(L.store)) {                   // a head's few columns of the raw outputs
            const int col0 = trunk_store_col0(L.store), ld = trunk_store_ld(L.store);
            const long long mt = m0 + 32 * c.wr + 4 * c.lh;
            NSRW_CHECK(dest == kTrunkToRaw && col0 + n < ld);
            float* rp = g.RAW + mt * ld + col0 + n;
#pragma unroll
            for (int r = 0; r < 16; ++r)
              if (inside || mt + trunk_acc_row(r) < g.M) rp[trunk_acc_row(r) * ld] = v[r >> 2][r & 3];
          }
        }
      }
      if constexpr (HEADS) {
        // behind the last pts_linears layer the encoding image is dead: the block's direction encodings take its place (the barrier
        // below stands between this and views_linears.0's reads, and every later read of the image is behind a stage's barrier)
        if (ed_here) trunk_rows_store<kEncIt, WC>(c, g.ldED >> 4, ed, row_e, kEPiece, kTrunkSE, kLds, amax);
      }
      if (dest == kTrunkToLds) trunk_lds_barrier();
    }
  }
  trunk_tail(c, amax, g.range_flag);
}
#endif
template <int NJ, bool HEADS, int WR = 4>
__global__ void __launch_bounds__(512, 1) kw_trunk_h2(const TrunkArgs g) {
#ifdef __HIP_DEVICE_COMPILE__
  trunk_h2_body<NJ, HEADS, WR, false, false>(g, TrunkKeepArgs{});
#endif
}
template <int NJ, bool HEADS, int WR = 4>
__global__ void __launch_bounds__(512, 1) kw_enc_trunk_h2(const TrunkArgs g) {
#ifdef __HIP_DEVICE_COMPILE__
  trunk_h2_body<NJ, HEADS, WR, true, false>(g, TrunkKeepArgs{});
#endif
}
template <int NJ, bool HEADS>
__global__ void __launch_bounds__(512, 1) kw_keep_h2(const TrunkArgs g, const TrunkKeepArgs a) {
#ifdef __HIP_DEVICE_COMPILE__
  trunk_h2_body<NJ, HEADS, 4, false, true>(g, a);
#endif
}
template <int NJ, bool HEADS>
__global__ void __launch_bounds__(512, 1) kw_enc_keep_h2(const TrunkArgs g, const TrunkKeepArgs a) {
#ifdef __HIP_DEVICE_COMPILE__
  trunk_h2_body<NJ, HEADS, 4, true, true>(g, a);
#endif
}

// ---- the BACKWARD trunk (NSRW_FLAG_TRUNK_BWD): kw_trunk_bwd_h2<NJ>, the input-gradient chain of net_backward_chain behind its head
// launches -- per pts layer i = D - 1 .. 0 the product g W_i[:, encoding part] (layer 0 and the skip layers; summed into GEP) and the
// product g W_i[:, hidden part] masked by relu'(h_{i-1}) (i > 0; the next g) -- over blocks of 128 points, with g in the activation
// image instead of HBM.  What differs from kw_trunk_h2<NJ, true>, whose shape it has (4 x 2 waves, the column blocks dealt to the two
// halves in turn): the weights are the transposed images Net::bwd_h / bwd_e (inside the same dImg[kH2]), every row has K = Wp from the
// activation image, and there is no encoding image: 2 x 8 NJ KiB of weights + 2 pieces x 128 x (128 NJ + 16) B = 102 400 B at
// NJ = 2, 53 248 B at NJ = 1.  Per output element it restates the chain's launches (gemm_split_body<.., NP = 2>): acc * cscale + 0.0f
// (no bias: the addition turns -0 into +0 as the chain's does), then
//   * a hidden row (kTrunkToLds): x where the fp32 mask H[i-1][row, n] > 0 and 0 elsewhere (NaN mask: 0), as kMaskEpi; split in place
//     and fed to amax -- with the block's incoming g (what b_head left in G0) every value the chain would load as an A operand;
//   * an encoding row (kTrunkToGep): the lane that owns (row, n) owns it in every such row, so the sum lives in registers -- the
//     first row sets it, every later one computes old + new (old on the left, as kAccum), and behind the last row (layer 0) it is stored:
//     ((e_first + e_next) + ...) in fp32, the chain's association.  GEP is not an A operand and is not fed to amax.
// The mask of a row is fetched in front of its stages (an encoding row fetches the mask of the hidden row behind it: branch-free,
// and the lines are in L2 when that row asks again).  Rows >= M: g is clamped on the way in, their masks read 0 (the mask and GEP go
// through buffer descriptors of the block's rows inside M), so they add nothing to amax, and their GEP stores are dropped.
struct TrunkBwdArgs {
  const float* G; int Wp;           // dL/d pre-activation of the last pts layer [M, Wp] (Chunk::G0)
  const char* img; unsigned img_bytes;
  const TrunkLayer* rows; int R;    // the backward rows of the table: kbe = 0, kbh = Wp / 16, store = the index of the mask's layer
  const float* H0; long long ldH;   // the kept activations: layer l at H0 + l * ldH, [M, Wp] each; n_masks = D - 1 of them are read
  int n_masks;
  float* GEP; int Ci;               // dL/d encoding [M, Ci]
  long long M;
  unsigned* range_flag;
};

template <int NJ> constexpr int trunk_bwd_lds_bytes() { return 2 * trunk_wstage<NJ>() + 2 * trunk_rows<4>() * trunk_sh<NJ>(); }

// ONE body, trunk_bwd_body<NJ, BITS>, behind two kernels: kw_trunk_bwd_h2<NJ> (BITS = false: the masks are the fp32 activations the
// per-layer forward kept, as above) and kw_keep_bwd_h2<NJ> (BITS = true, NSRW_FLAG_TRUNK_KEEP: behind a forward kept on chip, which
// left bits -- KeepMasks, above; g.H0 / g.ldH are not read).  Three things differ: the fetch -- NJ 16-bit words of a lane per row
// where the fp32 form has 16 NJ dword buffer loads; `live`, the registers of the lane whose row lies inside M (a word has a bit for
// a row >= M, of its clamped input, where the descriptor's extent gives the fp32 form its 0); and the select, bit r for mask > 0.
#ifdef __HIP_DEVICE_COMPILE__
template <int NJ, bool BITS>
__device__ __forceinline__ void trunk_bwd_body(const TrunkBwdArgs g, const KeepMasks masks) {
  constexpr int NCB = trunk_ncb<NJ>(), kTrunkRows = trunk_rows<4>();
  constexpr int kWStage = trunk_wstage<NJ>(), kSH = trunk_sh<NJ>(), kHPiece = kTrunkRows * kSH;
  constexpr int kHOff = 2 * kWStage, kLds = trunk_bwd_lds_bytes<NJ>();
  constexpr int kGIt = NCB;         // k16 blocks of g one wave column splits: kb = 2 i + wc < 2 NCB
  const TrunkCtx<kLds> c = trunk_ctx<4, kLds>();
  auto cb_of = [&](int j) { return 2 * j + c.wc; };
  const int mblocks = (int)((g.M + kTrunkRows - 1) / kTrunkRows);      // (the host refuses more than 2^31 - 1 blocks)
  if ((int)blockIdx.x >= mblocks) return;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.img, 0, (int)g.img_bytes, 0x00020000);
  const int KBH = g.Wp >> 4, ncbh = g.Wp >> 5, ncbe = g.Ci >> 5;
  NSRW_CHECK(KBH >= 2 && KBH <= 2 * NCB && (KBH & 1) == 0 && ncbe >= 1 && ncbe <= NCB && g.R >= 2 && g.n_masks >= 1);
  if constexpr (BITS) NSRW_CHECK(masks.nblk == mblocks && masks.n_layers == g.n_masks);
  auto dma = [&](unsigned img_off, int kb0, int b, int ncb) { trunk_dma<NCB, true>(c, rsrc, g.img_bytes, img_off, KBH, kb0, b, ncb); };

  float amax = 0.0f;                // largest magnitude this lane has split (the incoming g and every masked g2)
  int buf = 0;
  const int row_h = c.frag0(kHOff, kSH);
  // the table through the constant address space: scalar loads, so that a row's fields do not wait in the vector memory queue
  // behind the masks (the host wrote the table before the launch)
  const auto rows = (const __attribute__((address_space(4))) TrunkLayer*)(uintptr_t)g.rows;
  dma(rows[0].img_off, 0, 0, trunk_form_ncb(rows[0].form));
  for (int mb = blockIdx.x; mb < mblocks; mb += gridDim.x) {
    const long long m0 = (long long)mb * kTrunkRows;
    const int rows_in = g.M - m0 < kTrunkRows ? (int)(g.M - m0) : kTrunkRows;      // the block's rows inside M
    const int voff_m = (32 * c.wr + 4 * c.lh) * g.Wp + c.lrow;          // this lane's first element in a block of masks ...
    const int voff_e = (32 * c.wr + 4 * c.lh) * g.Ci + c.lrow;          // ... and of GEP, from column block 0 (floats)
    // BITS: the registers of this lane whose row lies inside M: a row >= M has a bit of its clamped input, which must count for nothing
    unsigned live = 0u;
    if constexpr (BITS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) live |= (trunk_acc_row(r, 32 * c.wr, 4 * c.lh) < rows_in ? 1u : 0u) << r;
    }
    {
      f32x4 e[kGIt][2];
      trunk_rows_fetch<kGIt, 2>(c, g.G, g.Wp, KBH, m0, g.M, e);
      trunk_rows_store<kGIt, 2>(c, KBH, e, row_h, kHPiece, kSH, kLds, amax);
    }
    trunk_sync();                   // g is written (and, in the first block, the first stage of weights has landed)
    float gep[NJ][16];              // dL/d encoding of this lane's elements: the sum over the encoding rows so far
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) gep[j][r] = 0.0f;
    for (int li = 0; li < g.R; ++li) {
      TrunkLayer L{};
      L.img_off = rows[li].img_off; L.kbe = rows[li].kbe; L.kbh = rows[li].kbh; L.cscale = rows[li].cscale;
      L.form = rows[li].form; L.store = rows[li].store;
      const int ln = li + 1 < g.R ? li + 1 : 0;                       // behind the last row: row 0 of the next block
      const unsigned img_next = rows[ln].img_off;
      const int ncb_next = trunk_form_ncb(rows[ln].form);
      const int nst = KBH >> 1;
      const int L_ncb = trunk_form_ncb(L.form), L_ncbo = trunk_form_ncbo(L.form), dest = trunk_form_dest(L.form);
      const bool accum = trunk_form_accum(L.form);
      NSRW_CHECK(L.kbe == 0 && L.kbh == KBH && L_ncb >= 1 && L_ncb <= NCB && L_ncbo == L_ncb && L.store >= 0 && L.store < g.n_masks &&
                 (dest == kTrunkToLds ? L_ncbo == ncbh : (dest == kTrunkToGep && L_ncbo == ncbe)));
      // the accumulators of this wave that a column block of the row's output stands behind (cb_of(j) < ncbo: j < na)
      const int na = (L_ncbo - c.wc + 1) >> 1 > NJ ? NJ : (L_ncbo - c.wc + 1) >> 1;
      // the relu mask of layer L.store at this lane's elements, branch-free: a column block behind Wp re-reads block 0 (unused).
      // BITS: one word per column block.  Else fp32, through a descriptor of the block's rows inside M: one vector offset per lane
      // and a scalar one per element; a row >= M lies behind the extent and reads 0 (its g2 is then 0 and adds nothing to amax)
      float mk[NJ][16];
      unsigned mkb[NJ];
      if constexpr (BITS) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int cbm = cb_of(j) < ncbh ? cb_of(j) : 0;
          mkb[j] = masks.bits[keep_mask_word(masks, L.store, mb, ncbh, cbm, c.wr, c.lane)] & live;
        }
      } else {
        const __amdgpu_buffer_rsrc_t mrs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(g.H0 + L.store * g.ldH + m0 * g.Wp), 0, rows_in * g.Wp * 4, 0x00020000);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int cbm = cb_of(j) < ncbh ? cb_of(j) : 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ro = trunk_acc_row(r);
            NSRW_CHECK(rows_in >= 1 && m0 + rows_in <= g.M && 32 * c.wr + 4 * c.lh + ro < kTrunkRows && cbm * 32 + c.lrow < g.Wp);
            mk[j][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(mrs, voff_m * 4, (ro * g.Wp + cbm * 32) * 4, 0));
          }
        }
      }
      f32x16 acc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
      for (int s = 0; s < nst; ++s) {
        const bool last = s + 1 >= nst;
        dma(last ? img_next : L.img_off, last ? 0 : 2 * s + 2, buf ^ 1, last ? ncb_next : L_ncb);
        const int aoff = row_h + 2 * s * 32;
        NSRW_CHECK(2 * s + 1 < KBH && aoff >= kHOff && aoff + kHPiece + 32 + 16 <= kLds);
        if (na >= NJ) trunk_stage<NJ>(c, cb_of, acc, buf * kWStage, aoff, kHPiece);
        else if (NJ > 1 && na == 1) trunk_stage<1>(c, cb_of, acc, buf * kWStage, aoff, kHPiece);
        trunk_sync();
        buf ^= 1;
      }
      // epilogue: the masked product to the activation image, or the product into the GEP sum
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = cb_of(j);
        if (cb < L_ncbo) {
          if (dest == kTrunkToLds) {
            const int n = cb * 32 + c.lrow;
            f32x4 v[4];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float x = acc[j][r] * L.cscale + 0.0f;
              bool on;
              if constexpr (BITS) on = mkb[j] >> r & 1u;
              else on = mk[j][r] > 0.0f;
              v[r >> 2][r & 3] = on ? x : 0.0f;
            }
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              u32x4 p[2];
              split8_h2(v[2 * hf], v[2 * hf + 1], p, amax);
              trunk_write_inplace<NJ, 4>(c, p, hf, n, kLds);
            }
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float x = acc[j][r] * L.cscale + 0.0f;
              gep[j][r] = accum ? gep[j][r] + x : x;
            }
          }
        }
      }
      if (dest == kTrunkToLds) trunk_lds_barrier();
    }
    // behind layer 0's row the sum is complete: GEP through a descriptor of the block's rows inside M, as the masks (a row >= M
    // lies behind the extent: its store is dropped)
    {
      const __amdgpu_buffer_rsrc_t ers = __builtin_amdgcn_make_buffer_rsrc((void*)(g.GEP + m0 * g.Ci), 0, rows_in * g.Ci * 4, 0x00020000);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = cb_of(j);
        if (cb < ncbe) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ro = trunk_acc_row(r);
            NSRW_CHECK(rows_in >= 1 && m0 + rows_in <= g.M && 32 * c.wr + 4 * c.lh + ro < kTrunkRows && cb * 32 + c.lrow < g.Ci);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gep[j][r]), ers, voff_e * 4, (ro * g.Ci + cb * 32) * 4, 0);
          }
        }
      }
    }
  }
  trunk_tail(c, amax, g.range_flag);
}
#endif
template <int NJ>
__global__ void __launch_bounds__(512, 1) kw_trunk_bwd_h2(const TrunkBwdArgs g) {
#ifdef __HIP_DEVICE_COMPILE__
  trunk_bwd_body<NJ, false>(g, KeepMasks{});
#endif
}
template <int NJ>
__global__ void __launch_bounds__(512, 1) kw_keep_bwd_h2(const TrunkBwdArgs g, const KeepMasks masks) {
#ifdef __HIP_DEVICE_COMPILE__
  trunk_bwd_body<NJ, true>(g, masks);
#endif
}

// The masks between the on-chip kernels and the per-layer chain, which keeps and reads fp32 activations; both return at once unless
// *run_if is set, like the chain's own conditional launches.  One thread per word of the layout.
//   kw_mask_pack: behind a kept forward's bf16x3 re-run, which has rewritten every H -- the bits of H[0 .. D - 2] (a row >= M: 0);
//   kw_mask_unpack: in front of a backward's bf16x3 re-run, which masks by mask > 0 -- H[0 .. D - 2] = 1.0f / 0.0f from the bits.
struct MaskArgs {
  float* H0; long long ldH;         // the kept activations: layer l at H0 + l * ldH, [M, Wp] each
  int Wp;
  long long M;
  KeepMasks masks;
  const unsigned* run_if;
};
template <bool PACK>
__device__ __forceinline__ void mask_convert(const MaskArgs& g) {
  if (*g.run_if == 0u) return;
  const int ncb = g.Wp >> 5;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x, per_layer = g.masks.ld;
  if (t >= per_layer * g.masks.n_layers) return;
  const int layer = (int)(t / per_layer), s = (int)(t & 255), wr = s >> 6, lane = s & 63;
  const long long u = (t - layer * per_layer) >> 8;
  const int blk = (int)(u / ncb), cb = (int)(u - (long long)blk * ncb);
  const long long w = keep_mask_word(g.masks, layer, blk, ncb, cb, wr, lane);
  NSRW_CHECK(w == t);
  float* hp = g.H0 + layer * g.ldH + cb * 32 + (lane & 31);
  unsigned bits = PACK ? 0u : g.masks.bits[w];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long m = (long long)blk * 128 + trunk_acc_row(r, 32 * wr, 4 * (lane >> 5));
    if (m < g.M) {
      NSRW_CHECK(cb * 32 + (lane & 31) < g.Wp);
      if (PACK) bits |= (hp[m * g.Wp] > 0.0f ? 1u : 0u) << r;
      else hp[m * g.Wp] = (bits >> r & 1u) ? 1.0f : 0.0f;
    }
  }
  if (PACK) g.masks.bits[w] = (unsigned short)bits;
}
__global__ void __launch_bounds__(256) kw_mask_pack(const MaskArgs g) { mask_convert<true>(g); }
__global__ void __launch_bounds__(256) kw_mask_unpack(const MaskArgs g) { mask_convert<false>(g); }

// ---- the bf16x3 RE-RUN of the trunk (NSRW_FLAG_TRUNK_RERUN): kw_rerun_b3<NJ, WR>, the pts_linears of the conditional bf16x3 pass that
// follows an f16x2 pass which left fp16's range, as ONE launch in place of net_forward_chain's D kw_gemm_b3 launches.  The shape and
// cadence of kw_trunk_h2<NJ, false, WR> -- trunk_dma one stage ahead, trunk_stage, trunk_sync, the in-place split, the last row's fp32
// output to C (rows of Wp floats: where the per-layer chain leaves it, what its head launches read) -- on THREE bf16 pieces per
// operand.  Per output element it restates gemm_split_body<.., NP = 3>: the accumulator from 0, the k16 blocks of [encoding | h]
// ascending, per block (2,0) (1,1) (0,2) (1,0) (0,1) (0,0) on v_mfma_f32_32x32x16_bf16, acc + bias (no cscale), relu with NaN kept,
// the next row's A pieces by split8_b3 (truncation pieces, exact) of that fp32 value; the weights are the image the chain's LDS-DMA
// moves (Mat::img[kB3], [col-block][k16 block][piece 3][64 lanes][8]).  bf16x3 has fp32's range: there is no amax, and the range word
// is only READ -- a workgroup whose *run_if is 0 returns before its first LDS-DMA or store, the contract of the chain's conditional
// launches and of kw_mask_pack.
//
// Three pieces do not fit the f16x2 tile shapes into 160 KiB, so the forms are (trunk_lds_bytes<NJ, WR, 3>):
//   Wp <= 64      <NJ = 1, WR = 4>: 128 rows x 64 columns; weights 2 x 12 288, activation 3 x 128 x 144, encoding 3 x 128 x 208 = 159 744 B
//   Wp = 96, 128  <NJ = 1, WR = 2>:  64 rows x 128 columns, 2 x 4 waves of one column block each; 2 x 24 576 + 3 x 64 x 272 + 3 x 64 x 208 = 141 312 B
// (128 rows x 128 columns would take 233 472 B).  The image of either width has exactly the form's column blocks (col_blocks rounds up
// to an even count); at Wp = 96 the fourth wave column multiplies zero weights and stores nothing.
template <int NJ, int WR>
__global__ void __launch_bounds__(512, 1) kw_rerun_b3(const TrunkArgs g, const unsigned* run_if) {
#ifdef __HIP_DEVICE_COMPILE__
  static_assert(NJ == 1 && (WR == 4 || WR == 2), "one column block a wave: 4 x 2 waves on 128 rows, or 2 x 4 on 64");
  constexpr int NP = 3, WC = 8 / WR, NCB = trunk_ncb<NJ, WR>(), kTrunkRows = trunk_rows<WR>();
  constexpr int kWStage = trunk_wstage<NJ, WR, NP>(), kSH = trunk_sh<NJ, WR>(), kHPiece = kTrunkRows * kSH, kEPiece = kTrunkRows * kTrunkSE;
  constexpr int kHOff = 2 * kWStage, kEOff = kHOff + NP * kHPiece, kLds = trunk_lds_bytes<NJ, WR, NP>();
  constexpr int kKbeMax = kTrunkCiMax / 16, kEncIt = (kKbeMax + WC - 1) / WC;
  static_assert(kEOff + NP * kEPiece == kLds && kLds <= 160 * 1024, "the three piece images behind the weight double buffer");
  if (*run_if == 0u) return;          // the f16x2 pass stayed in range: nothing is fetched, nothing is stored
  const TrunkCtx<kLds> c = trunk_ctx<WR, kLds>();
  auto cb_of = [&](int j) { return c.wc * NJ + j; };
  const int mblocks = (int)((g.M + kTrunkRows - 1) / kTrunkRows);      // (the host refuses more than 2^31 - 1 blocks)
  if ((int)blockIdx.x >= mblocks) return;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.img, 0, (int)g.img_bytes, 0x00020000);
  const int KBE = g.ldE >> 4, KBH = g.Wp >> 4, ncbr = g.Wp >> 5;
  NSRW_CHECK(KBE >= 2 && KBE <= kKbeMax && KBH >= 2 && KBH <= 2 * NCB && ncbr >= 1 && ncbr <= NCB && g.D >= 1);
  auto dma = [&](unsigned img_off, int KB, int kb0, int b) { trunk_dma<NCB, false, NP>(c, rsrc, g.img_bytes, img_off, KB, kb0, b, NCB); };

  float no_amax = 0.0f;             // (trunk_rows_store's f16x2 argument: split8_b3 has no range)
  int buf = 0;
  const int row_e = c.frag0(kEOff, kTrunkSE), row_h = c.frag0(kHOff, kSH);
  {
    const TrunkLayer l0 = g.layers[0];
    dma(l0.img_off, l0.kbe + l0.kbh, 0, 0);
  }
  for (int mb = blockIdx.x; mb < mblocks; mb += gridDim.x) {
    const long long m0 = (long long)mb * kTrunkRows;
    {
      f32x4 e[kEncIt][2];
      trunk_rows_fetch<kEncIt, WC>(c, g.E, g.ldE, KBE, m0, g.M, e);
      trunk_rows_store<kEncIt, WC, NP>(c, KBE, e, row_e, kEPiece, kTrunkSE, kLds, no_amax);
    }
    trunk_sync();                   // the encodings are written (and, in the first block, the first stage of weights has landed)
    for (int li = 0; li < g.D; ++li) {
      const TrunkLayer L = g.layers[li];
      const int ln = li + 1 < g.D ? li + 1 : 0;                       // behind the last row: layer 0 of the next block
      const unsigned img_next = g.layers[ln].img_off;
      const int kb_next = g.layers[ln].kbe + g.layers[ln].kbh;
      const int KB = L.kbe + L.kbh, nst = KB >> 1;
      NSRW_CHECK((L.kbe == 0 || L.kbe == KBE) && (L.kbh == 0 || L.kbh == KBH) && KB >= 2 && (KB & 1) == 0 &&
                 trunk_form_ncb(L.form) == NCB && trunk_form_ncb(g.layers[ln].form) == NCB);
      f32x16 acc[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
      for (int s = 0; s < nst; ++s) {
        const bool last = s + 1 >= nst;
        dma(last ? img_next : L.img_off, last ? kb_next : KB, last ? 0 : 2 * s + 2, buf ^ 1);
        const int kb0 = 2 * s;
        const bool from_e = kb0 < L.kbe;
        const int kbr = from_e ? kb0 : kb0 - L.kbe;                      // kb0 within its image
        const int aoff = (from_e ? row_e : row_h) + kbr * 32;
        const int pstride = from_e ? kEPiece : kHPiece;
        NSRW_CHECK(from_e ? (kb0 + 1 < KBE) : (kbr >= 0 && kbr + 1 < KBH));
        NSRW_CHECK(aoff >= kHOff && aoff + (NP - 1) * pstride + 32 + 16 <= kLds);
        trunk_stage<NJ, NP>(c, cb_of, acc, buf * kWStage, aoff, pstride);
        trunk_sync();
        buf ^= 1;
      }
      // epilogue: acc + bias, relu, split in place for the next row or (the last row) to C.  Column blocks behind Wp hold zero weights
      // and are dropped.
      const bool to_c = li + 1 == g.D;
      const bool inside = m0 + kTrunkRows <= g.M;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = cb_of(j);
        if (cb < ncbr) {
          const int n = cb * 32 + c.lrow;
          NSRW_CHECK(n < g.Wp && L.bias_off + (unsigned)n < g.bias_floats);
          const float b = g.bias[L.bias_off + n];
          f32x4 v[4];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float x = acc[j][r] + b;
            x = (x < 0.0f) ? 0.0f : x;                                   // NaN stays NaN, as through torch's relu
            v[r >> 2][r & 3] = x;
          }
          if (!to_c) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              u32x4 p[NP];
              split8_b3(v[2 * hf], v[2 * hf + 1], p);
              trunk_write_inplace<NJ, WR>(c, p, hf, n, kEOff);
            }
          } else {
            NSRW_ROWS_OUT(c, v, g.C, g.Wp, n, m0, g.M, inside);
          }
        }
      }
      if (!to_c) trunk_lds_barrier();
    }
  }
  trunk_drain();                    // no LDS-DMA may outlive the workgroup
#endif
}
