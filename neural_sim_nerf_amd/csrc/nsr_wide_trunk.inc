// nsr_wide_trunk.inc -- the ON-CHIP trunk of the layered renderer's f16x2 arithmetic: kw_trunk_h2<NJ, HEADS, WR>, ONE persistent launch
// that runs all D pts_linears layers (RH:99-107) of a network of packed width Wp <= 128 on a block of 128 points (WR = 2, below: Wp <= 256, 64 points), with the activation
// between two layers in LDS instead of HBM.  Included inside namespace nsrw (nsr_wide.hip), after nsr_wide_gemm.inc, whose
// arithmetic it restates per output element and must reproduce BIT FOR BIT (tests/test_gpu_wide_trunk.py, test_gpu_wide_heads.py):
//   * the accumulator of an output element starts at 0 and takes the k16 blocks of K = [encoding | h] in ascending order, per
//     block the piece products (1,0) (0,1) (0,0) on v_mfma_f32_32x32x16_f16, A operand = activation, B operand = weight -- the
//     operands are the very fragments gemm_split_body feeds: the weights are the same image (Mat::img[kH2]) moved by the same
//     LDS-DMA, the activation pieces come from split8_h2 and reach the lane (row % 32 + 32 (k % 16 / 8), element k % 8);
//   * epilogue acc * cscale + bias, relu with NaN kept; the value is then split by split8_h2's formulas (RNE fp16, exact
//     residual -> fp16) into the next layer's A pieces and fed to amax, so the range flag rises exactly when the per-layer chain's
//     next launch would raise it.  HEADS = false: only the last layer's fp32 output goes to HBM (rows of Wp floats: what the
//     heads read).
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
// Shape.  512 threads = 8 waves = two per SIMD, as 4 (rows) x 2 (columns): wave w owns rows 32 (w % 4) .. + 31 of the block and the
// NJ column blocks of half w / 4 (NJ accumulators of 32 x 32).  The accumulator has the column on the lane and the rows in
// registers, the A fragment the row on the lane and k in the register: the transposition is the epilogue's 16-bit LDS writes into
// the row-major piece images [piece][row][k], whose row stride (2 K + 16 bytes: an odd number of 16-byte slots) spreads the 16
// rows of a ds_read_b128 lane group over all 64 banks.  A layer's output overwrites its input IN PLACE: every stage ends in a
// barrier, so the last read of h is behind every wave before the first epilogue write, and one more barrier per layer puts the
// writes in front of the next layer's reads.  The weights are double-buffered in stages of two k16 blocks of every column block
// (8 NJ KiB), fetched one stage ahead ACROSS layer and block boundaries; one barrier per stage = per 6 NJ MFMAs of a wave.
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
// kw_trunk_bwd_h2<NJ> (NSRW_FLAG_TRUNK_BWD; at the end of this file, with its own description): the BACKWARD sibling, a second
// __global__ that shares split8_h2, mfma_h2w, the layout constants and the row type with the forms above and leaves them as they
// were -- the input-gradient chain of net_backward_chain (the masked products with the transposed hidden weights, the summed products
// with the transposed encoding weights) in one persistent launch over blocks of 128 points, the gradient between two layers in LDS.
#undef NSRW_FILE_TAG
#define NSRW_FILE_TAG 200000        /* a failed NSRW_CHECK of this file reports 200000 + its line (nsrw_debug_bounds_status) */

enum { kTrunkToLds = 0, kTrunkToC = 1, kTrunkToRaw = 2 };       // TrunkLayer::dest

struct TrunkLayer {                 // one pts_linears layer or, behind them, one head; the table is built by nsrw_upload_network (Net::dTrunk)
  unsigned img_off;                 // byte offset of the layer's f16x2 weight image in Net::dImg[kH2]
  unsigned bias_off;                // its bias in Net::dBias (floats)
  int kbe, kbh;                     // k16 blocks of K taken from the encoding image / from the activation image
  float cscale;                     // Mat::cscale
  // what the heads form reads on top (the trunk-only form has them fixed: encoding first, 2 NJ col-blocks, relu, the last layer to
  // C), packed into two words (trunk_form, trunk_store) so that a row stays eight scalar registers:
  //   form   bits 0-3  col-blocks of the weight image (Mat::ncb <= 2 NJ): what the LDS-DMA moves
  //          bits 4-7  col-blocks of output that are computed (the rest of the image holds zero weights)
  //          bit 8     the matrix's K order: 0 = [encoding | hidden] (pts_linears), 1 = [hidden | encoding] (views_linears.0)
  //          bit 9     epilogue: relu behind acc * cscale + bias
  //          bits 10-11  kTrunkToLds: split in place into the activation image; kTrunkToC: TrunkArgs::C; kTrunkToRaw:
  //   store  ... columns 0 .. (bits 0-7) - 1 to TrunkArgs::RAW[row * (bits 16-23) + (bits 8-15) + column]
  int form, store;
  int pad_;
};
inline int trunk_form(int ncb, int ncbo, bool h_first, bool relu, int dest) { return ncb | ncbo << 4 | (int)h_first << 8 | (int)relu << 9 | dest << 10; }
inline int trunk_store(int ncols, int col0, int ld) { return ncols | col0 << 8 | ld << 16; }

struct TrunkArgs {
  const float* E; int ldE;          // encodings [M, ldE], ldE = Ci <= kTrunkCiMax
  const char* img; unsigned img_bytes;
  const float* bias; unsigned bias_floats;
  const TrunkLayer* layers; int D;  // rows of the table: the pts_linears (trunk-only form), and the heads behind them (heads form)
  float* C; int Wp;                 // trunk-only form: the last layer's output [M, Wp]
  int Dt;                           // heads form: the pts_linears among the D rows; the direction encodings [M, ldED], ldED = Cv <=
  const float* ED; int ldED;        // kTrunkCiMax (nullptr: a network without view directions); the raw outputs the kTrunkToRaw
  float* RAW;                       // rows store to
  long long M;
  unsigned* range_flag;
};

// WR wave rows of 32 points by 8 / WR wave columns of NJ column blocks: WR = 4 the 128-row forms, WR = 2 the wide form
constexpr int kTrunkCiMax = 96;
constexpr int kTrunkSE = 2 * kTrunkCiMax + 16;                                  // row stride of an encoding piece image (bytes)
template <int WR = 4> constexpr int trunk_rows() { return 32 * WR; }             // points of a block
template <int NJ, int WR = 4> constexpr int trunk_ncb() { return 8 / WR * NJ; }  // col-blocks of a block's output
template <int NJ, int WR = 4> constexpr int trunk_sh() { return 64 * trunk_ncb<NJ, WR>() + 16; }          // ... of an activation piece image
template <int NJ, int WR = 4> constexpr int trunk_wstage() { return trunk_ncb<NJ, WR>() * 2 * 2048; }     // one stage of weights: every col-block x 2 k16 blocks
template <int NJ, int WR = 4> constexpr int trunk_lds_bytes() {
  return 2 * trunk_wstage<NJ, WR>() + 2 * trunk_rows<WR>() * trunk_sh<NJ, WR>() + 2 * trunk_rows<WR>() * kTrunkSE;
}

typedef unsigned short __attribute__((may_alias)) u16a;
typedef u32x4 __attribute__((may_alias)) u32x4a;
template <int N> struct TrunkCount { static constexpr int value = N; };          // a compile-time count as a function argument

template <int NJ, bool HEADS, int WR = 4>
__global__ void __launch_bounds__(512, 1) kw_trunk_h2(const TrunkArgs g) {
  static_assert((WR == 4 || (WR == 2 && NJ == 2 && !HEADS)), "the wide form is trunk-only, two column blocks a wave");
  constexpr int WC = 8 / WR, NCB = trunk_ncb<NJ, WR>(), kTrunkRows = trunk_rows<WR>();
  constexpr int kWStage = trunk_wstage<NJ, WR>(), kSH = trunk_sh<NJ, WR>(), kHPiece = kTrunkRows * kSH, kEPiece = kTrunkRows * kTrunkSE;
  constexpr int kHOff = 2 * kWStage, kEOff = kHOff + 2 * kHPiece, kLds = trunk_lds_bytes<NJ, WR>();
  constexpr int kKbeMax = kTrunkCiMax / 16, kEncIt = (kKbeMax + WC - 1) / WC;
  constexpr bool kNcbVaries = HEADS || WR != 4;       // a row's weight image may have fewer than NCB col-blocks (TrunkLayer::form)
  __shared__ __attribute__((aligned(1024))) char smem[kLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave & (WR - 1), wc = wave >> (WR == 4 ? 2 : 1);
  const int lrow = lane & 31, lh = lane >> 5;
  // accumulator j of this wave is column block cb_of(j).  Trunk-only form: the NJ blocks of the wave's half.  Heads form: the two
  // halves take the blocks in turn, so that a head of two column blocks (views_linears.0 of a wide network) occupies all eight waves
  auto cb_of = [&](int j) { return HEADS ? 2 * j + wc : wc * NJ + j; };
  static_assert(!HEADS || WC == 2, "the heads form deals the column blocks to two halves");
  const int mblocks = (int)((g.M + kTrunkRows - 1) / kTrunkRows);      // (the host refuses more than 2^31 - 1 blocks)
  if ((int)blockIdx.x >= mblocks) return;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.img, 0, (int)g.img_bytes, 0x00020000);
  const int KBE = g.ldE >> 4, KBH = g.Wp >> 4, ncbr = g.Wp >> 5;
  NSRW_CHECK(KBE >= 2 && KBE <= kKbeMax && KBH >= 2 && KBH <= 2 * NCB && g.D >= 1);
  if constexpr (HEADS) NSRW_CHECK(g.Dt >= 1 && g.Dt < g.D && (!g.ED || ((g.ldED >> 4) >= 2 && (g.ldED >> 4) <= kKbeMax)));

  // weights of the stage (k16 blocks kb0, kb0 + 1 of a layer with KB blocks) -> LDS buffer `buf`: 4 NJ chunks of 2 KiB, each
  // [piece 2][64 lanes][8 fp16] as the image holds it; wave w moves chunk w % (4 NJ) (NJ = 1: every chunk twice, the same bytes to
  // the same place, so that one wait serves all waves; wide form: 16 chunks, wave w moves w and w + 8, the two k16 blocks of
  // col-block w).  Heads and wide form: the image of a row may have fewer than NCB col-blocks (`ncb`); the chunks behind them are not
  // moved, and no MFMA reads them.
  auto dma = [&](unsigned img_off, int KB, int kb0, int buf, int ncb) {
#pragma unroll
    for (int c = 0; c < (2 * NCB + 7) / 8; ++c) {
      const int u = (wave + 8 * c) % (2 * NCB), cb = u % NCB, kbl = u / NCB;
      if constexpr (kNcbVaries) {
        NSRW_CHECK(ncb >= 1 && ncb <= NCB);
        if (cb >= ncb) continue;
      }
      char* l = smem + buf * kWStage + (cb * 2 + kbl) * 2048;
      const int soff = __builtin_amdgcn_readfirstlane((int)img_off + (cb * KB + kb0 + kbl) * 2048);
      NSRW_CHECK(kb0 >= 0 && kb0 + kbl < KB && soff >= 0 && (unsigned)soff + 2048u <= g.img_bytes && (buf == 0 || buf == 1) &&
                 buf * kWStage + (cb * 2 + kbl) * 2048 + 2048 <= kHOff);
#define NSRW_DMA(P)                                                                                                   \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)l, 16, lane * 16, soff, \
                                           (P) * 1024, 0) /* the immediate offsets BOTH the source and the LDS address */
      NSRW_DMA(0); NSRW_DMA(1);
#undef NSRW_DMA
    }
  };
  // this wave's LDS-DMA has landed and its LDS reads and writes are done; the barrier makes that true for the workgroup
  auto sync = [&]() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  float amax = 0.0f;                // largest magnitude this lane has split (encodings and activations)
  int buf = 0;
  const int row_e = kEOff + (32 * wr + lrow) * kTrunkSE + lh * 16;     // this lane's A fragment of k16 block 0, piece 0
  const int row_h = kHOff + (32 * wr + lrow) * kSH + lh * 16;

  // the encodings X [M, ld] (KBX k16 blocks) of the block at m0 -> the encoding image, in two steps (the heads form puts a layer
  // between them): lane = (row, k half) loads the 8 consecutive k of its fragment, as gemm_split_body's gload does, for the k16
  // blocks of its wave's column (kb % WC); rows behind M are clamped on the way in and never stored.  (Branch-free loads: a block behind KBX
  // re-reads the last one and is not written.)
  auto enc_fetch = [&](const float* X, int ld, int KBX, long long m0, f32x4 (&e)[kEncIt][2]) {
    long long am = m0 + 32 * wr + lrow;
    if (am >= g.M) am = g.M - 1;
    NSRW_CHECK(am >= 0 && am < g.M);
    const float* ep = X + am * ld + 8 * lh;
#pragma unroll
    for (int i = 0; i < kEncIt; ++i) {
      const int kb = WC * i + wc, kc = kb < KBX ? kb : KBX - 1;
      NSRW_CHECK(kc >= 0 && kc * 16 + 8 * lh + 8 <= ld);
      e[i][0] = *reinterpret_cast<const f32x4*>(ep + kc * 16);
      e[i][1] = *reinterpret_cast<const f32x4*>(ep + kc * 16 + 4);
    }
  };
  auto enc_store = [&](int KBX, const f32x4 (&e)[kEncIt][2]) {
#pragma unroll
    for (int i = 0; i < kEncIt; ++i) {
      const int kb = WC * i + wc;
      if (kb < KBX) {
        u32x4 p[2];
        split8_h2(e[i][0], e[i][1], p, amax);
        NSRW_CHECK(row_e + kEPiece + kb * 32 + 16 <= kLds);
        *reinterpret_cast<u32x4a*>(smem + row_e + kb * 32) = p[0];
        *reinterpret_cast<u32x4a*>(smem + row_e + kEPiece + kb * 32) = p[1];
      }
    }
  };

  // one stage of this wave's first NA accumulators: the A fragments at aoff (pieces pstride apart), the weights of buffer `buf`
  auto stage = [&](auto na, f32x16 (&acc)[NJ], int aoff, int pstride) {
    constexpr int NA = decltype(na)::value;
    const char* pb = smem + buf * kWStage + lane * 16;
    u32x4 fa[2][2], fb[2][NA][2];
#pragma unroll
    for (int kbl = 0; kbl < 2; ++kbl) {
#pragma unroll
      for (int q = 0; q < 2; ++q) fa[kbl][q] = *reinterpret_cast<const u32x4a*>(smem + aoff + q * pstride + kbl * 32);
#pragma unroll
      for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int q = 0; q < 2; ++q) fb[kbl][j][q] = *reinterpret_cast<const u32x4a*>(pb + (cb_of(j) * 2 + kbl) * 2048 + q * 1024);
    }
    // per accumulator the order of gemm_split_body: k16 blocks ascending, per block (1,0) (0,1) (0,0); the column blocks alternate
#pragma unroll
    for (int kbl = 0; kbl < 2; ++kbl) {
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][1], fb[kbl][j][0], acc[j]);
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][1], acc[j]);
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][0], acc[j]);
    }
    NSRW_SGB(NSRW_MASK_DSRD, 4 + 4 * NA);                                // every fragment read of the stage ahead of its MFMAs
    NSRW_SGB(NSRW_MASK_MFMA, 6 * NA);
  };

  {
    const TrunkLayer l0 = g.layers[0];
    dma(l0.img_off, l0.kbe + l0.kbh, 0, 0, l0.form & 15);
  }
  for (int mb = blockIdx.x; mb < mblocks; mb += gridDim.x) {
    const long long m0 = (long long)mb * kTrunkRows;
    {
      f32x4 e[kEncIt][2];
      enc_fetch(g.E, g.ldE, KBE, m0, e);
      enc_store(KBE, e);
    }
    sync();                         // the encodings are written (and, in the first block, the first stage of weights has landed)
    for (int li = 0; li < g.D; ++li) {
      const TrunkLayer L = g.layers[li];
      const int ln = li + 1 < g.D ? li + 1 : 0;                       // behind the last row: layer 0 of the next block
      const unsigned img_next = g.layers[ln].img_off;
      const int kb_next = g.layers[ln].kbe + g.layers[ln].kbh;
      const int ncb_next = kNcbVaries ? (g.layers[ln].form & 15) : NCB;
      const int KB = L.kbe + L.kbh, nst = KB >> 1;
      const int L_ncb = L.form & 15, L_ncbo = L.form >> 4 & 15;
      const bool L_h_first = L.form >> 8 & 1, L_relu = L.form >> 9 & 1;
      if constexpr (HEADS)
        NSRW_CHECK(L.kbe >= 0 && L.kbe <= kKbeMax && (L.kbe & 1) == 0 && L.kbh >= 0 && L.kbh <= KBH && (L.kbh & 1) == 0 && KB >= 2 &&
                   L_ncb >= 1 && L_ncb <= NCB && L_ncbo >= 1 && L_ncbo <= L_ncb);
      else
        NSRW_CHECK((L.kbe == 0 || L.kbe == KBE) && (L.kbh == 0 || L.kbh == KBH) && KB >= 2 && (KB & 1) == 0 &&
                   (!kNcbVaries || (L_ncb >= ncbr && L_ncb <= NCB && (L_ncb & 1) == 0)));
      // heads form: the accumulators of this wave that a column block of the row's output stands behind (cb_of(j) < ncbo: j < na)
      const int na = HEADS ? ((L_ncbo - wc + 1) >> 1 > NJ ? NJ : (L_ncbo - wc + 1) >> 1) : NJ;
      // heads form: the block's direction encodings are fetched in front of the last pts_linears layer and stored behind it
      f32x4 ed[kEncIt][2];
      const bool ed_here = HEADS && li + 1 == g.Dt && g.ED;
      if constexpr (HEADS) {
        if (ed_here) enc_fetch(g.ED, g.ldED, g.ldED >> 4, m0, ed);
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
          if (na >= NJ) stage(TrunkCount<NJ>(), acc, aoff, pstride);
          else if (NJ > 1 && na == 1) stage(TrunkCount<1>(), acc, aoff, pstride);
        } else if constexpr (WR != 4) {
          if (wc * NJ < L_ncb) stage(TrunkCount<NJ>(), acc, aoff, pstride);      // (the image holds both of the wave's col-blocks or neither)
        } else {
          stage(TrunkCount<NJ>(), acc, aoff, pstride);
        }
        sync();
        buf ^= 1;
      }
      // epilogue: lane owns column n, rows 8 (r / 4) + 4 (lane / 32) + r % 4 of its wave's 32.  Column blocks behind Wp hold zero weights and are dropped.
      const int dest = HEADS ? (L.form >> 10 & 3) : (li + 1 == g.D ? kTrunkToC : kTrunkToLds);
      const int ncbo = HEADS ? L_ncbo : ncbr;
      const bool inside = m0 + kTrunkRows <= g.M;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = cb_of(j);
        if (cb < ncbo) {
          const int n = cb * 32 + lrow;
          NSRW_CHECK(n < (HEADS ? 32 * ncbo : g.Wp) && L.bias_off + (unsigned)n < g.bias_floats);
          const float b = g.bias[L.bias_off + n];
          f32x4 v[4];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float x = acc[j][r] * L.cscale + b;
            if (!HEADS || L_relu) x = (x < 0.0f) ? 0.0f : x;             // NaN stays NaN, as through torch's relu
            v[r >> 2][r & 3] = x;
          }
          if (dest == kTrunkToLds) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {                             // registers 8 hf .. 8 hf + 7 -> pieces, packed pairs (r, r + 1)
              u32x4 p[2];
              split8_h2(v[2 * hf], v[2 * hf + 1], p, amax);
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) {
                const int r = 8 * hf + 2 * jj;
                const int row = 32 * wr + 8 * (r >> 2) + 4 * lh + (r & 3);
                const int off = kHOff + row * kSH + n * 2;
                NSRW_CHECK(row + 1 < kTrunkRows && n * 2 + 2 <= kSH - 16 && off + kSH + kHPiece + 2 <= kEOff);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                  *reinterpret_cast<u16a*>(smem + off + q * kHPiece) = (unsigned short)(p[q][jj] & 0xffffu);
                  *reinterpret_cast<u16a*>(smem + off + q * kHPiece + kSH) = (unsigned short)(p[q][jj] >> 16);
                }
              }
            }
          } else if (!HEADS) {
            const long long mt = m0 + 32 * wr + 4 * lh;
            float* cp = g.C + mt * g.Wp + n;
            if (inside) {
              NSRW_CHECK(mt + 27 < g.M && n < g.Wp);
#pragma unroll
              for (int r = 0; r < 16; ++r) cp[(8 * (r >> 2) + (r & 3)) * g.Wp] = v[r >> 2][r & 3];
            } else {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int ro = 8 * (r >> 2) + (r & 3);
                if (mt + ro < g.M) cp[ro * g.Wp] = v[r >> 2][r & 3];
              }
            }
          } else if (n < (L.store & 255)) {                              // a head's few columns of the raw outputs
            const int col0 = L.store >> 8 & 255, ld = L.store >> 16 & 255;
            const long long mt = m0 + 32 * wr + 4 * lh;
            NSRW_CHECK(dest == kTrunkToRaw && col0 + n < ld);
            float* rp = g.RAW + mt * ld + col0 + n;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int ro = 8 * (r >> 2) + (r & 3);
              if (inside || mt + ro < g.M) rp[ro * ld] = v[r >> 2][r & 3];
            }
          }
        }
      }
      if constexpr (HEADS) {
        // behind the last pts_linears layer the encoding image is dead: the block's direction encodings take its place (the barrier
        // below stands between this and views_linears.0's reads, and every later read of the image is behind a stage's barrier)
        if (ed_here) enc_store(g.ldED >> 4, ed);
      }
      if (dest == kTrunkToLds) {                                         // the next layer reads what every wave of its rows has written
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // no LDS-DMA may outlive the workgroup
  if (__builtin_amdgcn_ballot_w64(!(amax < 65504.0f)) != 0ull && lane == 0) atomicOr(g.range_flag, 1u);
}

// ---- the BACKWARD trunk (NSRW_FLAG_TRUNK_BWD): kw_trunk_bwd_h2<NJ>, the input-gradient chain of net_backward_chain behind its head
// launches -- per pts layer i = D - 1 .. 0 the product g W_i[:, encoding part] (layer 0 and the skip layers; summed into GEP) and the
// product g W_i[:, hidden part] masked by relu'(h_{i-1}) (i > 0; the next g) -- in ONE persistent launch over blocks of 128 points,
// with g in the activation image instead of HBM.  A sibling of kw_trunk_h2<NJ, true>: the same 4 x 2 waves with the column blocks
// dealt to the two halves in turn, the same weight stages (the transposed images Net::bwd_h / bwd_e inside the same dImg[kH2]), the
// same piece images, written in place.  No encoding image: 2 x 8 NJ KiB of weights + 2 pieces x 128 x (128 NJ + 16) B = 102 400 B at
// NJ = 2, 53 248 B at NJ = 1.  Per output element it restates the chain's launches (gemm_split_body<.., NP = 2>) bit for bit
// (tests/test_gpu_wide_trunk_bwd.py): accumulator from 0, k16 blocks ascending, per block (1,0) (0,1) (0,0), acc * cscale + 0.0f (no
// bias: the addition turns -0 into +0 as the chain's does), then
//   * a hidden row (kTrunkToLds): x where the fp32 mask H[i-1][row, n] > 0 and 0 elsewhere (NaN mask: 0), as kMaskEpi; split in place
//     by split8_h2 and fed to amax -- with the block's incoming g (what b_head left in G0) every value the chain would load as an A
//     operand, so the range flag rises exactly when the chain would raise it;
//   * an encoding row (kTrunkToGep): the lane that owns (row, n) owns it in every such row, so the sum lives in registers -- the
//     first row sets it, every later one computes old + new (old on the left, as kAccum), and behind the last row (layer 0) it is stored:
//     ((e_first + e_next) + ...) in fp32, the chain's association.  GEP is not an A operand and is not fed to amax.
// The mask of a row is fetched in front of its stages (an encoding row fetches the mask of the hidden row behind it: branch-free,
// and the lines are in L2 when that row asks again).  Rows >= M: g is clamped on the way in, their masks read 0 (the mask and GEP go
// through buffer descriptors of the block's rows inside M), so they add nothing to amax, and their GEP stores are dropped.
enum { kTrunkToGep = 3 };           // TrunkLayer::form bits 10-11 of a backward row; bit 12: the encoding row adds to the sum
inline int trunk_bwd_form(int ncbo, int dest, bool accum) { return trunk_form(ncbo, ncbo, false, false, dest) | (int)accum << 12; }

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

template <int NJ>
__global__ void __launch_bounds__(512, 1) kw_trunk_bwd_h2(const TrunkBwdArgs g) {
  constexpr int NCB = trunk_ncb<NJ>(), kTrunkRows = trunk_rows<4>();
  constexpr int kWStage = trunk_wstage<NJ>(), kSH = trunk_sh<NJ>(), kHPiece = kTrunkRows * kSH;
  constexpr int kHOff = 2 * kWStage, kLds = trunk_bwd_lds_bytes<NJ>();
  constexpr int kGIt = NCB;         // k16 blocks of g one wave column splits: kb = 2 i + wc < 2 NCB
  __shared__ __attribute__((aligned(1024))) char smem[kLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave & 3, wc = wave >> 2;
  const int lrow = lane & 31, lh = lane >> 5;
  auto cb_of = [&](int j) { return 2 * j + wc; };                      // the two halves take the column blocks in turn (heads form)
  const int mblocks = (int)((g.M + kTrunkRows - 1) / kTrunkRows);      // (the host refuses more than 2^31 - 1 blocks)
  if ((int)blockIdx.x >= mblocks) return;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.img, 0, (int)g.img_bytes, 0x00020000);
  const int KBH = g.Wp >> 4, ncbh = g.Wp >> 5, ncbe = g.Ci >> 5;
  NSRW_CHECK(KBH >= 2 && KBH <= 2 * NCB && (KBH & 1) == 0 && ncbe >= 1 && ncbe <= NCB && g.R >= 2 && g.n_masks >= 1);

  // kw_trunk_h2's stage of weights, of a row whose image has its first `ncb` col-blocks moved
  auto dma = [&](unsigned img_off, int kb0, int buf, int ncb) {
#pragma unroll
    for (int c = 0; c < (2 * NCB + 7) / 8; ++c) {
      const int u = (wave + 8 * c) % (2 * NCB), cb = u % NCB, kbl = u / NCB;
      NSRW_CHECK(ncb >= 1 && ncb <= NCB);
      if (cb >= ncb) continue;
      char* l = smem + buf * kWStage + (cb * 2 + kbl) * 2048;
      const int soff = __builtin_amdgcn_readfirstlane((int)img_off + (cb * KBH + kb0 + kbl) * 2048);
      NSRW_CHECK(kb0 >= 0 && kb0 + kbl < KBH && soff >= 0 && (unsigned)soff + 2048u <= g.img_bytes && (buf == 0 || buf == 1) &&
                 buf * kWStage + (cb * 2 + kbl) * 2048 + 2048 <= kHOff);
#define NSRW_DMA(P)                                                                                                   \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)l, 16, lane * 16, soff, \
                                           (P) * 1024, 0) /* the immediate offsets BOTH the source and the LDS address */
      NSRW_DMA(0); NSRW_DMA(1);
#undef NSRW_DMA
    }
  };
  // this wave's LDS-DMA and global loads have landed and its LDS reads and writes are done; the barrier makes that true for the workgroup
  auto sync = [&]() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  float amax = 0.0f;                // largest magnitude this lane has split (the incoming g and every masked g2)
  int buf = 0;
  const int row_h = kHOff + (32 * wr + lrow) * kSH + lh * 16;          // this lane's A fragment of k16 block 0, piece 0

  // the block's g -> the activation image, as enc_fetch / enc_store put the encodings into theirs: lane = (row, k half) loads the 8
  // consecutive k of its fragment for the k16 blocks of its wave's column (kb % 2)
  auto g_fetch = [&](long long m0, f32x4 (&e)[kGIt][2]) {
    long long am = m0 + 32 * wr + lrow;
    if (am >= g.M) am = g.M - 1;
    NSRW_CHECK(am >= 0 && am < g.M);
    const float* gp = g.G + am * g.Wp + 8 * lh;
#pragma unroll
    for (int i = 0; i < kGIt; ++i) {
      const int kb = 2 * i + wc, kc = kb < KBH ? kb : KBH - 1;
      NSRW_CHECK(kc >= 0 && kc * 16 + 8 * lh + 8 <= g.Wp);
      e[i][0] = *reinterpret_cast<const f32x4*>(gp + kc * 16);
      e[i][1] = *reinterpret_cast<const f32x4*>(gp + kc * 16 + 4);
    }
  };
  auto g_store = [&](const f32x4 (&e)[kGIt][2]) {
#pragma unroll
    for (int i = 0; i < kGIt; ++i) {
      const int kb = 2 * i + wc;
      if (kb < KBH) {
        u32x4 p[2];
        split8_h2(e[i][0], e[i][1], p, amax);
        NSRW_CHECK(kb * 32 + lh * 16 + 16 <= kSH - 16 && row_h + kHPiece + kb * 32 + 16 <= kLds);
        *reinterpret_cast<u32x4a*>(smem + row_h + kb * 32) = p[0];
        *reinterpret_cast<u32x4a*>(smem + row_h + kHPiece + kb * 32) = p[1];
      }
    }
  };

  // kw_trunk_h2's stage: this wave's first NA accumulators, the A fragments at aoff, the weights of buffer `buf`
  auto stage = [&](auto na, f32x16 (&acc)[NJ], int aoff) {
    constexpr int NA = decltype(na)::value;
    const char* pb = smem + buf * kWStage + lane * 16;
    u32x4 fa[2][2], fb[2][NA][2];
#pragma unroll
    for (int kbl = 0; kbl < 2; ++kbl) {
#pragma unroll
      for (int q = 0; q < 2; ++q) fa[kbl][q] = *reinterpret_cast<const u32x4a*>(smem + aoff + q * kHPiece + kbl * 32);
#pragma unroll
      for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int q = 0; q < 2; ++q) fb[kbl][j][q] = *reinterpret_cast<const u32x4a*>(pb + (cb_of(j) * 2 + kbl) * 2048 + q * 1024);
    }
    // per accumulator the order of gemm_split_body: k16 blocks ascending, per block (1,0) (0,1) (0,0); the column blocks alternate
#pragma unroll
    for (int kbl = 0; kbl < 2; ++kbl) {
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][1], fb[kbl][j][0], acc[j]);
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][1], acc[j]);
#pragma unroll
      for (int j = 0; j < NA; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][0], acc[j]);
    }
    NSRW_SGB(NSRW_MASK_DSRD, 4 + 4 * NA);                                // every fragment read of the stage ahead of its MFMAs
    NSRW_SGB(NSRW_MASK_MFMA, 6 * NA);
  };

  // the table through the constant address space: scalar loads, so that a row's fields do not wait in the vector memory queue
  // behind the masks (the host wrote the table before the launch)
  const auto rows = (const __attribute__((address_space(4))) TrunkLayer*)(uintptr_t)g.rows;
  dma(rows[0].img_off, 0, 0, rows[0].form & 15);
  for (int mb = blockIdx.x; mb < mblocks; mb += gridDim.x) {
    const long long m0 = (long long)mb * kTrunkRows;
    const int rows_in = g.M - m0 < kTrunkRows ? (int)(g.M - m0) : kTrunkRows;      // the block's rows inside M
    const int voff_m = (32 * wr + 4 * lh) * g.Wp + lrow;                // this lane's first element in a block of masks ...
    const int voff_e = (32 * wr + 4 * lh) * g.Ci + lrow;                // ... and of GEP, from column block 0 (floats)
    {
      f32x4 e[kGIt][2];
      g_fetch(m0, e);
      g_store(e);
    }
    sync();                         // g is written (and, in the first block, the first stage of weights has landed)
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
      const int ncb_next = rows[ln].form & 15;
      const int nst = KBH >> 1;
      const int L_ncb = L.form & 15, L_ncbo = L.form >> 4 & 15, dest = L.form >> 10 & 3;
      const bool accum = L.form >> 12 & 1;
      NSRW_CHECK(L.kbe == 0 && L.kbh == KBH && L_ncb >= 1 && L_ncb <= NCB && L_ncbo == L_ncb && L.store >= 0 && L.store < g.n_masks &&
                 (dest == kTrunkToLds ? L_ncbo == ncbh : (dest == kTrunkToGep && L_ncbo == ncbe)));
      // the accumulators of this wave that a column block of the row's output stands behind (cb_of(j) < ncbo: j < na)
      const int na = (L_ncbo - wc + 1) >> 1 > NJ ? NJ : (L_ncbo - wc + 1) >> 1;
      // the relu mask of layer L.store at this lane's elements, through a descriptor of the block's rows inside M: branch-free, one
      // vector offset per lane and a scalar one per element; a row >= M lies behind the extent and reads 0 (its g2 is then 0 and
      // adds nothing to amax), a column block behind Wp re-reads block 0 (unused)
      float mk[NJ][16];
      {
        const __amdgpu_buffer_rsrc_t mrs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(g.H0 + L.store * g.ldH + m0 * g.Wp), 0, rows_in * g.Wp * 4, 0x00020000);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int cbm = cb_of(j) < ncbh ? cb_of(j) : 0;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ro = 8 * (r >> 2) + (r & 3);
            NSRW_CHECK(rows_in >= 1 && m0 + rows_in <= g.M && 32 * wr + 4 * lh + ro < kTrunkRows && cbm * 32 + lrow < g.Wp);
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
        if (na >= NJ) stage(TrunkCount<NJ>(), acc, aoff);
        else if (NJ > 1 && na == 1) stage(TrunkCount<1>(), acc, aoff);
        sync();
        buf ^= 1;
      }
      // epilogue: lane owns column n, rows 8 (r / 4) + 4 (lane / 32) + r % 4 of its wave's 32
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = cb_of(j);
        if (cb < L_ncbo) {
          if (dest == kTrunkToLds) {
            const int n = cb * 32 + lrow;
            f32x4 v[4];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float x = acc[j][r] * L.cscale + 0.0f;
              v[r >> 2][r & 3] = (mk[j][r] > 0.0f) ? x : 0.0f;
            }
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {                             // registers 8 hf .. 8 hf + 7 -> pieces, packed pairs (r, r + 1)
              u32x4 p[2];
              split8_h2(v[2 * hf], v[2 * hf + 1], p, amax);
#pragma unroll
              for (int jj = 0; jj < 4; ++jj) {
                const int r = 8 * hf + 2 * jj;
                const int row = 32 * wr + 8 * (r >> 2) + 4 * lh + (r & 3);
                const int off = kHOff + row * kSH + n * 2;
                NSRW_CHECK(row + 1 < kTrunkRows && n * 2 + 2 <= kSH - 16 && off + kSH + kHPiece + 2 <= kLds);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                  *reinterpret_cast<u16a*>(smem + off + q * kHPiece) = (unsigned short)(p[q][jj] & 0xffffu);
                  *reinterpret_cast<u16a*>(smem + off + q * kHPiece + kSH) = (unsigned short)(p[q][jj] >> 16);
                }
              }
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
      if (dest == kTrunkToLds) {                                         // the next row reads what every wave of its rows has written
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
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
            const int ro = 8 * (r >> 2) + (r & 3);
            NSRW_CHECK(rows_in >= 1 && m0 + rows_in <= g.M && 32 * wr + 4 * lh + ro < kTrunkRows && cb * 32 + lrow < g.Ci);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gep[j][r]), ers, voff_e * 4, (ro * g.Ci + cb * 32) * 4, 0);
          }
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // no LDS-DMA may outlive the workgroup
  if (__builtin_amdgcn_ballot_w64(!(amax < 65504.0f)) != 0ull && lane == 0) atomicOr(g.range_flag, 1u);
}
