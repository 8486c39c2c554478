// nsr_wide_trunk.inc -- the ON-CHIP trunk of the layered renderer's f16x2 arithmetic: kw_trunk_h2<NJ>, ONE persistent launch that
// runs all D pts_linears layers (RH:99-107) of a network of packed width Wp <= 128 on a block of 128 points, with the activation
// between two layers in LDS instead of HBM.  Included inside namespace nsrw (nsr_wide.hip), after nsr_wide_gemm.inc, whose
// arithmetic it restates per output element and must reproduce BIT FOR BIT (tests/test_gpu_wide_trunk.py):
//   * the accumulator of an output element starts at 0 and takes the k16 blocks of K = [encoding | h] in ascending order, per
//     block the piece products (1,0) (0,1) (0,0) on v_mfma_f32_32x32x16_f16, A operand = activation, B operand = weight -- the
//     operands are the very fragments gemm_split_body feeds: the weights are the same image (Mat::img[kH2]) moved by the same
//     LDS-DMA, the activation pieces come from split8_h2 and reach the lane (row % 32 + 32 (k % 16 / 8), element k % 8);
//   * epilogue acc * cscale + bias, relu with NaN kept; the value is then split by split8_h2's formulas (RNE fp16, exact
//     residual -> fp16) into the next layer's A pieces and fed to amax, so the range flag rises exactly when the per-layer chain's
//     next launch would raise it.  Only the last layer's fp32 output goes to HBM (rows of Wp floats: what the heads read).
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
// 128 x 208 B (Ci <= 96) -- 155 648 B at NJ = 2, 106 496 B at NJ = 1.
#undef NSRW_FILE_TAG
#define NSRW_FILE_TAG 200000        /* a failed NSRW_CHECK of this file reports 200000 + its line (nsrw_debug_bounds_status) */

struct TrunkLayer {                 // one pts_linears layer; the table is built by nsrw_upload_network (Net::dTrunk)
  unsigned img_off;                 // byte offset of the layer's f16x2 weight image in Net::dImg[kH2]
  unsigned bias_off;                // its bias in Net::dBias (floats)
  int kbe, kbh;                     // k16 blocks of K taken from the encoding (layer 0 and skip layers) / from the previous layer
  float cscale;                     // Mat::cscale
  int pad_[3];
};

struct TrunkArgs {
  const float* E; int ldE;          // encodings [M, ldE], ldE = Ci <= kTrunkCiMax
  const char* img; unsigned img_bytes;
  const float* bias; unsigned bias_floats;
  const TrunkLayer* layers; int D;
  float* C; int Wp;                 // the last layer's output [M, Wp]
  long long M;
  unsigned* range_flag;
};

constexpr int kTrunkRows = 128, kTrunkCiMax = 96;
constexpr int kTrunkSE = 2 * kTrunkCiMax + 16;                                  // row stride of an encoding piece image (bytes)
template <int NJ> constexpr int trunk_sh() { return 2 * 64 * NJ + 16; }          // ... of an activation piece image
template <int NJ> constexpr int trunk_wstage() { return 2 * NJ * 2 * 2048; }     // one stage of weights: 2 NJ col-blocks x 2 k16 blocks
template <int NJ> constexpr int trunk_lds_bytes() { return 2 * trunk_wstage<NJ>() + 2 * kTrunkRows * trunk_sh<NJ>() + 2 * kTrunkRows * kTrunkSE; }

typedef unsigned short __attribute__((may_alias)) u16a;
typedef u32x4 __attribute__((may_alias)) u32x4a;

template <int NJ>
__global__ void __launch_bounds__(512, 1) kw_trunk_h2(const TrunkArgs g) {
  constexpr int NCB = 2 * NJ;
  constexpr int kWStage = trunk_wstage<NJ>(), kSH = trunk_sh<NJ>(), kHPiece = kTrunkRows * kSH, kEPiece = kTrunkRows * kTrunkSE;
  constexpr int kHOff = 2 * kWStage, kEOff = kHOff + 2 * kHPiece, kLds = trunk_lds_bytes<NJ>();
  constexpr int kKbeMax = kTrunkCiMax / 16;
  __shared__ __attribute__((aligned(1024))) char smem[kLds];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave & 3, wc = wave >> 2;
  const int lrow = lane & 31, lh = lane >> 5;
  const int mblocks = (int)((g.M + kTrunkRows - 1) / kTrunkRows);      // (the host refuses more than 2^31 - 1 blocks)
  if ((int)blockIdx.x >= mblocks) return;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)g.img, 0, (int)g.img_bytes, 0x00020000);
  const int KBE = g.ldE >> 4, KBH = g.Wp >> 4, ncbr = g.Wp >> 5;
  NSRW_CHECK(KBE >= 2 && KBE <= kKbeMax && KBH >= 2 && KBH <= 8 * NJ && g.D >= 1);

  // weights of the stage (k16 blocks kb0, kb0 + 1 of a layer with KB blocks) -> LDS buffer `buf`: 4 NJ chunks of 2 KiB, each
  // [piece 2][64 lanes][8 fp16] as the image holds it; wave w moves chunk w % (4 NJ) (NJ = 1: every chunk twice, the same bytes to
  // the same place, so that one wait serves all waves)
  auto dma = [&](unsigned img_off, int KB, int kb0, int buf) {
    const int u = wave % (2 * NCB), cb = u % NCB, kbl = u / NCB;
    char* l = smem + buf * kWStage + (cb * 2 + kbl) * 2048;
    const int soff = __builtin_amdgcn_readfirstlane((int)img_off + (cb * KB + kb0 + kbl) * 2048);
    NSRW_CHECK(kb0 >= 0 && kb0 + kbl < KB && soff >= 0 && (unsigned)soff + 2048u <= g.img_bytes && (buf == 0 || buf == 1));
#define NSRW_DMA(P)                                                                                                   \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)l, 16, lane * 16, soff, \
                                           (P) * 1024, 0) /* the immediate offsets BOTH the source and the LDS address */
    NSRW_DMA(0); NSRW_DMA(1);
#undef NSRW_DMA
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
  {
    const TrunkLayer l0 = g.layers[0];
    dma(l0.img_off, l0.kbe + l0.kbh, 0, 0);
  }
  for (int mb = blockIdx.x; mb < mblocks; mb += gridDim.x) {
    const long long m0 = (long long)mb * kTrunkRows;
    {
      // the block's encodings: lane = (row, k half) loads the 8 consecutive k of its fragment, as gemm_split_body's gload does, for
      // the k16 blocks of its wave's parity; rows behind M are clamped on the way in and never stored.  (Branch-free loads: a
      // block behind KBE re-reads the last one and is not written.)
      long long am = m0 + 32 * wr + lrow;
      if (am >= g.M) am = g.M - 1;
      NSRW_CHECK(am >= 0 && am < g.M);
      const float* ep = g.E + am * g.ldE + 8 * lh;
      f32x4 e[kKbeMax / 2][2];
#pragma unroll
      for (int i = 0; i < kKbeMax / 2; ++i) {
        const int kb = 2 * i + wc, kc = kb < KBE ? kb : KBE - 1;
        NSRW_CHECK(kc >= 0 && kc * 16 + 8 * lh + 8 <= g.ldE);
        e[i][0] = *reinterpret_cast<const f32x4*>(ep + kc * 16);
        e[i][1] = *reinterpret_cast<const f32x4*>(ep + kc * 16 + 4);
      }
#pragma unroll
      for (int i = 0; i < kKbeMax / 2; ++i) {
        const int kb = 2 * i + wc;
        if (kb < KBE) {
          u32x4 p[2];
          split8_h2(e[i][0], e[i][1], p, amax);
          NSRW_CHECK(row_e + kEPiece + kb * 32 + 16 <= kLds);
          *reinterpret_cast<u32x4a*>(smem + row_e + kb * 32) = p[0];
          *reinterpret_cast<u32x4a*>(smem + row_e + kEPiece + kb * 32) = p[1];
        }
      }
    }
    sync();                         // the encodings are written (and, in the first block, the first stage of weights has landed)
    for (int li = 0; li < g.D; ++li) {
      const TrunkLayer L = g.layers[li];
      const int ln = li + 1 < g.D ? li + 1 : 0;                       // behind the last layer: layer 0 of the next block
      const unsigned img_next = g.layers[ln].img_off;
      const int kb_next = g.layers[ln].kbe + g.layers[ln].kbh;
      const int KB = L.kbe + L.kbh, nst = KB >> 1;
      NSRW_CHECK((L.kbe == 0 || L.kbe == KBE) && (L.kbh == 0 || L.kbh == KBH) && KB >= 2 && (KB & 1) == 0);
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
        const int aoff = from_e ? row_e + kb0 * 32 : row_h + (kb0 - L.kbe) * 32;
        const int pstride = from_e ? kEPiece : kHPiece;
        NSRW_CHECK(from_e ? (kb0 + 1 < KBE) : (kb0 - L.kbe >= 0 && kb0 - L.kbe + 1 < KBH));
        NSRW_CHECK(aoff >= kHOff && aoff + pstride + 32 + 16 <= kLds);
        const char* pb = smem + buf * kWStage + (wc * NJ) * 4096 + lane * 16;
        u32x4 fa[2][2], fb[2][NJ][2];
#pragma unroll
        for (int kbl = 0; kbl < 2; ++kbl) {
#pragma unroll
          for (int q = 0; q < 2; ++q) fa[kbl][q] = *reinterpret_cast<const u32x4a*>(smem + aoff + q * pstride + kbl * 32);
#pragma unroll
          for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 2; ++q) fb[kbl][j][q] = *reinterpret_cast<const u32x4a*>(pb + (j * 2 + kbl) * 2048 + q * 1024);
        }
        // per accumulator the order of gemm_split_body: k16 blocks ascending, per block (1,0) (0,1) (0,0); the column blocks alternate
#pragma unroll
        for (int kbl = 0; kbl < 2; ++kbl) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] = mfma_h2w(fa[kbl][1], fb[kbl][j][0], acc[j]);
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][1], acc[j]);
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[j] = mfma_h2w(fa[kbl][0], fb[kbl][j][0], acc[j]);
        }
        NSRW_SGB(NSRW_MASK_DSRD, 4 + 4 * NJ);                            // every fragment read of the stage ahead of its MFMAs
        NSRW_SGB(NSRW_MASK_MFMA, 6 * NJ);
        sync();
        buf ^= 1;
      }
      // epilogue: lane owns column n, rows 8 (r / 4) + 4 (lane / 32) + r % 4 of its wave's 32.  Column blocks behind Wp hold zero weights and are dropped.
      const bool to_hbm = li + 1 == g.D;
      const bool inside = m0 + kTrunkRows <= g.M;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int cb = wc * NJ + j;
        if (cb < ncbr) {
          const int n = cb * 32 + lrow;
          NSRW_CHECK(n < g.Wp && L.bias_off + (unsigned)n < g.bias_floats);
          const float b = g.bias[L.bias_off + n];
          f32x4 v[4];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float x = acc[j][r] * L.cscale + b;
            x = (x < 0.0f) ? 0.0f : x;                                   // NaN stays NaN, as through torch's relu
            v[r >> 2][r & 3] = x;
          }
          if (!to_hbm) {
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
          } else {
            const long long mt = m0 + 32 * wr + 4 * lh;
            float* cp = g.C + mt * g.Wp + n;
            if (inside) {
              NSRW_CHECK(mt + 27 < g.M);
#pragma unroll
              for (int r = 0; r < 16; ++r) cp[(8 * (r >> 2) + (r & 3)) * g.Wp] = v[r >> 2][r & 3];
            } else {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int ro = 8 * (r >> 2) + (r & 3);
                if (mt + ro < g.M) cp[ro * g.Wp] = v[r >> 2][r & 3];
              }
            }
          }
        }
      }
      if (!to_hbm) {                                                     // the next layer reads what every wave of its rows has written
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                       // no LDS-DMA may outlive the workgroup
  if (__builtin_amdgcn_ballot_w64(!(amax < 65504.0f)) != 0ull && lane == 0) atomicOr(g.range_flag, 1u);
}
