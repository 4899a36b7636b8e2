// Fused whole-model BERT-tiny forward: ONE workgroup per log line.
//
// The flagship detector config (BASELINE.json config 5) is tiny enough
// that the idiomatic MI355X mapping is a per-line megakernel: all
// activations for one line (S=64 tokens, hidden 128) live in LDS for the
// whole forward pass; the model's weights (~600 KB) are read through the
// XCD L2s and shared by every workgroup; HBM traffic is line bytes in +
// one f32 score out.
//
// v3 design notes (PMC-driven, profiles/*):
//  * v1 (layered kernels) was HBM-bound on inter-op traffic (74% GEMM).
//  * v2 (fused, 118 KiB arena, 1 block/CU) showed MemUnitStalled~0 and
//    VALUBusy 33%: bulk-synchronous phases at 1 block/CU leave the CU
//    idle at every barrier. This version shrinks the arena to ~70 KiB so
//    TWO blocks co-reside per CU - one block's barrier idle overlaps the
//    other block's compute. 8 waves/block (512 thr), VGPR<=128 keeps both
//    resident (4 waves/SIMD from two independent barrier domains).
//  * arena cuts: qkv buffer holds Q|K only (V written transposed to vt
//    during the qkv GEMM epilogue); FFN runs in two K=256 halves that
//    accumulate into x; the attention P tile aliases the (dead) Q|K area.
//  * pair-chunked weight fragments: one L2 B-fragment load feeds two
//    independent MFMA chains.
//
// v4: epilogue / softmax instruction diet (profiles/r14). The kernel is
// instruction-issue-bound at 4 waves/SIMD, and most of the issue was not
// MFMA: the W1 GEMM carried 686 other vector instructions around 32 MFMAs.
//  * gelu_f32 (common.h): hardware reciprocal + base-2 exp instead of the
//    IEEE division expansion (-7.1% step time on its own).
//  * operand-swapped MFMA, mfma(weight, activation): the lane owns one row
//    and FOUR CONSECUTIVE columns, so every row-major epilogue is one
//    8-byte LDS store (and one 8-byte residual load) per fragment instead
//    of four 2-byte ones, and the bias is one 16-byte load that seeds the
//    accumulators. The qkv GEMM picks swapped (Q|K) or plain (V, written
//    transposed) once per wave on a scalar (-8.2%).
//  * attention the same way: S^T and O^T tiles put a whole query in the
//    lanes lane&15, so softmax reductions are in-lane plus two cross-lane
//    steps, 1/sum is already where it is used, P and O leave as 8-byte
//    stores (-4.8%).
//  * the adjacent values invite v_pk_mul_f32 / v_pk_add_f32 (16 in W1, 8
//    per residual GEMM). Keeping them apart needs inline-asm arithmetic,
//    which steps outside the compiler's hazard handling (a v_rcp_f32
//    result read too early) and computed garbage: not done (r14).
//
// Fixed geometry (asserted host-side): S=64 tokens, H=128, 2 heads
// (Dh=64), FFN=512, arbitrary layer count.
#include "common.h"
#include "kernels.h"  // geometry, blob offsets, BF_LDS_BYTES, launchers

// Explicit LDS address-space typing: the noinline block_gemm receives the
// arena pointers as arguments, and a generic (flat) short* there makes
// hipcc emit flat_load for what are really LDS reads (35 flat_load in the
// .s before this change). AS(3) pointers guarantee ds_* lowering.
typedef __attribute__((address_space(3))) short lds_short;
typedef __attribute__((address_space(1))) const short glob_cshort;
typedef __attribute__((address_space(1))) const float glob_cfloat;
typedef __attribute__((address_space(3))) const short lds_cshort;
typedef __attribute__((address_space(3))) float lds_float;

#define BF_THREADS (BF_WAVES * DMX_WAVE)

// LDS strides (elements); +8 pads keep rows 16-B aligned and bank-spread
#define XS (BF_H + 8)       // 136, x rows
// QKS at +16 (not +8): stride 136 dw = 8 mod 64 makes the FFN W2 /
// attention A-fragment ds_read_b128 groups conflict-free (PMC: FFN's
// 6.98B conflict cycles are 100% A-reads — probe ABL=2 zeroes them).
// Q|K (64x272=17408) and FFN halves still fit inside BUF_ELEMS (17920,
// sized by the P+O region), so this costs ZERO extra LDS. Measured
// NEUTRAL on wall (7.30M both ways): in this latency-bound regime the
// conflict cycles hide under the operand waits — kept because it is
// free and removes them from every future profile.
#define QKS (2 * BF_H + 16)  // 272, Q|K rows and FFN-half rows
#define VTS (BF_S + 8)      // 72, transposed-V and P rows
#define O_OFF (BF_WAVES * 16 * VTS)    // 9216: attn-out after the P tiles
#define BUF_ELEMS (O_OFF + BF_S * XS)  // 17920 = P+O (>= QK 17408)

// arena: x [S][XS] | buf | Vt [2*Dh][VTS] (bf16), then [H] f32 pooling
static_assert(BF_LDS_BYTES ==
                  (BF_S * XS + BUF_ELEMS + 2 * BF_DH * VTS) * sizeof(short) +
                      BF_H * sizeof(float),
              "kernels.h BF_LDS_BYTES out of step with the LDS strides");

// The GEMM and attention epilogues move four bf16 per lane with one 8-byte
// LDS access at column offsets that are multiples of 4, so every row
// stride and every region offset they are used with must be a multiple of
// 4 elements (the arena base is 16-byte aligned).
static_assert(XS % 4 == 0 && QKS % 4 == 0 && VTS % 4 == 0,
              "8-byte LDS access: row strides must be multiples of 4");
static_assert(O_OFF % 4 == 0 && (BF_S * XS) % 4 == 0 && BUF_ELEMS % 4 == 0 &&
                  (BF_WAVES * 16 * VTS) % 4 == 0 && (16 * VTS) % 4 == 0,
              "8-byte LDS access: buf, vt, P-tile and O offsets must be "
              "multiples of 4");
// ... and the swapped GEMMs fetch four biases with one 16-byte load: every
// bias vector must start a multiple of 4 floats into the (16-byte aligned,
// checked by the bindings) blob.
static_assert(FB_BQKV % 4 == 0 && FB_BO % 4 == 0 && FB_B1 % 4 == 0 &&
                  FB_B2 % 4 == 0 && FB_SIZE % 4 == 0 &&
                  (BF_FFN / 2) % 4 == 0,
              "16-byte bias loads: bias offsets must be multiples of 4");

typedef __attribute__((address_space(3))) short4v lds_short4;

// four f32 -> four bf16 (RNE, as f32_to_bf16) as two v_cvt_pk_bf16_f32;
// element-wise f32_to_bf16 left the compiler re-pairing halves with
// v_perm_b32 / v_alignbit_b32
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
static __device__ __forceinline__ short4v pack_bf16x4(f32x4 v) {
  return __builtin_bit_cast(short4v, __builtin_convertvector(v, bf16x4_t));
}

// ---- in-block GEMM: out = act(in_lds[64][K] @ Wt[N][WTS] + bias) ---------
// MODE 0: write out_lds[m][n]; MODE 1 (qkv): n<2H -> out (Q|K), else vt
// transposed; MODE 2: x[m][n] += v (residual-accumulate). ACT 1 = GELU.
// ABL (perf-ablation diagnostics, numerically wrong on purpose):
// bit 1 = B operand from an opaque register instead of the L2 weight
// load (removes vmcnt parks); bit 2 = A operand from a register instead
// of the LDS read (removes lgkmcnt parks). Epilogue stores stay, so the
// MFMA chains cannot be dead-code-eliminated (guide §5.4 rule 17).
// All pointers __restrict__: without it the epilogue's LDS stores
// between quads alias the activation reads for the analyzer (the
// pointers arrive as opaque noinline args), so the compiler re-reads
// every A fragment per quad (32 ds_reads for 32 MFMAs in the .s) and
// cannot hoist reads across the quad boundary. The caller guarantees
// in_lds never overlaps this GEMM's outputs.
//
// Operand order (SWAP). The 16x16x32 bf16 A and B fragment layouts are the
// same function of the lane (row or column lane&15, k (lane>>4)*8..+7), so
// mfma(weight, activation) yields the transposed tile of mfma(activation,
// weight): the lane then owns ONE row m = fm*16 + (lane&15) and FOUR
// CONSECUTIVE columns n0 = fn*16 + (lane>>4)*4 + r. Row-major outputs
// (MODE 0, MODE 2, the Q|K columns of MODE 1) run swapped: the bias is one
// 16-byte load that seeds the accumulators (no epilogue add), the four
// results leave as one 8-byte LDS store (was four 2-byte stores), and the
// MODE 2 residual arrives as one 8-byte LDS load. The V columns of MODE 1
// keep weight-as-B order: there the lane owns four consecutive m of one n,
// which is what is contiguous in vt[n][m..m+3].
template <int K, int MODE, int ACT, int WTS, int ABL, bool BIAS, bool SWAP>
static __device__ __forceinline__ void gemm_quad(
    const lds_short* __restrict__ in_lds, int in_stride,
    const glob_cshort* __restrict__ Wt, const glob_cfloat* __restrict__ bias,
    lds_short* __restrict__ out_lds, int out_stride,
    lds_short* __restrict__ x_lds, lds_short* __restrict__ vt_lds, int fn,
    int lane, bf16x8 zb) {
  static_assert(SWAP || MODE == 1, "only the V quads keep weight-as-B order");
  constexpr int KS = K / 32;
  const int l15 = lane & 15;
  const int l4 = lane >> 4;
  // bias up front: a bias load in the epilogue made the compiler wait
  // vmcnt(0) mid-GEMM, draining the weight-load pipeline with it. It seeds
  // the accumulators, which adds it in f32 at no instruction at all.
  f32x4 binit = {0.f, 0.f, 0.f, 0.f};
  if constexpr (BIAS) {
    if constexpr (SWAP) {
      binit = *(const __attribute__((address_space(1))) f32x4*)(bias + fn * 16 +
                                                               l4 * 4);
    } else {
      const float bval = bias[fn * 16 + l15];
      binit = {bval, bval, bval, bval};
    }
  }
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = binit;
#pragma unroll 4
  for (int ks = 0; ks < KS; ++ks) {
    bf16x8 w;
    if constexpr (ABL & 1) {
      w = zb;
    } else {
      w = *(const __attribute__((address_space(1))) bf16x8*)(
          Wt + (long)(fn * 16 + l15) * WTS + ks * 32 + l4 * 8);
    }
#pragma unroll
    for (int fm = 0; fm < 4; ++fm) {
      bf16x8 a;
      if constexpr (ABL & 2) {
        a = zb;
      } else {
        a = *(const __attribute__((address_space(3))) bf16x8*)(
            in_lds + (fm * 16 + l15) * in_stride + ks * 32 + l4 * 8);
      }
      if constexpr (SWAP)
        acc[fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, a, acc[fm], 0, 0, 0);
      else
        acc[fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w, acc[fm], 0, 0, 0);
    }
  }
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    f32x4 v = acc[fm];
    if constexpr (!SWAP) {
      // V transposed: vt[n][m0..m0+3]
      *(lds_short4*)(vt_lds + (fn * 16 + l15 - 2 * BF_H) * VTS + fm * 16 +
                     l4 * 4) = pack_bf16x4(v);
    } else if constexpr (MODE == 2) {
      lds_short4* px = (lds_short4*)(x_lds + (fm * 16 + l15) * XS + fn * 16 + l4 * 4);
      const short4v xv = *px;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(xv[r]);
      *px = pack_bf16x4(v);
    } else {
      if constexpr (ACT == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_f32(v[r]);
      }
      *(lds_short4*)(out_lds + (fm * 16 + l15) * out_stride + fn * 16 + l4 * 4) =
          pack_bf16x4(v);
    }
  }
}

// CNT consecutive quads from fn0, all in one operand order. unroll 2: the
// second quad's (independent) weight loads issue under the first quad's
// MFMA chains, hiding the L2 latency that dominated the per-quad cost
// (phase probe: GEMMs ~3.9 of 4.5 ms while pure MFMA issue accounts for
// <10% of that)
template <int K, int MODE, int ACT, int WTS, int ABL, bool BIAS, bool SWAP,
          int CNT>
static __device__ __forceinline__ void gemm_quads(
    const lds_short* __restrict__ in_lds, int in_stride,
    const glob_cshort* __restrict__ Wt, const glob_cfloat* __restrict__ bias,
    lds_short* __restrict__ out_lds, int out_stride,
    lds_short* __restrict__ x_lds, lds_short* __restrict__ vt_lds, int fn0,
    int lane, bf16x8 zb) {
#pragma unroll 2
  for (int q = 0; q < CNT; ++q)
    gemm_quad<K, MODE, ACT, WTS, ABL, BIAS, SWAP>(in_lds, in_stride, Wt, bias, out_lds,
                                            out_stride, x_lds, vt_lds, fn0 + q,
                                            lane, zb);
}

template <int K, int N, int MODE, int ACT, int WTS, int ABL = 0,
          bool BIAS = true>
static __device__ __attribute__((noinline)) void block_gemm(
    const lds_short* __restrict__ in_lds, int in_stride,
    const glob_cshort* __restrict__ Wt, const glob_cfloat* __restrict__ bias,
    lds_short* __restrict__ out_lds, int out_stride,
    lds_short* __restrict__ x_lds, lds_short* __restrict__ vt_lds, int wid,
    int lane) {
  bf16x8 zb;
  if constexpr (ABL != 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) zb[j] = (short)0x3f01;  // ~1.008 bf16
    asm volatile("" : "+v"(zb));  // opaque: keeps realistic data/clocks
  }
  constexpr int N16 = N / 16;
  constexpr int TOTAL = 4 * N16;
  constexpr int FPW = TOTAL / BF_WAVES;
  static_assert(FPW >= 4 && FPW % 4 == 0, "quad-chunked assignment");
  // quad-chunk: each iteration owns a FULL fn column (all 4 m-fragments):
  // ONE L2 weight-fragment load feeds FOUR independent MFMA chains.
  // wid is wave-uniform but arrives as a VGPR; as an SGPR the quad range,
  // the Q|K / V choice and the weight-row base are scalar work
  constexpr int QPW = FPW / 4;  // quads per wave
  const int fn_lo = __builtin_amdgcn_readfirstlane(wid) * QPW;
  if constexpr (MODE != 1) {
    gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, true, QPW>(in_lds, in_stride, Wt, bias,
                                                  out_lds, out_stride, x_lds,
                                                  vt_lds, fn_lo, lane, zb);
  } else {
    // qkv: fn below FN_SWAP (Q|K, row-major) runs operand-swapped, the V
    // columns in weight-as-B order. The choice is made ONCE per wave on a
    // scalar, outside the MFMA loops, and every arm has compile-time trip
    // counts (a per-quad `n < 2H` test compiled to a divergent exec-mask
    // ladder of ~200 scalar instructions around the MFMAs; runtime trip
    // counts lose the unroll-2 weight prefetch). With QPW = 3 wave 5 owns
    // fn 15 (K) and 16, 17 (V): the one mixed wave.
    constexpr int FN_SWAP = 2 * BF_H / 16;
    constexpr int NSW = FN_SWAP % QPW;  // swapped quads of the mixed wave
    if (fn_lo + QPW <= FN_SWAP) {
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, true, QPW>(in_lds, in_stride, Wt, bias,
                                                    out_lds, out_stride, x_lds,
                                                    vt_lds, fn_lo, lane, zb);
    } else if (fn_lo >= FN_SWAP) {
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, false, QPW>(in_lds, in_stride, Wt,
                                                     bias, out_lds, out_stride,
                                                     x_lds, vt_lds, fn_lo, lane,
                                                     zb);
    } else {
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, true, NSW>(in_lds, in_stride, Wt, bias,
                                                    out_lds, out_stride, x_lds,
                                                    vt_lds, fn_lo, lane, zb);
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, false, QPW - NSW>(
          in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds,
          fn_lo + NSW, lane, zb);
    }
  }
}

// ---- in-block LayerNorm on x (post-LN) -----------------------------------
// All 8 of the wave's rows in ONE parallel pass: 8 lanes per row, 16
// elements per lane, 3-step shfl_xor reduction within each 8-lane row
// group. (The serial per-row loop with full-wave reductions measured
// +1.12 ms of the 5.2 ms step — as costly as the whole QKV GEMM.)
static __device__ __forceinline__ void block_layernorm(
    lds_short* x_lds, const short* __restrict__ gamma,
    const short* __restrict__ beta, int wid, int lane, float eps) {
  const int row = wid * 8 + (lane >> 3);
  const int c0 = (lane & 7) * 16;
  short8v va = *(const __attribute__((address_space(3))) short8v*)(x_lds + row * XS + c0);
  short8v vb = *(const __attribute__((address_space(3))) short8v*)(x_lds + row * XS + c0 + 8);
  float v[16];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = bf16_to_f32(va[j]);
    v[8 + j] = bf16_to_f32(vb[j]);
    sum += v[j] + v[8 + j];
  }
#pragma unroll
  for (int mask = 1; mask < 8; mask <<= 1) sum += __shfl_xor(sum, mask, 64);
  const float mean = sum / BF_H;
  float var = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float d = v[j] - mean;
    var += d * d;
  }
#pragma unroll
  for (int mask = 1; mask < 8; mask <<= 1) var += __shfl_xor(var, mask, 64);
  const float rstd = rsqrtf(var / BF_H + eps);
  short8v ga = *(const short8v*)(gamma + c0);
  short8v gb = *(const short8v*)(gamma + c0 + 8);
  short8v ba = *(const short8v*)(beta + c0);
  short8v bb = *(const short8v*)(beta + c0 + 8);
  short8v oa, ob;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    oa[j] = f32_to_bf16((v[j] - mean) * rstd * bf16_to_f32(ga[j]) +
                        bf16_to_f32(ba[j]));
    ob[j] = f32_to_bf16((v[8 + j] - mean) * rstd * bf16_to_f32(gb[j]) +
                        bf16_to_f32(bb[j]));
  }
  *(__attribute__((address_space(3))) short8v*)(x_lds + row * XS + c0) = oa;
  *(__attribute__((address_space(3))) short8v*)(x_lds + row * XS + c0 + 8) = ob;
}

// Phase bits for the profiling probe (production uses PH_ALL; skipped
// phases cannot be dead-code-eliminated backwards because every phase
// ends in LDS stores).
#define PH_QKV 1
#define PH_ATTN 2
#define PH_PROJ 4
#define PH_LN 8
#define PH_FFN 16
#define PH_ALL 31

// Per-wave phase timing (diagnostic builds): stamps[k] = s_memrealtime at
// phase boundaries; slot pairs (work-done, barrier-crossed) separate each
// wave's compute time from its barrier wait. 100 MHz constant clock.
// BF_NSTAMP slots per wave (kernels.h).

template <int PHASES, bool TIMED = false, int ABL = 0>
static __device__ __forceinline__ void bert_fused_body(
    const unsigned char* __restrict__ lines,  // [B, max_len]
    const int* __restrict__ start,            // [B] content span start
    const int* __restrict__ end,              // [B] content span end
    const short* __restrict__ wb,             // bf16 weight blob
    const float* __restrict__ fb,             // f32 bias blob
    float* __restrict__ scores,               // [B]
    int B, int max_len, int n_layers, float eps,
    unsigned long long* __restrict__ stamps_out = nullptr) {
  unsigned long long tstamp[TIMED ? BF_NSTAMP : 1];
  int tidx = 0;
#define BF_STAMP()                                                          \
  if constexpr (TIMED) {                                                    \
    if (tidx < BF_NSTAMP) tstamp[tidx++] = __builtin_amdgcn_s_memrealtime(); \
  }
  const int line = blockIdx.x;
  if (line >= B) return;
  const int tid = threadIdx.x;
  const int wid = tid / DMX_WAVE;
  const int lane = tid % DMX_WAVE;

  extern __shared__ __attribute__((aligned(16))) short smem_raw[];
  lds_short* smem = (lds_short*)smem_raw;
  lds_short* x_lds = smem;             // [64][XS]
  lds_short* buf = x_lds + BF_S * XS;  // BUF_ELEMS: QK | P+O | FFN-half
  lds_short* vt = buf + BUF_ELEMS;     // [128][VTS]
  lds_float* red = (lds_float*)(vt + 2 * BF_DH * VTS);  // [128] pooling

  BF_STAMP();  // 0: kernel start
  // ---- embed: x[s][c] = tok_emb[byte+3 or 0][c] + pos_emb[s][c] ----
  {
    const int s0 = start[line], e0 = end[line];
    for (int i = tid * 8; i < BF_S * BF_H; i += BF_THREADS * 8) {
      const int s = i / BF_H, c = i % BF_H;
      int tok = 0;
      const int idx = s0 + s;
      if (idx < e0 && idx < max_len)
        tok = (int)lines[(long)line * max_len + idx] + 3;
      short8v te = *(const short8v*)(wb + WB_TOK + (long)tok * BF_H + c);
      short8v pe = *(const short8v*)(wb + WB_POS + (long)s * BF_H + c);
      short8v xv;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        xv[j] = f32_to_bf16(bf16_to_f32(te[j]) + bf16_to_f32(pe[j]));
      *(__attribute__((address_space(3))) short8v*)(x_lds + s * XS + c) = xv;
    }
  }
  BF_STAMP();  // 1: embed work done
  __syncthreads();
  BF_STAMP();  // 2: embed barrier crossed

  for (int layer = 0; layer < n_layers; ++layer) {
    const short* lw = wb + WB_LAYER0 + (long)layer * LW_SIZE;
    const float* lf = fb + (long)layer * FB_SIZE;

    // ---- qkv: Q|K -> buf[64][QKS], V -> vt transposed ----
    if (PHASES & PH_QKV)
      block_gemm<BF_H, 3 * BF_H, 1, 0, BF_H, ABL>(x_lds, XS, (glob_cshort*)(lw + LW_QKV),
                                             (glob_cfloat*)(lf + FB_BQKV), buf, QKS, x_lds, vt,
                                             wid, lane);
    BF_STAMP();  // qkv work done
    __syncthreads();
    BF_STAMP();  // qkv barrier crossed

    // ---- attention: wave = (head hh, 16 q-rows) ----
    // Both MFMAs run operand-swapped (see block_gemm): S^T = K Q^T puts
    // query q0 + (lane&15) and 16 keys (f*16 + (lane>>4)*4 + r) in each
    // lane, so a softmax row is 15 in-lane ops plus two cross-lane steps
    // (xor 16, 32) instead of four, every lane of a query ends up holding
    // that query's 1/sum, and P leaves as four 8-byte stores. O^T = V^T P^T
    // again gives the lane its own query and four consecutive d: scaled by
    // the in-lane 1/sum (no __shfl) and stored 8 bytes at a time.
    if (PHASES & PH_ATTN) {
      const int hh = wid >> 2;
      const int q0 = (wid & 3) * 16;
      const int l15 = lane & 15;
      const int l4 = lane >> 4;
      const float scale = 0.125f;  // 1/sqrt(64)

      f32x4 acc_p[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) acc_p[f] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < BF_DH / 32; ++ks) {
        bf16x8 qf = *(const __attribute__((address_space(3))) bf16x8*)(
            buf + (q0 + l15) * QKS + hh * BF_DH + ks * 32 + l4 * 8);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          bf16x8 kf = *(const __attribute__((address_space(3))) bf16x8*)(
              buf + (f * 16 + l15) * QKS + BF_H + hh * BF_DH + ks * 32 +
              l4 * 8);
          acc_p[f] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, acc_p[f], 0, 0, 0);
        }
      }
      float m = -1e30f;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, acc_p[f][r] * scale);
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      float sum = 0.f;
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __expf(acc_p[f][r] * scale - m);
          acc_p[f][r] = e;
          sum += e;
        }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      const float inv = 1.f / sum;
      // P tiles alias the Q|K area: every wave must be done reading Q/K
      __syncthreads();
      lds_short* my_p = buf + wid * 16 * VTS;
#pragma unroll
      for (int f = 0; f < 4; ++f)
        *(lds_short4*)(my_p + l15 * VTS + f * 16 + l4 * 4) =
            pack_bf16x4(acc_p[f]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-local P

      f32x4 acc_o[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) acc_o[f] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < BF_S / 32; ++ks) {
        bf16x8 pf = *(const __attribute__((address_space(3))) bf16x8*)(
            my_p + l15 * VTS + ks * 32 + l4 * 8);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          bf16x8 vf = *(const __attribute__((address_space(3))) bf16x8*)(
              vt + (hh * BF_DH + f * 16 + l15) * VTS + ks * 32 + l4 * 8);
          acc_o[f] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc_o[f], 0, 0, 0);
        }
      }
      // attn out -> buf[O_OFF + q*XS + hh*64 + d] (disjoint from P tiles)
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        f32x4 o = acc_o[f];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] *= inv;
        *(lds_short4*)(buf + O_OFF + (q0 + l15) * XS + hh * BF_DH + f * 16 +
                       l4 * 4) = pack_bf16x4(o);
      }
    }
    BF_STAMP();  // attention work done
    __syncthreads();
    BF_STAMP();  // attention barrier crossed

    // ---- proj: x += Wo(attn) ; LN1 ----
    if (PHASES & PH_PROJ)
      block_gemm<BF_H, BF_H, 2, 0, BF_H, ABL>(buf + O_OFF, XS, (glob_cshort*)(lw + LW_WO),
                                         (glob_cfloat*)(lf + FB_BO), nullptr, 0, x_lds,
                                         nullptr, wid, lane);
    __syncthreads();
    if (PHASES & PH_LN)
      block_layernorm(x_lds, lw + LW_LN1G, lw + LW_LN1B, wid, lane, eps);
    BF_STAMP();  // proj+LN1 work done
    __syncthreads();
    BF_STAMP();  // proj+LN1 barrier crossed

    // ---- FFN in two K=256 halves: buf = gelu(x@W1_h); x += buf@W2_h ----
    if (PHASES & PH_FFN)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      block_gemm<BF_H, BF_FFN / 2, 0, 1, BF_H, ABL>(
          x_lds, XS, (glob_cshort*)(lw + LW_W1 + (long)h * (BF_FFN / 2) * BF_H),
          (glob_cfloat*)(lf + FB_B1 + h * (BF_FFN / 2)), buf, QKS, nullptr,
          nullptr, wid, lane);
      __syncthreads();
      // bias b2 added once (half 0); half 1 adds only the partial product
      // (compile-time: a runtime null test on the pointer, a VGPR in the
      // noinline callee, put an exec-mask branch in front of every quad)
      if (h == 0)
        block_gemm<BF_FFN / 2, BF_H, 2, 0, BF_FFN, ABL, true>(
            buf, QKS, (glob_cshort*)(lw + LW_W2), (glob_cfloat*)(lf + FB_B2),
            nullptr, 0, x_lds, nullptr, wid, lane);
      else
        block_gemm<BF_FFN / 2, BF_H, 2, 0, BF_FFN, ABL, false>(
            buf, QKS, (glob_cshort*)(lw + LW_W2 + (long)h * (BF_FFN / 2)),
            nullptr, nullptr, 0, x_lds, nullptr, wid, lane);
      __syncthreads();
    }
    if (PHASES & PH_LN)
      block_layernorm(x_lds, lw + LW_LN2G, lw + LW_LN2B, wid, lane, eps);
    BF_STAMP();  // ffn+LN2 work done
    __syncthreads();
    BF_STAMP();  // ffn+LN2 barrier crossed
  }

  // ---- pool (mean over S) + score head ----
  {
    if (tid < BF_H) {
      float s = 0.f;
      for (int row = 0; row < BF_S; ++row)
        s += bf16_to_f32(x_lds[row * XS + tid]);
      const float w =
          bf16_to_f32(wb[WB_LAYER0 + (long)n_layers * LW_SIZE + tid]);
      red[tid] = (s / BF_S) * w;
    }
    __syncthreads();
    if (wid == 0) {
      float v = red[lane] + red[lane + 64];
      v = warp_reduce_sum_f32(v);
      if (lane == 0)
        scores[line] = v + fb[(long)n_layers * FB_SIZE];  // b_score
    }
  }
  BF_STAMP();  // final
  if constexpr (TIMED) {
    if (lane == 0 && stamps_out != nullptr) {
      unsigned long long* dst =
          stamps_out + ((long)line * BF_WAVES + wid) * BF_NSTAMP;
      for (int k = 0; k < BF_NSTAMP; ++k)
        dst[k] = k < tidx ? tstamp[k] : 0ull;
    }
  }
#undef BF_STAMP
}

extern "C" __global__ __launch_bounds__(BF_THREADS, 4)
void dmx_bert_fused_bf16(const unsigned char* __restrict__ lines,
                         const int* __restrict__ start,
                         const int* __restrict__ end,
                         const short* __restrict__ wb,
                         const float* __restrict__ fb,
                         float* __restrict__ scores, int B, int max_len,
                         int n_layers, float eps) {
  bert_fused_body<PH_ALL>(lines, start, end, wb, fb, scores, B, max_len,
                          n_layers, eps);
}

// probe variants (in-kernel phase ablation; guide §5.4 rule 19: co-compiled
// variants can perturb codegen by a few % — read the deltas, not absolutes)
template <int PHASES, int ABL = 0>
__global__ __launch_bounds__(BF_THREADS, 4) void dmx_bert_fused_probe(
    const unsigned char* lines, const int* start, const int* end,
    const short* wb, const float* fb, float* scores, int B, int max_len,
    int n_layers, float eps) {
  bert_fused_body<PHASES, false, ABL>(lines, start, end, wb, fb, scores, B,
                                      max_len, n_layers, eps);
}

extern "C" __global__ __launch_bounds__(BF_THREADS, 4)
void dmx_bert_fused_timed(const unsigned char* lines, const int* start,
                          const int* end, const short* wb, const float* fb,
                          float* scores, int B, int max_len, int n_layers,
                          float eps, unsigned long long* stamps) {
  bert_fused_body<PH_ALL, true>(lines, start, end, wb, fb, scores, B,
                                max_len, n_layers, eps, stamps);
}

// ---- host side -------------------------------------------------------------
// The one launch path of all three entry points. BF_LDS_BYTES is above the
// default dynamic-LDS limit, so each (kernel, device) pair needs the opt-in
// attribute once; `attr_done` is that kernel's per-device flag array, which
// keeps the attribute call off the production kernel's per-launch path
// (unsynchronised on purpose: a racing second call sets the same value).
constexpr int BF_MAX_DEVICES = 64;

template <typename... KArgs, typename... Args>
static hipError_t launch_bert_fused(void (*kernel)(KArgs...),
                                    bool (&attr_done)[BF_MAX_DEVICES], int B,
                                    hipStream_t stream, Args... args) {
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  if (dev < 0 || dev >= BF_MAX_DEVICES) return hipErrorInvalidDevice;
  if (!attr_done[dev]) {
    err = hipFuncSetAttribute((const void*)kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              BF_LDS_BYTES);
    if (err != hipSuccess) return err;
    attr_done[dev] = true;
  }
  hipLaunchKernelGGL(kernel, dim3(B), dim3(BF_THREADS), BF_LDS_BYTES, stream,
                     args...);
  return hipSuccess;  // launch errors surface through hipGetLastError()
}

extern "C" hipError_t dmx_launch_bert_fused_bf16(
    const uint8_t* lines, const int32_t* start, const int32_t* end,
    const int16_t* wb, const float* fb, float* scores, int B, int max_len,
    int n_layers, float eps, hipStream_t stream) {
  static bool attr_done[BF_MAX_DEVICES];
  return launch_bert_fused(dmx_bert_fused_bf16, attr_done, B, stream, lines,
                           start, end, wb, fb, scores, B, max_len, n_layers,
                           eps);
}

extern "C" hipError_t dmx_launch_bert_fused_timed(
    const uint8_t* lines, const int32_t* start, const int32_t* end,
    const int16_t* wb, const float* fb, float* scores, int64_t* stamps, int B,
    int max_len, int n_layers, float eps, hipStream_t stream) {
  static bool attr_done[BF_MAX_DEVICES];
  return launch_bert_fused(dmx_bert_fused_timed, attr_done, B, stream, lines,
                           start, end, wb, fb, scores, B, max_len, n_layers,
                           eps, (unsigned long long*)stamps);
}

// Compiled probe variants as X(phases, ablation); phase_mask = PH | AB << 8.
#define BF_PROBE_VARIANTS(X)                                                 \
  X(0, 0)                                                                    \
  X(PH_QKV, 0)                                                               \
  X(PH_QKV | PH_ATTN, 0)                                                     \
  X(PH_QKV | PH_ATTN | PH_PROJ, 0)                                           \
  X(PH_QKV | PH_ATTN | PH_PROJ | PH_LN, 0)                                   \
  X(PH_ALL, 0)                                                               \
  X(PH_FFN, 0)                                                               \
  X(PH_LN, 0)                                                                \
  /* perf-ablation variants (numerically wrong by design): */                \
  X(PH_ALL, 1) /* B operand constant (no L2 weight loads) */                 \
  X(PH_ALL, 2) /* A operand constant (no LDS activation reads) */            \
  X(PH_ALL, 3) /* both constant (pure MFMA + epilogue) */                    \
  X(PH_FFN, 1)                                                               \
  X(PH_FFN, 2)                                                               \
  X(PH_FFN, 3)

extern "C" bool dmx_bert_fused_probe_mask_known(int phase_mask) {
  switch (phase_mask) {
#define KNOWN(PH, AB) case ((PH) | ((AB) << 8)):
    BF_PROBE_VARIANTS(KNOWN)
#undef KNOWN
    return true;
    default:
      return false;
  }
}

extern "C" hipError_t dmx_launch_bert_fused_probe(
    const uint8_t* lines, const int32_t* start, const int32_t* end,
    const int16_t* wb, const float* fb, float* scores, int B, int max_len,
    int n_layers, float eps, int phase_mask, hipStream_t stream) {
  switch (phase_mask) {
#define LAUNCH_PROBE(PH, AB)                                                 \
  case ((PH) | ((AB) << 8)): {                                               \
    static bool attr_done[BF_MAX_DEVICES];                                   \
    return launch_bert_fused(dmx_bert_fused_probe<PH, AB>, attr_done, B,     \
                             stream, lines, start, end, wb, fb, scores, B,   \
                             max_len, n_layers, eps);                        \
  }
    BF_PROBE_VARIANTS(LAUNCH_PROBE)
#undef LAUNCH_PROBE
    default:
      return hipErrorInvalidValue;
  }
}
