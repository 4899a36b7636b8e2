// Fused whole-model BERT-tiny forward: ONE workgroup per log line.
//
// The flagship detector config (BASELINE.json config 5) is tiny enough
// that the idiomatic MI355X mapping is a per-line megakernel: all
// activations for one line live in LDS for the whole forward pass; the
// model's weights (~600 KB) are read through the XCD L2s and shared by
// every workgroup; HBM traffic is line bytes in + one f32 score out.
//
// Geometry (kernels.h, checked by the bindings): S=64 tokens, H=128,
// 2 heads (Dh=64), FFN=512, any layer count. 8 waves x 64 lanes.
//
// Two blocks per CU. The phases are bulk-synchronous, so a lone block
// leaves its CU idle at every barrier; with a ~70 KiB arena and <= 128
// VGPRs two blocks co-reside (4 waves/SIMD from two independent barrier
// domains) and one block's barrier wait overlaps the other's compute.
//
// Arena (the Tile aliases below): x | buf | vt, bf16, then [H] f32 for
// pooling. vt holds V^T through attention and x + the first FFN half
// between the two W2 GEMMs. `buf` has three tenants in turn: Q|K; then the
// per-wave P tiles followed by the attention output; then one FFN half. V
// never enters buf:
// the qkv GEMM writes it transposed into vt, k-contiguous for the P.V MFMA.
//
// Schedule (bert_fused_body; every `|` is a block barrier):
//   embed | per layer: qkv | attention (one barrier inside, before the P
//   tiles overwrite Q|K) | x += Wo | LN1 | 2 x (W1 half + GELU | x += W2
//   half |) LN2 | pool | score. Both W1 halves read the LN1 output: the first
//   W2 half writes x + its update to XMid, not over x, and the second adds
//   its update to XMid and writes x. dmx_bert_fused_embed_bf16 runs the same
//   schedule and ends in pool_embed instead: the pooled vector and / or its
//   distance from a fitted diagonal Gaussian.
//
// Operand feed (profiles/r19_operand_pipeline.txt). The kernel is bound by
// operand latency, not by MFMA, L2 or LDS throughput, so the GEMMs make the
// weight stream explicit: a quad's K/32 weight fragments and its bias are
// all issued before its first MFMA (quad_operands) and the chain steps down
// through counted vmcnt waits; the next quad's are issued between the K
// chain and the epilogue; and the barrier in front of every GEMM is executed
// inside block_gemm, after the first quad's loads have been issued, so they
// are in flight while the wave waits for the block (a `|` below directly in
// front of a GEMM is that barrier). The A side stays as the compiler
// schedules it: double-buffering the ds_read_b128 by K step was built and
// measured no gain on top of this.
//
// Operand order. The 16x16x32 bf16 A and B fragment layouts are the same
// function of the lane (row or column lane&15, k (lane>>4)*8..+7), so
// mfma(weight, activation) yields the transposed tile of mfma(activation,
// weight): the lane then owns ONE row m = fm*16 + (lane&15) and FOUR
// CONSECUTIVE columns n = fn*16 + (lane>>4)*4 + r. Everything stored
// row-major runs weight-first: the four results leave as one 8-byte LDS
// store, a residual arrives as one 8-byte load, the bias as one 16-byte
// load. Only V keeps activation-first order: there the lane owns four
// consecutive m of one n, which is what is contiguous in vt[n][m..m+3].
// Attention does the same with S^T = K Q^T and O^T = V^T P^T.
//
// The adjacent values invite v_pk_mul_f32 / v_pk_add_f32 in the epilogues,
// an anti-lever beside MFMAs. The compiler's pairing is left alone: keeping
// them apart needs inline-asm arithmetic, which steps outside the
// compiler's hazard handling (a v_rcp_f32 result read too early) and
// computed garbage.
#include "common.h"
#include "kernels.h"  // geometry, blob offsets, BF_LDS_BYTES, launchers

// Explicit address-space typing: a generic (flat) short* makes hipcc emit
// flat_load for what are really LDS reads. AS(3) pointers guarantee ds_*
// lowering.
typedef __attribute__((address_space(3))) short lds_short;
typedef __attribute__((address_space(3))) short4v lds_short4;
typedef __attribute__((address_space(3))) float lds_float;
typedef __attribute__((address_space(1))) const short glob_cshort;
typedef __attribute__((address_space(1))) const float glob_cfloat;

#define BF_THREADS (BF_WAVES * DMX_WAVE)

// LDS strides (elements); +8 pads keep rows 16-B aligned and bank-spread
#define XS (BF_H + 8)  // 136, x and attention-output rows
// QKS at +16 (not +8): stride 136 dw = 8 mod 64 makes the W2 / attention
// A-fragment ds_read_b128 groups conflict-free. Both tenants still fit in
// buf (asserted below), so it costs no LDS.
#define QKS (2 * BF_H + 16)  // 272, Q|K rows and FFN-half rows
#define VTS (BF_S + 8)       // 72, transposed-V and P rows

// ---- LDS arena --------------------------------------------------------------
extern __shared__ __attribute__((aligned(16))) short smem_raw[];

// A [ROWS][COLS] bf16 tenant of the arena: OFF elements from its base, rows
// STRIDE apart.
template <int OFF_, int ROWS, int COLS_, int STRIDE_>
struct Tile {
  static constexpr int OFF = OFF_, COLS = COLS_, STRIDE = STRIDE_;
  static constexpr int END = OFF + ROWS * STRIDE;
  // The GEMM and attention epilogues move four bf16 per lane with one
  // 8-byte LDS access at column offsets that are multiples of 4.
  static_assert(OFF % 4 == 0 && STRIDE % 4 == 0 && COLS <= STRIDE,
                "8-byte LDS access: offsets and strides are multiples of 4");
  static __device__ __forceinline__ lds_short* ptr() {
    return (lds_short*)smem_raw + OFF;
  }
};
using XTile = Tile<0, BF_S, BF_H, XS>;
// buf, first tenant
using QkTile = Tile<XTile::END, BF_S, 2 * BF_H, QKS>;
// buf, second tenants: wave w owns P rows 16w .. 16w+15
using PTiles = Tile<XTile::END, BF_WAVES * 16, BF_S, VTS>;
using AttnOut = Tile<PTiles::END, BF_S, BF_H, XS>;
// buf, third tenant
using FfnHalf = Tile<XTile::END, BF_S, BF_FFN / 2, QKS>;
using VtTile = Tile<AttnOut::END, 2 * BF_DH, BF_S, VTS>;  // after buf
// vt, second tenant (V^T is dead once attention is done): x + W2 half 0,
// while x itself still feeds the W1 GEMM of half 1
using XMid = Tile<VtTile::OFF, BF_S, BF_H, XS>;
constexpr int RED_OFF = VtTile::END;                      // [H] f32 pooling

static_assert(QkTile::END <= VtTile::OFF, "Q|K runs past buf");
static_assert(FfnHalf::END <= VtTile::OFF, "the FFN half runs past buf");
static_assert(PTiles::END <= AttnOut::OFF,
              "the P tiles reach into the attention output");
static_assert(AttnOut::END <= VtTile::OFF,
              "the attention output runs past buf");
static_assert(XMid::END <= VtTile::END, "XMid runs past vt");
static_assert(BF_LDS_BYTES == RED_OFF * sizeof(short) + BF_H * sizeof(float),
              "kernels.h BF_LDS_BYTES out of step with the LDS strides");
// The weight-first GEMMs fetch four biases with one 16-byte load: every
// bias vector must start a multiple of 4 floats into the (16-byte aligned,
// checked by the bindings) blob.
static_assert(FB_BQKV % 4 == 0 && FB_BO % 4 == 0 && FB_B1 % 4 == 0 &&
                  FB_B2 % 4 == 0 && FB_SIZE % 4 == 0 &&
                  (BF_FFN / 2) % 4 == 0,
              "16-byte bias loads: bias offsets must be multiples of 4");

// ---- MFMA fragment addressing in LDS --------------------------------------
// A lane's place in every 16x16 fragment: l15 = lane&15, l4 = lane>>4. Each
// phase splits the lane once and hands the pair to the helpers below.
struct FragLane {
  int l15, l4;
  __device__ __forceinline__ explicit FragLane(int lane)
      : l15(lane & 15), l4(lane >> 4) {}
};

// 16x16x32 bf16 operand fragment (A and B alike) whose first row is r0 and
// first k is k0: the lane reads row r0 + l15, k0 + l4*8 .. +7, one
// ds_read_b128.
static __device__ __forceinline__ bf16x8 lds_frag(const lds_short* base,
                                                  int stride, int r0, int k0,
                                                  FragLane fl) {
  return *(const __attribute__((address_space(3))) bf16x8*)(
      base + (r0 + fl.l15) * stride + k0 + fl.l4 * 8);
}

// The four consecutive elements a lane owns of the 16x16 accumulator tile at
// (r0, c0): row r0 + l15, columns c0 + l4*4 .. +3, one 8-byte LDS access
// either way.
static __device__ __forceinline__ lds_short4* lds_quad(lds_short* base,
                                                       int stride, int r0,
                                                       int c0, FragLane fl) {
  return (lds_short4*)(base + (r0 + fl.l15) * stride + c0 + fl.l4 * 4);
}

// four f32 -> four bf16 (RNE, as f32_to_bf16) as two v_cvt_pk_bf16_f32;
// element-wise f32_to_bf16 left the compiler re-pairing halves with
// v_perm_b32 / v_alignbit_b32
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
static __device__ __forceinline__ short4v pack_bf16x4(f32x4 v) {
  return __builtin_bit_cast(short4v, __builtin_convertvector(v, bf16x4_t));
}

// ---- in-block GEMM: out = act(in_lds[64][K] @ Wt[N][WTS] + bias) ---------
// MODE 0: write out_lds[m][n]; MODE 1 (qkv): n<2H -> out (Q|K), else vt
// transposed; MODE 2: x[m][n] += v (residual-accumulate); MODE 3:
// out[m][n] = x[m][n] + v, rows XS apart (residual-accumulate into another
// tile, x left as it is). ACT 1 = GELU.
// ABL (perf-ablation diagnostics, numerically wrong on purpose):
// bit 1 = B operand from an opaque register instead of the L2 weight
// load (removes vmcnt parks); bit 2 = A operand from a register instead
// of the LDS read (removes lgkmcnt parks). Epilogue stores stay, so the
// MFMA chains cannot be dead-code-eliminated.
// All pointers __restrict__: the pointers arrive as opaque noinline
// arguments, and without it the epilogue's LDS stores between quads alias
// the activation reads for the analyzer, which then re-reads every A
// fragment per quad and cannot hoist reads across the quad boundary. The
// caller guarantees in_lds never overlaps this GEMM's outputs.
//
// SWAP is the weight-first operand order of the file header: MODE 0, MODE 2,
// MODE 3 and the Q|K columns of MODE 1 run swapped, the V columns of MODE 1
// do not.
//
// The three functions below keep one scalar argument list and spell their
// fragment addresses out instead of using lds_frag / lds_quad. Every call
// passes the same LDS addresses and strides, the compiler folds them into
// each block_gemm instance, and the code it then generates depends on how
// they arrive: bundled into by-value structs, turned into compile-time
// tiles, or merely read through lds_frag, the qkv GEMM comes out between
// 719 and 806 instructions instead of 741 and spills up to 13 more
// registers (profiles/r15_fused_refactor_isa.txt).
// One quad is three steps, so that gemm_quads can place the next quad's
// loads between this quad's K chain and its epilogue.
//
// quad_operands: every weight fragment of quad fn (K/32 global_load_dwordx4,
// 4 VGPRs each) and its bias, all issued back to back. Nothing here touches
// LDS, so it may run ahead of the barrier that guards in_lds.
template <int K, int WTS, int ABL, bool BIAS, bool SWAP>
static __device__ __forceinline__ void quad_operands(
    const glob_cshort* __restrict__ Wt, const glob_cfloat* __restrict__ bias,
    int fn, int l15, int l4, bf16x8 zb, bf16x8 (&w)[K / 32], f32x4& binit) {
  // bias up front: a bias load in the epilogue made the compiler wait
  // vmcnt(0) mid-GEMM, draining the weight-load pipeline with it. It seeds
  // the accumulators, which adds it in f32 at no instruction at all.
  binit = {0.f, 0.f, 0.f, 0.f};
  if constexpr (BIAS) {
    if constexpr (SWAP) {
      binit = *(const __attribute__((address_space(1))) f32x4*)(bias + fn * 16 +
                                                               l4 * 4);
    } else {
      const float bval = bias[fn * 16 + l15];
      binit = {bval, bval, bval, bval};
    }
  }
#pragma unroll
  for (int ks = 0; ks < K / 32; ++ks) {
    if constexpr (ABL & 1) {
      w[ks] = zb;
    } else {
      w[ks] = *(const __attribute__((address_space(1))) bf16x8*)(
          Wt + (long)(fn * 16 + l15) * WTS + ks * 32 + l4 * 8);
    }
  }
  // Left alone, the scheduler sinks each load to just before the MFMA that
  // needs it and the chain waits a full L2 round trip per K step.
  __builtin_amdgcn_sched_barrier(0);
}

// quad_chain: the four K chains of a quad, ascending k, each accumulator
// seeded by the caller. The A-fragment reads are left to the compiler's
// scheduler (an explicit K-step double buffer, 32 VGPRs, measured no gain).
template <int K, int ABL, bool SWAP>
static __device__ __forceinline__ void quad_chain(
    const lds_short* __restrict__ in_lds, int in_stride, int l15, int l4,
    bf16x8 zb, const bf16x8 (&w)[K / 32], f32x4 (&acc)[4]) {
  constexpr int KS = K / 32;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
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
        acc[fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[ks], a, acc[fm], 0, 0, 0);
      else
        acc[fm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, w[ks], acc[fm], 0, 0, 0);
    }
  }
}

// quad_store: the epilogue of quad fn.
template <int MODE, int ACT, bool SWAP>
static __device__ __forceinline__ void quad_store(
    lds_short* __restrict__ out_lds, int out_stride,
    lds_short* __restrict__ x_lds, lds_short* __restrict__ vt_lds, int fn,
    int l15, int l4, const f32x4 (&acc)[4]) {
  static_assert(SWAP || MODE == 1, "only the V quads keep weight-as-B order");
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
    } else if constexpr (MODE == 3) {
      const int off = (fm * 16 + l15) * XS + fn * 16 + l4 * 4;
      const short4v xv = *(const lds_short4*)(x_lds + off);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(xv[r]);
      *(lds_short4*)(out_lds + off) = pack_bf16x4(v);
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

// CNT consecutive quads from fn0, all in one operand order. One quad body
// at a time: all of a quad's weight fragments are in flight before its
// first MFMA, and the next quad's are issued between this quad's K chain
// and its epilogue, into the registers the chain has just freed, so their
// L2 latency runs under the epilogue.
//
// BAR: this call executes the block barrier that guards in_lds (block_gemm).
// The first quad's loads are in flight when the wave arrives at it, so the
// phase no longer opens with a bare L2 round trip on all eight waves. Each
// recorder in `rec` (none, or the timed variant's) stamps "barrier crossed".
template <int K, int MODE, int ACT, int WTS, int ABL, bool BIAS, bool SWAP,
          int CNT, bool BAR, typename... REC>
static __device__ __forceinline__ void gemm_quads(
    const lds_short* __restrict__ in_lds, int in_stride,
    const glob_cshort* __restrict__ Wt, const glob_cfloat* __restrict__ bias,
    lds_short* __restrict__ out_lds, int out_stride,
    lds_short* __restrict__ x_lds, lds_short* __restrict__ vt_lds, int fn0,
    int lane, bf16x8 zb, REC&... rec) {
  const int l15 = lane & 15;
  const int l4 = lane >> 4;
  bf16x8 w[K / 32];
  f32x4 binit;
  quad_operands<K, WTS, ABL, BIAS, SWAP>(Wt, bias, fn0, l15, l4, zb, w, binit);
  // The timed variant reads the clock right behind the barrier and waits
  // for it there (an outstanding scalar load turns every counted lgkmcnt wait
  // of the chain into lgkmcnt(0)), but files the stamp after the last quad:
  // the recorder lives in scratch, and a store in here would sit on vmcnt.
  unsigned long long crossed = 0;
  if constexpr (BAR) {
    // lowers to s_waitcnt lgkmcnt(0); s_barrier: the loads stay in flight
    __syncthreads();
    if constexpr (sizeof...(REC) != 0) {
      crossed = __builtin_amdgcn_s_memrealtime();
      asm volatile("" : "+s"(crossed));
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int q = 0; q < CNT; ++q) {
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = binit;
    quad_chain<K, ABL, SWAP>(in_lds, in_stride, l15, l4, zb, w, acc);
    if (q + 1 < CNT)
      quad_operands<K, WTS, ABL, BIAS, SWAP>(Wt, bias, fn0 + q + 1, l15, l4,
                                             zb, w, binit);
    quad_store<MODE, ACT, SWAP>(out_lds, out_stride, x_lds, vt_lds, fn0 + q,
                                l15, l4, acc);
  }
  if constexpr (BAR) (rec.mark_at(crossed), ...);
}

// BAR: the block barrier that precedes this GEMM is executed inside it,
// after the wave's first weight and bias loads have been issued and before
// anything touches in_lds; the caller then leaves its own __syncthreads()
// out. Every wave executes exactly one barrier on every path.
template <int K, int N, int MODE, int ACT, int WTS, int ABL = 0,
          bool BIAS = true, bool BAR = false, typename... REC>
static __device__ __attribute__((noinline)) void block_gemm(
    const lds_short* __restrict__ in_lds, int in_stride,
    const glob_cshort* __restrict__ Wt, const glob_cfloat* __restrict__ bias,
    lds_short* __restrict__ out_lds, int out_stride,
    lds_short* __restrict__ x_lds, lds_short* __restrict__ vt_lds, int wid,
    int lane, REC&... rec) {
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
    gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, true, QPW, BAR>(
        in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds, fn_lo,
        lane, zb, rec...);
  } else {
    // qkv: fn below FN_SWAP (Q|K, row-major) runs operand-swapped, the V
    // columns in weight-as-B order. The choice is made ONCE per wave on a
    // scalar, outside the MFMA loops, and every arm has compile-time trip
    // counts (a per-quad `n < 2H` test compiled to a divergent exec-mask
    // ladder of ~200 scalar instructions around the MFMAs). With QPW = 3
    // wave 5 owns fn 15 (K) and 16, 17 (V): the one mixed wave. Its second
    // run of quads starts without a prefetch under the first run's epilogue:
    // the shallower schedule, on one wave of eight.
    constexpr int FN_SWAP = 2 * BF_H / 16;
    constexpr int NSW = FN_SWAP % QPW;  // swapped quads of the mixed wave
    if (fn_lo + QPW <= FN_SWAP) {
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, true, QPW, BAR>(
          in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds,
          fn_lo, lane, zb, rec...);
    } else if (fn_lo >= FN_SWAP) {
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, false, QPW, BAR>(
          in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds,
          fn_lo, lane, zb, rec...);
    } else {
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, true, NSW, BAR>(
          in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds,
          fn_lo, lane, zb, rec...);
      gemm_quads<K, MODE, ACT, WTS, ABL, BIAS, false, QPW - NSW, false>(
          in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds,
          fn_lo + NSW, lane, zb);
    }
  }
}

// ---- embed: x[s][c] = tok_emb[byte+3 or 0][c] + pos_emb[s][c] -------------
static __device__ __forceinline__ void embed(
    const unsigned char* __restrict__ lines, const int* __restrict__ start,
    const int* __restrict__ end, const short* __restrict__ wb, lds_short* x_lds,
    int line, int max_len, int tid) {
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

// ---- attention: wave = (head hh, 16 q-rows) -------------------------------
// Both MFMAs run weight-first (file header): S^T = K Q^T puts query
// q0 + (lane&15) and 16 keys (f*16 + (lane>>4)*4 + r) in each lane, so a
// softmax row is 15 in-lane ops plus two cross-lane steps (xor 16, 32),
// every lane of a query ends up holding that query's 1/sum, and P leaves as
// four 8-byte stores. O^T = V^T P^T again gives the lane its own query and
// four consecutive d: scaled by the in-lane 1/sum (no __shfl) and stored
// 8 bytes at a time.
static __device__ __forceinline__ void attention(int wid, int lane) {
  const FragLane fl(lane);
  const int hh = wid >> 2;
  const int q0 = (wid & 3) * 16;
  const float scale = 0.125f;  // 1/sqrt(64)

  f32x4 acc_p[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc_p[f] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < BF_DH / 32; ++ks) {
    bf16x8 qf = lds_frag(QkTile::ptr(), QKS, q0, hh * BF_DH + ks * 32, fl);
#pragma unroll
    for (int f = 0; f < 4; ++f)
      acc_p[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          lds_frag(QkTile::ptr(), QKS, f * 16, BF_H + hh * BF_DH + ks * 32, fl),
          qf, acc_p[f], 0, 0, 0);
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
  lds_short* my_p = PTiles::ptr() + wid * 16 * VTS;
#pragma unroll
  for (int f = 0; f < 4; ++f)
    *lds_quad(my_p, VTS, 0, f * 16, fl) = pack_bf16x4(acc_p[f]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-local P

  f32x4 acc_o[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) acc_o[f] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < BF_S / 32; ++ks) {
    bf16x8 pf = lds_frag(my_p, VTS, 0, ks * 32, fl);
#pragma unroll
    for (int f = 0; f < 4; ++f)
      acc_o[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          lds_frag(VtTile::ptr(), VTS, hh * BF_DH + f * 16, ks * 32, fl), pf,
          acc_o[f], 0, 0, 0);
  }
  // out[q][hh*64 + d], disjoint from the P tiles (asserted at the tiles)
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    f32x4 o = acc_o[f];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] *= inv;
    *lds_quad(AttnOut::ptr(), XS, q0, hh * BF_DH + f * 16, fl) = pack_bf16x4(o);
  }
}

// ---- in-block LayerNorm on x (post-LN) -----------------------------------
// All 8 of the wave's rows in ONE parallel pass: 8 lanes per row, 16
// elements per lane, 3-step shfl_xor reduction within each 8-lane row
// group (a serial per-row loop with full-wave reductions costs as much as
// the whole qkv GEMM).
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

// ---- pool (mean over S) + score head --------------------------------------
static __device__ __forceinline__ void pool_score(
    const short* __restrict__ w_score, const float* __restrict__ b_score,
    float* __restrict__ score, int tid) {
  const lds_short* x_lds = XTile::ptr();
  lds_float* red = (lds_float*)((lds_short*)smem_raw + RED_OFF);
  if (tid < BF_H) {
    float s = 0.f;
    for (int row = 0; row < BF_S; ++row)
      s += bf16_to_f32(x_lds[row * XS + tid]);
    red[tid] = (s / BF_S) * bf16_to_f32(w_score[tid]);
  }
  __syncthreads();
  const int wid = tid / DMX_WAVE, lane = tid % DMX_WAVE;
  if (wid == 0) {
    float v = red[lane] + red[lane + 64];
    v = warp_reduce_sum_f32(v);
    if (lane == 0) *score = v + *b_score;
  }
}

// ---- pool (mean over S) + embedding / distance head ------------------------
// The tail of dmx_bert_fused_embed_bf16: the pooled vector itself (emb, one
// coalesced 512-byte row per block) and / or its normalised distance from a
// fitted diagonal Gaussian, dist = sqrt(mean_c((m_c - mu_c)^2 * inv_var_c)).
// emb and mu are kernel arguments, so both null tests are scalar branches;
// inv_var and dist are read only when mu is given.
static __device__ __forceinline__ void pool_embed(
    float* __restrict__ emb, const float* __restrict__ mu,
    const float* __restrict__ inv_var, float* __restrict__ dist, int line,
    int tid) {
  const lds_short* x_lds = XTile::ptr();
  lds_float* red = (lds_float*)((lds_short*)smem_raw + RED_OFF);
  if (tid < BF_H) {
    float s = 0.f;
    for (int row = 0; row < BF_S; ++row)
      s += bf16_to_f32(x_lds[row * XS + tid]);
    const float m = s / BF_S;
    if (emb != nullptr) emb[(long)line * BF_H + tid] = m;
    if (mu != nullptr) {
      const float d = m - mu[tid];
      red[tid] = d * d * inv_var[tid];
    }
  }
  if (mu == nullptr) return;
  __syncthreads();
  const int wid = tid / DMX_WAVE, lane = tid % DMX_WAVE;
  if (wid == 0) {
    float v = red[lane] + red[lane + 64];
    v = warp_reduce_sum_f32(v);
    if (lane == 0) dist[line] = sqrtf(v / BF_H);
  }
}

// The tail phase of bert_fused_body: the score head of the production, probe
// and timed kernels, or the embedding / distance head.
#define HEAD_SCORE 0
#define HEAD_EMBED 1

// Phase bits for the profiling probe (production uses PH_ALL; skipped
// phases cannot be dead-code-eliminated backwards because every phase
// ends in LDS stores).
#define PH_QKV 1
#define PH_ATTN 2
#define PH_PROJ 4
#define PH_LN 8
#define PH_FFN 16
#define PH_ALL 31

// Per-wave phase timing (diagnostic builds): mark() stores s_memrealtime
// (100 MHz constant clock) at each phase boundary; slot pairs (work-done,
// barrier-crossed) separate a wave's compute time from its barrier wait.
// BF_NSTAMP slots per wave (kernels.h); unused ones are flushed as 0.
// Empty, and free, when not TIMED.
template <bool TIMED>
struct StampRecorder {
  __device__ void mark() {}
  __device__ void flush(unsigned long long*, int, int, int) {}
};
template <>
struct StampRecorder<true> {
  unsigned long long t[BF_NSTAMP];
  int n = 0;
  __device__ void mark() { mark_at(__builtin_amdgcn_s_memrealtime()); }
  // a clock value read earlier; slots are still filed in schedule order
  __device__ void mark_at(unsigned long long now) {
    if (n < BF_NSTAMP) t[n++] = now;
  }
  // out: [B, BF_WAVES, BF_NSTAMP]
  __device__ void flush(unsigned long long* out, int line, int wid, int lane) {
    if (lane == 0 && out != nullptr) {
      unsigned long long* dst = out + ((long)line * BF_WAVES + wid) * BF_NSTAMP;
      for (int k = 0; k < BF_NSTAMP; ++k) dst[k] = k < n ? t[k] : 0ull;
    }
  }
};

// A block_gemm that executes the barrier in front of it (BAR). Where that
// barrier carries a "barrier crossed" stamp the timed variant hands its
// recorder in; every other kernel calls the recorder-free instance, so the
// production kernel and the timed one run the same GEMM code but for the
// stamp. STAMPED is false for the barriers inside the FFN, which have no
// stamp slots.
template <int K, int N, int MODE, int ACT, int WTS, int ABL, bool BIAS,
          bool STAMPED, bool TIMED>
static __device__ __forceinline__ void block_gemm_bar(
    const lds_short* __restrict__ in_lds, int in_stride,
    const glob_cshort* __restrict__ Wt, const glob_cfloat* __restrict__ bias,
    lds_short* __restrict__ out_lds, int out_stride,
    lds_short* __restrict__ x_lds, lds_short* __restrict__ vt_lds, int wid,
    int lane, StampRecorder<TIMED>& stamp) {
  if constexpr (STAMPED && TIMED)
    block_gemm<K, N, MODE, ACT, WTS, ABL, BIAS, true>(
        in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds, wid,
        lane, stamp);
  else
    block_gemm<K, N, MODE, ACT, WTS, ABL, BIAS, true>(
        in_lds, in_stride, Wt, bias, out_lds, out_stride, x_lds, vt_lds, wid,
        lane);
}

// The schedule: phase, stamp, barrier, stamp. The barrier in front of a GEMM
// is executed inside it (block_gemm BAR), together with its "barrier
// crossed" stamp; where a probe variant leaves the GEMM out, the barrier and
// the stamp stand in its place. Stamp slots: 0 kernel start, 1-2 embed, then
// per layer (work done, barrier crossed) for qkv, attention, proj+LN1 and
// ffn+LN2, and one final stamp. HEAD picks the tail phase; with HEAD_EMBED
// `scores` is unused, with HEAD_SCORE the four arguments after `stamps_out`
// are.
template <int PHASES, bool TIMED = false, int ABL = 0, int HEAD = HEAD_SCORE>
static __device__ __forceinline__ void bert_fused_body(
    const unsigned char* __restrict__ lines,  // [B, max_len]
    const int* __restrict__ start,            // [B] content span start
    const int* __restrict__ end,              // [B] content span end
    const short* __restrict__ wb,             // bf16 weight blob
    const float* __restrict__ fb,             // f32 bias blob
    float* __restrict__ scores,               // [B]
    int B, int max_len, int n_layers, float eps,
    unsigned long long* __restrict__ stamps_out = nullptr,
    float* __restrict__ emb = nullptr,            // [B, H] or null
    const float* __restrict__ mu = nullptr,       // [H] or null
    const float* __restrict__ inv_var = nullptr,  // [H], read when mu given
    float* __restrict__ dist = nullptr) {         // [B], written when mu given
  StampRecorder<TIMED> stamp;
  const int line = blockIdx.x;
  if (line >= B) return;
  const int tid = threadIdx.x;
  const int wid = tid / DMX_WAVE;
  const int lane = tid % DMX_WAVE;

  lds_short* const x = XTile::ptr();

  stamp.mark();
  embed(lines, start, end, wb, x, line, max_len, tid);
  stamp.mark();

  for (int layer = 0; layer < n_layers; ++layer) {
    const short* lw = wb + WB_LAYER0 + (long)layer * LW_SIZE;
    const float* lf = fb + (long)layer * FB_SIZE;

    // opens with the barrier that ends embed or the previous layer's LN2
    if (PHASES & PH_QKV) {
      block_gemm_bar<BF_H, 3 * BF_H, 1, 0, BF_H, ABL, true, true, TIMED>(
          x, XS, (glob_cshort*)(lw + LW_QKV), (glob_cfloat*)(lf + FB_BQKV),
          QkTile::ptr(), QKS, x, VtTile::ptr(), wid, lane, stamp);
    } else {
      __syncthreads();
      stamp.mark();
    }
    stamp.mark();
    __syncthreads();
    stamp.mark();

    if (PHASES & PH_ATTN) attention(wid, lane);
    stamp.mark();

    // | x += Wo(attn) | LN1
    if (PHASES & PH_PROJ) {
      block_gemm_bar<BF_H, BF_H, 2, 0, BF_H, ABL, true, true, TIMED>(
          AttnOut::ptr(), XS, (glob_cshort*)(lw + LW_WO),
          (glob_cfloat*)(lf + FB_BO), nullptr, 0, x, nullptr, wid, lane, stamp);
    } else {
      __syncthreads();
      stamp.mark();
    }
    __syncthreads();
    if (PHASES & PH_LN)
      block_layernorm(x, lw + LW_LN1G, lw + LW_LN1B, wid, lane, eps);
    stamp.mark();

    // FFN in two K=256 halves, both reading the LN1 output in x:
    // | buf = gelu(x @ W1_0) | XMid = x + buf @ W2_0 + b2
    // | buf = gelu(x @ W1_1) | x = XMid + buf @ W2_1 | LN2
    // The first of the five barriers is the one after LN1 and has the stamp.
    if (PHASES & PH_FFN) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const glob_cshort* w1 =
            (glob_cshort*)(lw + LW_W1 + (long)h * (BF_FFN / 2) * BF_H);
        const glob_cfloat* b1 = (glob_cfloat*)(lf + FB_B1 + h * (BF_FFN / 2));
        // bias b2 added once (half 0); half 1 adds only the partial product
        // (compile-time: a runtime null test on the pointer, a VGPR in the
        // noinline callee, put an exec-mask branch in front of every quad)
        if (h == 0) {
          block_gemm_bar<BF_H, BF_FFN / 2, 0, 1, BF_H, ABL, true, true, TIMED>(
              x, XS, w1, b1, FfnHalf::ptr(), QKS, nullptr, nullptr, wid, lane,
              stamp);
          block_gemm_bar<BF_FFN / 2, BF_H, 3, 0, BF_FFN, ABL, true, false,
                         TIMED>(FfnHalf::ptr(), QKS, (glob_cshort*)(lw + LW_W2),
                                (glob_cfloat*)(lf + FB_B2), XMid::ptr(), XS, x,
                                nullptr, wid, lane, stamp);
        } else {
          block_gemm_bar<BF_H, BF_FFN / 2, 0, 1, BF_H, ABL, true, false, TIMED>(
              x, XS, w1, b1, FfnHalf::ptr(), QKS, nullptr, nullptr, wid, lane,
              stamp);
          block_gemm_bar<BF_FFN / 2, BF_H, 3, 0, BF_FFN, ABL, false, false,
                         TIMED>(
              FfnHalf::ptr(), QKS,
              (glob_cshort*)(lw + LW_W2 + (long)h * (BF_FFN / 2)), nullptr, x,
              XS, XMid::ptr(), nullptr, wid, lane, stamp);
        }
      }
      __syncthreads();
    } else {
      __syncthreads();
      stamp.mark();
    }
    if (PHASES & PH_LN)
      block_layernorm(x, lw + LW_LN2G, lw + LW_LN2B, wid, lane, eps);
    stamp.mark();
  }
  // the barrier that ends embed (no layers) or the last layer's LN2
  __syncthreads();
  stamp.mark();

  if constexpr (HEAD == HEAD_EMBED)
    pool_embed(emb, mu, inv_var, dist, line, tid);
  else
    pool_score(wb + WB_LAYER0 + (long)n_layers * LW_SIZE,
               fb + (long)n_layers * FB_SIZE, scores + line, tid);
  stamp.mark();
  stamp.flush(stamps_out, line, wid, lane);
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

// The same schedule with the embedding / distance head (pool_embed). A
// separate __global__: the production kernel's instruction stream is the same
// with and without it (profiles/r16_embed_head_isa.txt).
extern "C" __global__ __launch_bounds__(BF_THREADS, 4)
void dmx_bert_fused_embed_bf16(const unsigned char* __restrict__ lines,
                               const int* __restrict__ start,
                               const int* __restrict__ end,
                               const short* __restrict__ wb,
                               const float* __restrict__ fb,
                               float* __restrict__ emb,
                               const float* __restrict__ mu,
                               const float* __restrict__ inv_var,
                               float* __restrict__ dist, int B, int max_len,
                               int n_layers, float eps) {
  bert_fused_body<PH_ALL, false, 0, HEAD_EMBED>(lines, start, end, wb, fb,
                                                nullptr, B, max_len, n_layers,
                                                eps, nullptr, emb, mu, inv_var,
                                                dist);
}

// probe variants (in-kernel phase ablation; co-compiled variants can
// perturb codegen by a few % — read the deltas, not absolutes)
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
// The one launch path of all four entry points. BF_LDS_BYTES is above the
// default dynamic-LDS limit, so each (kernel, device) pair needs the opt-in
// attribute once; `attr_done` is that kernel's per-device flag array, which
// keeps the attribute call off the production kernel's per-launch path
// (unsynchronised on purpose: a racing second call sets the same value).
constexpr int BF_MAX_DEVICES = 64;
typedef bool AttrDone[BF_MAX_DEVICES];

template <typename... KArgs, typename... Args>
static hipError_t launch_bert_fused(void (*kernel)(KArgs...),
                                    AttrDone& attr_done, int B,
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
  static AttrDone attr_done;
  return launch_bert_fused(dmx_bert_fused_bf16, attr_done, B, stream, lines,
                           start, end, wb, fb, scores, B, max_len, n_layers,
                           eps);
}

extern "C" hipError_t dmx_launch_bert_fused_embed(
    const uint8_t* lines, const int32_t* start, const int32_t* end,
    const int16_t* wb, const float* fb, float* emb, const float* mu,
    const float* inv_var, float* dist, int B, int max_len, int n_layers,
    float eps, hipStream_t stream) {
  static AttrDone attr_done;
  return launch_bert_fused(dmx_bert_fused_embed_bf16, attr_done, B, stream,
                           lines, start, end, wb, fb, emb, mu, inv_var, dist,
                           B, max_len, n_layers, eps);
}

extern "C" hipError_t dmx_launch_bert_fused_timed(
    const uint8_t* lines, const int32_t* start, const int32_t* end,
    const int16_t* wb, const float* fb, float* scores, int64_t* stamps, int B,
    int max_len, int n_layers, float eps, hipStream_t stream) {
  static AttrDone attr_done;
  return launch_bert_fused(dmx_bert_fused_timed, attr_done, B, stream, lines,
                           start, end, wb, fb, scores, B, max_len, n_layers,
                           eps, (unsigned long long*)stamps);
}

// The compiled probe variants; phase_mask = phases | ablation << 8.
struct ProbeVariant {
  int mask;
  decltype(&dmx_bert_fused_probe<0, 0>) kernel;
  AttrDone attr_done;
};
template <int PHASES, int ABL = 0>
constexpr ProbeVariant probe_variant() {
  return {PHASES | (ABL << 8), dmx_bert_fused_probe<PHASES, ABL>, {}};
}
static ProbeVariant probe_variants[] = {
    probe_variant<0>(),
    probe_variant<PH_QKV>(),
    probe_variant<PH_QKV | PH_ATTN>(),
    probe_variant<PH_QKV | PH_ATTN | PH_PROJ>(),
    probe_variant<PH_QKV | PH_ATTN | PH_PROJ | PH_LN>(),
    probe_variant<PH_ALL>(),
    probe_variant<PH_FFN>(),
    probe_variant<PH_LN>(),
    // perf-ablation variants (numerically wrong by design):
    probe_variant<PH_ALL, 1>(),  // B operand constant (no L2 weight loads)
    probe_variant<PH_ALL, 2>(),  // A operand constant (no LDS reads)
    probe_variant<PH_ALL, 3>(),  // both constant (pure MFMA + epilogue)
    probe_variant<PH_FFN, 1>(),
    probe_variant<PH_FFN, 2>(),
    probe_variant<PH_FFN, 3>(),
};

static ProbeVariant* find_probe_variant(int phase_mask) {
  for (ProbeVariant& v : probe_variants)
    if (v.mask == phase_mask) return &v;
  return nullptr;
}

extern "C" bool dmx_bert_fused_probe_mask_known(int phase_mask) {
  return find_probe_variant(phase_mask) != nullptr;
}

extern "C" hipError_t dmx_launch_bert_fused_probe(
    const uint8_t* lines, const int32_t* start, const int32_t* end,
    const int16_t* wb, const float* fb, float* scores, int B, int max_len,
    int n_layers, float eps, int phase_mask, hipStream_t stream) {
  ProbeVariant* v = find_probe_variant(phase_mask);
  if (v == nullptr) return hipErrorInvalidValue;
  return launch_bert_fused(v->kernel, v->attr_done, B, stream, lines, start,
                           end, wb, fb, scores, B, max_len, n_layers, eps);
}
