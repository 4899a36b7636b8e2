// The launch boundary between the torch bindings and the HIP kernels.
//
// Every dmx_launch_* is declared HERE and nowhere else. bindings.cpp and
// each .hip that defines a launcher include this header, so a parameter
// added or reordered on one side only is a "conflicting types" compile
// error instead of garbage handed to the GPU (extern "C" names carry no
// signature). The header also owns every limit and layout constant that
// both sides need; it is host-includable and needs only the HIP runtime
// API header.
//
// Pointer conventions: bf16 tensors travel as int16_t (raw bits), u8 as
// uint8_t, int32 as int32_t, int64 hash words as int64_t (the kernels
// reinterpret them as unsigned 64-bit).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

// ---- limits the bindings check before launch -------------------------------
constexpr int GEMM_K_MULTIPLE = 64;   // fused_linear: K % 64 == 0 (BK tile)
constexpr int LN_MAX_D = 2048;        // layernorm: D % 64 == 0, D <= 2048
constexpr int ATTN_MAX_S = 128;       // attention (VALU and MFMA): S <= 128
constexpr int ATTN_MAX_DH = 64;       // attention: Dh <= 64
constexpr int AM_WAVES = 4;           // MFMA attention: waves per (b, h)
constexpr int ED_MAX_LEN = 256;       // edit_distance: bytes per string
constexpr int TM_WAVES = 4;           // template_match: lines per workgroup
constexpr int TM_MAX_LINE = 512;      // template_match: bytes per line
constexpr int LDS_DEFAULT_LIMIT = 64 * 1024;  // dynamic LDS without opt-in
constexpr int ER_MAX_EVENTS = 8192;   // event_rate: bins (32 KiB LDS histogram)
constexpr int64_t ER_MAX_CELLS = int64_t(1) << 24;  // event_rate: NW * E
constexpr int VR_MAX_SPAN = 17;       // value_range: bytes of a number
constexpr int VR_MAX_DIGITS = 15;     // value_range: digits (10^15 < 2^53)
constexpr int SEQ_MAX_LEN = 4;        // event_sequence: symbols of 16 bits
constexpr int SEQ_MAX_KEYS = 1 << 24; // event_sequence: history buckets
constexpr int SEQ_MAX_EVENTS = 65535; // event_sequence: a symbol is 16 bits

// Dynamic LDS of dmx_template_match: the segment blob (16-B rounded) plus
// one staged line per wave. The kernel carves its arena the same way.
constexpr int tm_seg_lds_bytes(int seg_bytes_len) {
  return (seg_bytes_len + 15) & ~15;
}
constexpr size_t tm_lds_bytes(int seg_bytes_len) {
  return tm_seg_lds_bytes(seg_bytes_len) + TM_WAVES * TM_MAX_LINE;
}

// Window slots of one dmx_event_rate call: B lines on top of an open window
// of up to L - 1 lines complete at most B / L + 1 windows and leave one open.
constexpr int er_window_slots(int64_t B, int64_t window_lines) {
  return (int)(B / window_lines + 2);
}

// ---- fused BERT-tiny kernel: fixed geometry --------------------------------
constexpr int BF_WAVES = 8;
constexpr int BF_S = 64;       // tokens per line
constexpr int BF_H = 128;      // hidden
constexpr int BF_HEADS = 2;
constexpr int BF_DH = 64;      // head dim
constexpr int BF_FFN = 512;
constexpr int BF_VOCAB = 259;  // 256 byte values + pad/cls/unused
constexpr int BF_NSTAMP = 22;  // timed variant: stamps per wave
// Dynamic LDS of the fused kernel (x | Q,K / P+O / FFN-half | Vt | pooling).
// bert_fused.hip static_asserts this against its private strides.
constexpr int BF_LDS_BYTES = 72192;

// bf16 weight blob (element offsets):
//   tok_emb [VOCAB,H] | pos_emb [S,H] | n_layers x layer | w_score [H]
// layer: wqkv_t [3H,H] | wo_t [H,H] | w1_t [FFN,H] | w2_t [H,FFN] |
//        ln1_g | ln1_b | ln2_g | ln2_b  (each [H])
constexpr int WB_TOK = 0;
constexpr int WB_POS = WB_TOK + BF_VOCAB * BF_H;
constexpr int WB_LAYER0 = WB_POS + BF_S * BF_H;
constexpr int LW_QKV = 0;
constexpr int LW_WO = LW_QKV + 3 * BF_H * BF_H;
constexpr int LW_W1 = LW_WO + BF_H * BF_H;
constexpr int LW_W2 = LW_W1 + BF_FFN * BF_H;
constexpr int LW_LN1G = LW_W2 + BF_H * BF_FFN;
constexpr int LW_LN1B = LW_LN1G + BF_H;
constexpr int LW_LN2G = LW_LN1B + BF_H;
constexpr int LW_LN2B = LW_LN2G + BF_H;
constexpr int LW_SIZE = LW_LN2B + BF_H;
// f32 bias blob: per layer [bqkv 3H | bo H | b1 FFN | b2 H], then b_score
constexpr int FB_BQKV = 0;
constexpr int FB_BO = FB_BQKV + 3 * BF_H;
constexpr int FB_B1 = FB_BO + BF_H;
constexpr int FB_B2 = FB_B1 + BF_FFN;
constexpr int FB_SIZE = FB_B2 + BF_H;

constexpr int64_t bert_fused_wb_elems(int n_layers) {
  return WB_LAYER0 + (int64_t)n_layers * LW_SIZE + BF_H;
}
constexpr int64_t bert_fused_fb_elems(int n_layers) {
  return (int64_t)n_layers * FB_SIZE + 1;
}

// ---- the parsed batch --------------------------------------------------------
// What dmx_template_match wrote for B lines of max_len bytes, as the field
// kernels read it (field_span.h; docs/kernels.md, "Parsed batch and field
// span"). Passed by value, to the launchers and on to the kernels.
struct ParsedBatch {
  const uint8_t* lines;       // [B, max_len]
  const int32_t* event_id;    // [B]
  const int32_t* caps;        // [B, max_caps, 2] (start, end) per capture
  const int32_t* n_caps;      // [B]
  const int32_t* fmt_caps;    // [B, max_fmt_caps, 2] header fields
  const int32_t* n_fmt_caps;  // [B]
  int B, max_len, max_caps, max_fmt_caps;
};

// ---- launchers --------------------------------------------------------------
// Each enqueues on `stream` of the CURRENT device and does not synchronize.
// The void ones report failure through hipGetLastError(); the fused-BERT
// ones also set a per-(kernel, device) function attribute and can be
// handed an unknown probe variant, so they return the error themselves.
extern "C" {

// gemm_bf16.hip
void dmx_launch_fused_linear_bf16(const int16_t* A, const int16_t* Wt,
                                  const float* bias, int16_t* C, int M, int N,
                                  int K, int epilogue, hipStream_t stream);
void dmx_launch_probe_mfma(const int16_t* A, const int16_t* B, float* D,
                           int a_layout, int b_layout, hipStream_t stream);
void dmx_launch_probe_mfma32(const int16_t* A, const int16_t* B, float* D,
                             hipStream_t stream);

// layernorm.hip (R and Xres may be null)
void dmx_launch_layernorm_bf16(const int16_t* X, const int16_t* R,
                               const int16_t* gamma, const int16_t* beta,
                               int16_t* Y, int16_t* Xres, int M, int D,
                               float eps, hipStream_t stream);

// attention.hip, attention_mfma.hip
void dmx_launch_attention_bf16(const int16_t* Q, const int16_t* K,
                               const int16_t* V, int16_t* O, int BH, int S,
                               int Dh, float scale, hipStream_t stream);
void dmx_launch_attention_mfma_bf16(const int16_t* QKV, int16_t* O, int B,
                                    int S, int H, int Dh, float scale,
                                    hipStream_t stream);

// bert_fused.hip
hipError_t dmx_launch_bert_fused_bf16(const uint8_t* lines,
                                      const int32_t* start, const int32_t* end,
                                      const int16_t* wb, const float* fb,
                                      float* scores, int B, int max_len,
                                      int n_layers, float eps,
                                      hipStream_t stream);
// Same forward, embedding / distance head. emb [B, BF_H] or null; mu and
// inv_var [BF_H], both or neither; dist [B], written when mu is given.
hipError_t dmx_launch_bert_fused_embed(const uint8_t* lines,
                                       const int32_t* start,
                                       const int32_t* end, const int16_t* wb,
                                       const float* fb, float* emb,
                                       const float* mu, const float* inv_var,
                                       float* dist, int B, int max_len,
                                       int n_layers, float eps,
                                       hipStream_t stream);
// hipErrorInvalidValue when phase_mask names no compiled variant
hipError_t dmx_launch_bert_fused_probe(const uint8_t* lines,
                                       const int32_t* start,
                                       const int32_t* end, const int16_t* wb,
                                       const float* fb, float* scores, int B,
                                       int max_len, int n_layers, float eps,
                                       int phase_mask, hipStream_t stream);
bool dmx_bert_fused_probe_mask_known(int phase_mask);
// stamps: [B, BF_WAVES, BF_NSTAMP] u64 clock words
hipError_t dmx_launch_bert_fused_timed(const uint8_t* lines,
                                       const int32_t* start,
                                       const int32_t* end, const int16_t* wb,
                                       const float* fb, float* scores,
                                       int64_t* stamps, int B, int max_len,
                                       int n_layers, float eps,
                                       hipStream_t stream);

// template_match.hip (fmt_bytes / fmt_seg_off null when nf_seg == 0)
void dmx_launch_template_match(
    const uint8_t* lines, const int32_t* line_len, int B, int max_len,
    const uint8_t* fmt_bytes, const int32_t* fmt_seg_off, int nf_seg,
    const uint8_t* seg_bytes, int seg_bytes_len, const int32_t* seg_off,
    const int32_t* tpl_seg_start, int n_tpl, int lower, int32_t* event_id,
    int32_t* fmt_caps, int32_t* n_fmt_caps, int32_t* caps, int32_t* n_caps,
    int32_t* span_start, int32_t* span_end, int max_fmt_caps, int max_caps,
    hipStream_t stream);

// hashset.hip (specs: [W, 4] int32 = kind, event, pos, pad)
void dmx_launch_watch_hashes(ParsedBatch batch, const int32_t* specs, int W,
                             int lower, int64_t* hashes, hipStream_t stream);
// hashes [B, W + C]: the W watch columns, then one column per combination.
// members: [M, 4] int32 rows laid out like specs; combo_off: [C + 1] int32,
// combination c owns member rows combo_off[c] .. combo_off[c + 1].
void dmx_launch_watch_combo_hashes(ParsedBatch batch, const int32_t* specs,
                                   int W, const int32_t* members, int M,
                                   const int32_t* combo_off, int C, int lower,
                                   int64_t* hashes, hipStream_t stream);
void dmx_launch_hashset_insert(const int64_t* hashes, int64_t* tables, int B,
                               int W, int capacity, hipStream_t stream);
void dmx_launch_hashset_probe(const int64_t* hashes, const int64_t* tables,
                              int B, int W, int capacity, int32_t* unseen,
                              hipStream_t stream);

// event_rate.hip: one batch of the event-rate stage (count + roll launches).
// State, updated in place: mean, var f64 [E]; known, open_counts int32 [E];
// ctl int32 [2] = in_window, windows_seen. n_valid: device int32 [1].
// Outputs, NW = er_window_slots(B, window_lines): rate_counts int32 [NW, E],
// rate_z f64 [NW, E], rate_hits and rate_slot int32 [B]. All fully written.
// base: f64 [NW, E] scratch of the roll kernel, contents unspecified.
void dmx_launch_event_rate(const int32_t* event_id, const int32_t* n_valid,
                           int B, int E, int window_lines, int train_upto,
                           double ewma_alpha, double z_threshold,
                           int min_windows, double* mean, double* var,
                           int32_t* known, int32_t* open_counts, int32_t* ctl,
                           double* base, int32_t* rate_counts, double* rate_z,
                           int32_t* rate_hits, int32_t* rate_slot,
                           hipStream_t stream);

// value_range.hip: one batch of the value-range stage (the fit launch only
// when train_upto > 0, then the judge launch). specs: [R, 4] int32 rows laid
// out like the watch specs, the pad word holding flags (bit 0 = a field that
// is not a number alerts). slack f64 [R], read only. State, updated in
// place: lo, hi f64 [R]; n int64 [R]. Outputs, fully written: range_code
// int32 [B, R], range_value f64 [B, R].
void dmx_launch_value_range(ParsedBatch batch, const int32_t* specs, int R,
                            const double* slack, double* lo, double* hi,
                            int64_t* n, int train_upto, int32_t* range_code,
                            double* range_value, hipStream_t stream);

// event_sequence.hip: one batch of the event-sequence stage (keys launch,
// rocPRIM radix sort, grams launch, commit launch). The key field is a watch
// spec by value, key_kind < 0 = no key (the stream is one sequence). n_valid:
// device int32 [1]; T templates, K buckets (a power of two), length symbols
// per gram. State, updated in place: seq_key, seq_hist int64 [K]. Scratch,
// contents unspecified: kh int64 [B]; words int64 [2, B] (sort input and
// output); sort_temp of the sort_temp_bytes that dmx_seq_sort_temp_bytes
// reports for (B, K), never null. Outputs, fully written: seq_gram and
// gram_hash int64 [B]. B >= 1.
hipError_t dmx_seq_sort_temp_bytes(int B, int K, hipStream_t stream,
                                   size_t* bytes);
hipError_t dmx_launch_event_sequence(
    ParsedBatch batch, int key_kind, int key_event, int key_pos, int lower,
    const int32_t* n_valid, int T, int K, int length, int64_t* seq_key,
    int64_t* seq_hist, int64_t* kh, int64_t* words, void* sort_temp,
    size_t sort_temp_bytes, int64_t* seq_gram, int64_t* gram_hash,
    hipStream_t stream);

// edit_distance.hip: dist [Na, Nb] int32. A and B are [N, max_len] rows with
// max_len <= ED_MAX_LEN; the kernel clamps every word of a_len and b_len to
// [0, min(max_len, ED_MAX_LEN)], so a length word never reaches past its row.
void dmx_launch_edit_distance(const uint8_t* A, const int32_t* a_len, int Na,
                              const uint8_t* B, const int32_t* b_len, int Nb,
                              int max_len, int32_t* dist, hipStream_t stream);

}  // extern "C"
