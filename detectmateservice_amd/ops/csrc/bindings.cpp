// Torch extension bindings for the detectmate-mi355x HIP kernels.
//
// All entry points validate every tensor they pass down (dtype, rank,
// contiguity, shape relations, one common GPU), run on the current torch
// HIP stream of the tensors' device, read the launch result, and are
// gfx950-only (no CPU fallback here — the Python layer in
// detectmateservice_amd/ops/__init__.py owns the CPU path and fails loudly
// when this extension is missing on a GPU box).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <c10/hip/HIPException.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>

#include "kernels.h"

namespace {

// ---- launch contract helpers ------------------------------------------------
// Every binding (1) validates each tensor it passes down with check_arg /
// check_numel / check_same_shape, (2) checks devices LAST with DeviceScope,
// so every other clause can be exercised with CPU tensors, (3) returns an
// empty result instead of launching a zero-sized grid, (4) launches on the
// current stream of the tensors' device and (5) reads the launch result.

void check_arg(const torch::Tensor& t, const char* name, c10::ScalarType dtype,
               int64_t dim) {
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", dtype, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == dim, name, " must be ", dim, "-D, got ", t.dim(),
              "-D");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_numel(const torch::Tensor& t, const char* name, int64_t n,
                 const char* what) {
  TORCH_CHECK(t.numel() == n, name, " must hold ", what, " = ", n,
              " elements, got ", t.numel());
}

void check_same_shape(const torch::Tensor& t, const char* name,
                      const torch::Tensor& ref, const char* ref_name) {
  TORCH_CHECK(t.sizes() == ref.sizes(), name, " must be shaped like ",
              ref_name, " ", ref.sizes(), ", got ", t.sizes());
}

// [B, n, 2] int32 capture table
void check_caps(const torch::Tensor& t, const char* name, int64_t B) {
  check_arg(t, name, torch::kInt32, 3);
  TORCH_CHECK(t.size(0) == B && t.size(1) >= 1 && t.size(2) == 2, name,
              " must be [B=", B, ", n>=1, 2], got ", t.sizes());
}

struct Arg {
  const char* name;
  const torch::Tensor& t;
};

// Device clause + launch scope: the first argument must live on a GPU and
// every other one on the same GPU; that device is made current for the
// scope's lifetime, so the current stream and the kernel launch belong to
// the tensors' device rather than to whatever device the caller left set.
class DeviceScope {
 public:
  // `more` continues `args` (parsed_batch_scope puts its own list first)
  DeviceScope(std::initializer_list<Arg> args,
              std::initializer_list<Arg> more = {}) {
    const Arg& first = *args.begin();
    TORCH_CHECK(first.t.is_cuda(), first.name, " must be on a GPU, got ",
                first.t.device());
    for (const auto& list : {args, more})
      for (const Arg& a : list)
        TORCH_CHECK(a.t.device() == first.t.device(), a.name, " must be on ",
                    first.name, "'s device ", first.t.device(), ", got ",
                    a.t.device());
    guard_.set_device(first.t.device());
    stream_ = at::hip::getCurrentHIPStream().stream();
  }
  hipStream_t stream() const { return stream_; }

 private:
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard_;
  hipStream_t stream_ = nullptr;
};

const int16_t* bf16_in(const torch::Tensor& t) {
  return static_cast<const int16_t*>(t.data_ptr());
}
int16_t* bf16_out(torch::Tensor& t) {
  return static_cast<int16_t*>(t.data_ptr());
}

// ---- dense ops ----------------------------------------------------------------

torch::Tensor fused_linear_bf16(torch::Tensor x, torch::Tensor wt,
                                c10::optional<torch::Tensor> bias,
                                int64_t epilogue) {
  check_arg(x, "x", torch::kBFloat16, 2);
  check_arg(wt, "wt", torch::kBFloat16, 2);
  const auto M = x.size(0), K = x.size(1), N = wt.size(0);
  TORCH_CHECK(wt.size(1) == K, "wt must be [N, K=", K,
              "] (pre-transposed weight), got ", wt.sizes());
  TORCH_CHECK(K % GEMM_K_MULTIPLE == 0, "x: K must be a multiple of ",
              GEMM_K_MULTIPLE, ", got ", K);
  TORCH_CHECK(epilogue >= 0 && epilogue <= 2, "epilogue must be 0, 1 or 2");
  const bool has_bias = bias.has_value() && bias->defined();
  if (has_bias) {
    check_arg(*bias, "bias", torch::kFloat32, 1);
    check_numel(*bias, "bias", N, "N");
  }
  DeviceScope dev({{"x", x}, {"wt", wt}, {"bias", has_bias ? *bias : x}});
  auto C = torch::empty({M, N}, x.options());
  if (M == 0 || N == 0) return C;
  dmx_launch_fused_linear_bf16(bf16_in(x), bf16_in(wt),
                               has_bias ? bias->data_ptr<float>() : nullptr,
                               bf16_out(C), (int)M, (int)N, (int)K,
                               (int)epilogue, dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return C;
}

torch::Tensor probe_mfma32(torch::Tensor A, torch::Tensor B) {
  check_arg(A, "A", torch::kBFloat16, 2);
  check_arg(B, "B", torch::kBFloat16, 2);
  TORCH_CHECK(A.size(0) == 32 && A.size(1) == 16, "A must be 32x16");
  TORCH_CHECK(B.size(0) == 16 && B.size(1) == 32, "B must be 16x32");
  DeviceScope dev({{"A", A}, {"B", B}});
  auto D = torch::zeros({32, 32}, A.options().dtype(torch::kFloat32));
  dmx_launch_probe_mfma32(bf16_in(A), bf16_in(B), D.data_ptr<float>(),
                          dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return D;
}

torch::Tensor probe_mfma(torch::Tensor A, torch::Tensor B, int64_t a_layout,
                         int64_t b_layout) {
  check_arg(A, "A", torch::kBFloat16, 2);
  check_arg(B, "B", torch::kBFloat16, 2);
  TORCH_CHECK(A.size(0) == 16 && A.size(1) == 32, "A must be 16x32");
  TORCH_CHECK(B.size(0) == 32 && B.size(1) == 16, "B must be 32x16");
  DeviceScope dev({{"A", A}, {"B", B}});
  auto D = torch::zeros({16, 16}, A.options().dtype(torch::kFloat32));
  dmx_launch_probe_mfma(bf16_in(A), bf16_in(B), D.data_ptr<float>(),
                        (int)a_layout, (int)b_layout, dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return D;
}

std::vector<torch::Tensor> layernorm_bf16(torch::Tensor x,
                                          c10::optional<torch::Tensor> res,
                                          torch::Tensor gamma,
                                          torch::Tensor beta, double eps,
                                          bool want_xres) {
  check_arg(x, "x", torch::kBFloat16, 2);
  const auto M = x.size(0), D = x.size(1);
  TORCH_CHECK(D % 64 == 0 && D <= LN_MAX_D,
              "x: D must be a multiple of 64, <= ", LN_MAX_D, ", got ", D);
  const bool has_res = res.has_value() && res->defined();
  if (has_res) {
    check_arg(*res, "res", torch::kBFloat16, 2);
    check_same_shape(*res, "res", x, "x");
  }
  check_arg(gamma, "gamma", torch::kBFloat16, 1);
  check_numel(gamma, "gamma", D, "D");
  check_arg(beta, "beta", torch::kBFloat16, 1);
  check_numel(beta, "beta", D, "D");
  DeviceScope dev({{"x", x},
                   {"res", has_res ? *res : x},
                   {"gamma", gamma},
                   {"beta", beta}});
  auto y = torch::empty_like(x);
  torch::Tensor xres;
  if (want_xres) xres = torch::empty_like(x);
  if (M > 0) {
    dmx_launch_layernorm_bf16(bf16_in(x), has_res ? bf16_in(*res) : nullptr,
                              bf16_in(gamma), bf16_in(beta), bf16_out(y),
                              want_xres ? bf16_out(xres) : nullptr, (int)M,
                              (int)D, (float)eps, dev.stream());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  if (want_xres) return {y, xres};
  return {y};
}

torch::Tensor attention_bf16(torch::Tensor q, torch::Tensor k,
                             torch::Tensor v, double scale) {
  check_arg(q, "q", torch::kBFloat16, 3);  // [BH, S, Dh]
  check_arg(k, "k", torch::kBFloat16, 3);
  check_same_shape(k, "k", q, "q");
  check_arg(v, "v", torch::kBFloat16, 3);
  check_same_shape(v, "v", q, "q");
  const auto BH = q.size(0), S = q.size(1), Dh = q.size(2);
  TORCH_CHECK(S >= 1 && S <= ATTN_MAX_S && Dh >= 8 && Dh <= ATTN_MAX_DH &&
                  Dh % 8 == 0,
              "q: attention kernel supports 1<=S<=", ATTN_MAX_S, ", Dh<=",
              ATTN_MAX_DH, " (multiple of 8), got ", q.sizes());
  DeviceScope dev({{"q", q}, {"k", k}, {"v", v}});
  auto o = torch::empty_like(q);
  if (BH == 0) return o;
  dmx_launch_attention_bf16(bf16_in(q), bf16_in(k), bf16_in(v), bf16_out(o),
                            (int)BH, (int)S, (int)Dh, (float)scale,
                            dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return o;
}

torch::Tensor attention_qkv_bf16(torch::Tensor qkv, int64_t S, int64_t H,
                                 int64_t Dh, double scale) {
  check_arg(qkv, "qkv", torch::kBFloat16, 3);
  TORCH_CHECK(S >= 32 && S % 32 == 0 && S <= ATTN_MAX_S,
              "S: MFMA attention needs S%32==0, 32<=S<=", ATTN_MAX_S, ", got ",
              S);
  TORCH_CHECK(Dh == 32 || Dh == 64, "Dh: MFMA attention needs Dh in {32,64}");
  TORCH_CHECK(H >= 1, "H must be >= 1");
  TORCH_CHECK(qkv.size(1) == S && qkv.size(2) == 3 * H * Dh,
              "qkv must be [B, S=", S, ", 3*H*Dh=", 3 * H * Dh, "], got ",
              qkv.sizes());
  DeviceScope dev({{"qkv", qkv}});
  const auto B = qkv.size(0);
  auto O = torch::empty({B, S, H * Dh}, qkv.options());
  if (B == 0) return O;
  dmx_launch_attention_mfma_bf16(bf16_in(qkv), bf16_out(O), (int)B, (int)S,
                                 (int)H, (int)Dh, (float)scale, dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return O;
}

// ---- fused BERT-tiny ------------------------------------------------------------

// A [BF_H] f32 statistics vector of the embedding head (mu, inv_var).
void check_embed_stat(const torch::Tensor& t, const char* name) {
  check_arg(t, name, torch::kFloat32, 1);
  check_numel(t, name, BF_H, "BF_H");
}

// Everything the fused entry points share, device clause last. The embed
// entry point hands its two statistics vectors (both or neither) through
// here so that their clauses also come before the device clause.
DeviceScope check_bert_fused_args(const torch::Tensor& lines,
                                  const torch::Tensor& start,
                                  const torch::Tensor& end,
                                  const torch::Tensor& wb,
                                  const torch::Tensor& fb, int64_t n_layers,
                                  const torch::Tensor* mu = nullptr,
                                  const torch::Tensor* inv_var = nullptr) {
  check_arg(lines, "lines", torch::kUInt8, 2);
  const auto B = lines.size(0);
  check_arg(start, "start", torch::kInt32, 1);
  check_numel(start, "start", B, "B");
  check_arg(end, "end", torch::kInt32, 1);
  check_numel(end, "end", B, "B");
  TORCH_CHECK(n_layers >= 1, "n_layers must be >= 1, got ", n_layers);
  check_arg(wb, "wb", torch::kBFloat16, 1);
  check_numel(wb, "wb", bert_fused_wb_elems((int)n_layers),
              "bert_fused_wb_elems(n_layers)");
  check_arg(fb, "fb", torch::kFloat32, 1);
  check_numel(fb, "fb", bert_fused_fb_elems((int)n_layers),
              "bert_fused_fb_elems(n_layers)");
  // the kernel fetches four biases with one 16-byte load (a storage-offset
  // view of a larger tensor can be contiguous and still start mid-vector)
  TORCH_CHECK(reinterpret_cast<uintptr_t>(fb.data_ptr<float>()) % 16 == 0,
              "fb: bias blob must be 16-byte aligned, got storage offset ",
              fb.storage_offset(), " floats");
  if (mu != nullptr) check_embed_stat(*mu, "mu");
  if (inv_var != nullptr) check_embed_stat(*inv_var, "inv_var");
  return DeviceScope({{"lines", lines},
                      {"start", start},
                      {"end", end},
                      {"wb", wb},
                      {"fb", fb},
                      {"mu", mu != nullptr ? *mu : lines},
                      {"inv_var", inv_var != nullptr ? *inv_var : lines}});
}

torch::Tensor bert_fused_bf16(torch::Tensor lines, torch::Tensor start,
                              torch::Tensor end, torch::Tensor wb,
                              torch::Tensor fb, int64_t n_layers,
                              double eps) {
  DeviceScope dev = check_bert_fused_args(lines, start, end, wb, fb, n_layers);
  const auto B = lines.size(0), max_len = lines.size(1);
  auto scores = torch::empty({B}, lines.options().dtype(torch::kFloat32));
  if (B == 0) return scores;
  C10_HIP_CHECK(dmx_launch_bert_fused_bf16(
      lines.data_ptr<uint8_t>(), start.data_ptr<int32_t>(),
      end.data_ptr<int32_t>(), bf16_in(wb), fb.data_ptr<float>(),
      scores.data_ptr<float>(), (int)B, (int)max_len, (int)n_layers,
      (float)eps, dev.stream()));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return scores;
}

// Same forward, embedding / distance head: (emb [B, BF_H] | None,
// dist [B] | None). dist needs the fitted statistics mu and inv_var.
py::tuple bert_fused_embed(torch::Tensor lines, torch::Tensor start,
                           torch::Tensor end, torch::Tensor wb,
                           torch::Tensor fb, int64_t n_layers, double eps,
                           c10::optional<torch::Tensor> mu,
                           c10::optional<torch::Tensor> inv_var,
                           bool want_emb) {
  const bool has_mu = mu.has_value() && mu->defined();
  const bool has_iv = inv_var.has_value() && inv_var->defined();
  TORCH_CHECK(!has_mu || has_iv, "inv_var must be given together with mu");
  TORCH_CHECK(!has_iv || has_mu, "mu must be given together with inv_var");
  TORCH_CHECK(want_emb || has_mu,
              "want_emb must be true when mu and inv_var are not given: "
              "there would be no output");
  DeviceScope dev =
      check_bert_fused_args(lines, start, end, wb, fb, n_layers,
                            has_mu ? &*mu : nullptr, has_iv ? &*inv_var : nullptr);
  const auto B = lines.size(0), max_len = lines.size(1);
  const auto f32 = lines.options().dtype(torch::kFloat32);
  torch::Tensor emb, dist;
  if (want_emb) emb = torch::empty({B, BF_H}, f32);
  if (has_mu) dist = torch::empty({B}, f32);
  if (B > 0) {
    C10_HIP_CHECK(dmx_launch_bert_fused_embed(
        lines.data_ptr<uint8_t>(), start.data_ptr<int32_t>(),
        end.data_ptr<int32_t>(), bf16_in(wb), fb.data_ptr<float>(),
        want_emb ? emb.data_ptr<float>() : nullptr,
        has_mu ? mu->data_ptr<float>() : nullptr,
        has_mu ? inv_var->data_ptr<float>() : nullptr,
        has_mu ? dist.data_ptr<float>() : nullptr, (int)B, (int)max_len,
        (int)n_layers, (float)eps, dev.stream()));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return py::make_tuple(want_emb ? py::cast(emb) : py::none(),
                        has_mu ? py::cast(dist) : py::none());
}

torch::Tensor bert_fused_probe(torch::Tensor lines, torch::Tensor start,
                               torch::Tensor end, torch::Tensor wb,
                               torch::Tensor fb, int64_t n_layers, double eps,
                               int64_t phase_mask) {
  TORCH_CHECK(phase_mask >= 0 && phase_mask <= INT32_MAX &&
                  dmx_bert_fused_probe_mask_known((int)phase_mask),
              "phase_mask ", phase_mask, " names no compiled probe variant");
  DeviceScope dev = check_bert_fused_args(lines, start, end, wb, fb, n_layers);
  const auto B = lines.size(0), max_len = lines.size(1);
  auto scores = torch::empty({B}, lines.options().dtype(torch::kFloat32));
  if (B == 0) return scores;
  C10_HIP_CHECK(dmx_launch_bert_fused_probe(
      lines.data_ptr<uint8_t>(), start.data_ptr<int32_t>(),
      end.data_ptr<int32_t>(), bf16_in(wb), fb.data_ptr<float>(),
      scores.data_ptr<float>(), (int)B, (int)max_len, (int)n_layers,
      (float)eps, (int)phase_mask, dev.stream()));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return scores;
}

std::vector<torch::Tensor> bert_fused_timed(torch::Tensor lines,
                                            torch::Tensor start,
                                            torch::Tensor end,
                                            torch::Tensor wb,
                                            torch::Tensor fb,
                                            int64_t n_layers, double eps) {
  DeviceScope dev = check_bert_fused_args(lines, start, end, wb, fb, n_layers);
  const auto B = lines.size(0), max_len = lines.size(1);
  auto scores = torch::empty({B}, lines.options().dtype(torch::kFloat32));
  auto stamps = torch::zeros({B, BF_WAVES, BF_NSTAMP},
                             lines.options().dtype(torch::kInt64));
  if (B == 0) return {scores, stamps};
  C10_HIP_CHECK(dmx_launch_bert_fused_timed(
      lines.data_ptr<uint8_t>(), start.data_ptr<int32_t>(),
      end.data_ptr<int32_t>(), bf16_in(wb), fb.data_ptr<float>(),
      scores.data_ptr<float>(), stamps.data_ptr<int64_t>(), (int)B,
      (int)max_len, (int)n_layers, (float)eps, dev.stream()));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {scores, stamps};
}

// The fused kernel's geometry and blob layout, for the Python side to pack
// against and to compare a model config with (no copy of these numbers
// lives in Python). Keys named like BertTinyConfig fields where one exists.
py::dict bert_fused_layout(int64_t n_layers) {
  TORCH_CHECK(n_layers >= 0 && n_layers <= 1024,
              "n_layers must be in [0, 1024], got ", n_layers);
  const int64_t wb_score = WB_LAYER0 + n_layers * LW_SIZE;
  py::dict d;
  d["max_seq"] = BF_S;
  d["hidden"] = BF_H;
  d["heads"] = BF_HEADS;
  d["head_dim"] = BF_DH;
  d["ffn"] = BF_FFN;
  d["vocab_size"] = BF_VOCAB;
  d["waves"] = BF_WAVES;
  d["nstamp"] = BF_NSTAMP;
  d["lds_bytes"] = BF_LDS_BYTES;
  d["wb_elems"] = bert_fused_wb_elems((int)n_layers);
  d["fb_elems"] = bert_fused_fb_elems((int)n_layers);
  d["wb_tok"] = WB_TOK;
  d["wb_pos"] = WB_POS;
  d["wb_layer0"] = WB_LAYER0;
  d["wb_score"] = wb_score;
  d["lw_qkv"] = LW_QKV;
  d["lw_wo"] = LW_WO;
  d["lw_w1"] = LW_W1;
  d["lw_w2"] = LW_W2;
  d["lw_ln1g"] = LW_LN1G;
  d["lw_ln1b"] = LW_LN1B;
  d["lw_ln2g"] = LW_LN2G;
  d["lw_ln2b"] = LW_LN2B;
  d["lw_size"] = LW_SIZE;
  d["fb_bqkv"] = FB_BQKV;
  d["fb_bo"] = FB_BO;
  d["fb_b1"] = FB_B1;
  d["fb_b2"] = FB_B2;
  d["fb_size"] = FB_SIZE;
  d["fb_score"] = n_layers * FB_SIZE;
  return d;
}

// ---- parser / detector ------------------------------------------------------------

std::vector<torch::Tensor> template_match(
    torch::Tensor lines, torch::Tensor line_len, torch::Tensor fmt_bytes,
    torch::Tensor fmt_seg_off, torch::Tensor seg_bytes, torch::Tensor seg_off,
    torch::Tensor tpl_seg_start, bool lower, int64_t max_fmt_caps,
    int64_t max_caps) {
  check_arg(lines, "lines", torch::kUInt8, 2);
  const auto B = lines.size(0), max_len = lines.size(1);
  TORCH_CHECK(max_len <= TM_MAX_LINE, "lines: max_len must be <= ",
              TM_MAX_LINE, " (TM_MAX_LINE), got ", max_len);
  check_arg(line_len, "line_len", torch::kInt32, 1);
  check_numel(line_len, "line_len", B, "B");
  check_arg(fmt_bytes, "fmt_bytes", torch::kUInt8, 1);
  check_arg(fmt_seg_off, "fmt_seg_off", torch::kInt32, 1);
  check_arg(seg_bytes, "seg_bytes", torch::kUInt8, 1);
  check_arg(seg_off, "seg_off", torch::kInt32, 1);
  check_arg(tpl_seg_start, "tpl_seg_start", torch::kInt32, 1);
  TORCH_CHECK(seg_off.numel() >= 1, "seg_off must hold at least one offset");
  TORCH_CHECK(tpl_seg_start.numel() >= 1,
              "tpl_seg_start must hold at least one offset");
  TORCH_CHECK(max_fmt_caps >= 1 && max_caps >= 1,
              "max_fmt_caps and max_caps must be >= 1");
  // the kernel stages the whole segment blob in LDS and its launcher does
  // not raise the per-kernel dynamic-LDS limit
  TORCH_CHECK(seg_bytes.numel() <= LDS_DEFAULT_LIMIT &&
                  tm_lds_bytes((int)seg_bytes.numel()) <= LDS_DEFAULT_LIMIT,
              "seg_bytes: a template segment blob of ", seg_bytes.numel(),
              " bytes needs more than the ", LDS_DEFAULT_LIMIT,
              " bytes of LDS the kernel may use (",
              TM_WAVES * TM_MAX_LINE, " of them hold the staged lines)");
  DeviceScope dev({{"lines", lines},
                   {"line_len", line_len},
                   {"fmt_bytes", fmt_bytes},
                   {"fmt_seg_off", fmt_seg_off},
                   {"seg_bytes", seg_bytes},
                   {"seg_off", seg_off},
                   {"tpl_seg_start", tpl_seg_start}});
  const int nf_seg = fmt_seg_off.numel() > 0 ? (int)fmt_seg_off.numel() - 1 : 0;
  const int n_tpl = (int)tpl_seg_start.numel() - 1;
  auto opts = lines.options().dtype(torch::kInt32);
  auto event_id = torch::empty({B}, opts);
  auto fmt_caps = torch::zeros({B, max_fmt_caps, 2}, opts);
  auto n_fmt_caps = torch::zeros({B}, opts);
  auto caps = torch::zeros({B, max_caps, 2}, opts);
  auto n_caps = torch::zeros({B}, opts);
  auto span_start = torch::empty({B}, opts);
  auto span_end = torch::empty({B}, opts);
  if (B > 0) {
    dmx_launch_template_match(
        lines.data_ptr<uint8_t>(), line_len.data_ptr<int32_t>(), (int)B,
        (int)max_len,
        fmt_bytes.numel() ? fmt_bytes.data_ptr<uint8_t>() : nullptr,
        fmt_seg_off.numel() ? fmt_seg_off.data_ptr<int32_t>() : nullptr,
        nf_seg, seg_bytes.data_ptr<uint8_t>(), (int)seg_bytes.numel(),
        seg_off.data_ptr<int32_t>(), tpl_seg_start.data_ptr<int32_t>(), n_tpl,
        lower ? 1 : 0, event_id.data_ptr<int32_t>(),
        fmt_caps.data_ptr<int32_t>(), n_fmt_caps.data_ptr<int32_t>(),
        caps.data_ptr<int32_t>(), n_caps.data_ptr<int32_t>(),
        span_start.data_ptr<int32_t>(), span_end.data_ptr<int32_t>(),
        (int)max_fmt_caps, (int)max_caps, dev.stream());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return {event_id, fmt_caps, n_fmt_caps, caps, n_caps, span_start, span_end};
}

torch::Tensor edit_distance(torch::Tensor A, torch::Tensor a_len,
                            torch::Tensor B, torch::Tensor b_len) {
  check_arg(A, "A", torch::kUInt8, 2);
  check_arg(B, "B", torch::kUInt8, 2);
  const auto Na = A.size(0), Nb = B.size(0), max_len = A.size(1);
  TORCH_CHECK(B.size(1) == max_len, "B must share A's max_len ", max_len,
              ", got ", B.size(1));
  TORCH_CHECK(max_len <= ED_MAX_LEN, "A: edit_distance supports max_len<=",
              ED_MAX_LEN, ", got ", max_len);
  check_arg(a_len, "a_len", torch::kInt32, 1);
  check_numel(a_len, "a_len", Na, "Na");
  check_arg(b_len, "b_len", torch::kInt32, 1);
  check_numel(b_len, "b_len", Nb, "Nb");
  DeviceScope dev({{"A", A}, {"a_len", a_len}, {"B", B}, {"b_len", b_len}});
  auto dist = torch::empty({Na, Nb}, A.options().dtype(torch::kInt32));
  if (Na == 0 || Nb == 0) return dist;
  dmx_launch_edit_distance(A.data_ptr<uint8_t>(), a_len.data_ptr<int32_t>(),
                           (int)Na, B.data_ptr<uint8_t>(),
                           b_len.data_ptr<int32_t>(), (int)Nb, (int)max_len,
                           dist.data_ptr<int32_t>(), dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dist;
}

// A [n, 4] int32 table of watch specs (kind, event, pos, pad).
void check_specs(const torch::Tensor& t, const char* name, const char* rows) {
  check_arg(t, name, torch::kInt32, 2);
  TORCH_CHECK(t.size(1) == 4, name, " must be int32 [", rows,
              ", 4] (kind, event, pos, pad), got ", t.sizes());
}

// The matcher's six tensors, as every field binding takes them: checked
// in this order, then viewed as the launchers' ParsedBatch.
ParsedBatch check_parsed_batch(const torch::Tensor& lines,
                               const torch::Tensor& event_id,
                               const torch::Tensor& caps,
                               const torch::Tensor& n_caps,
                               const torch::Tensor& fmt_caps,
                               const torch::Tensor& n_fmt_caps) {
  check_arg(lines, "lines", torch::kUInt8, 2);
  const auto B = lines.size(0);
  check_arg(event_id, "event_id", torch::kInt32, 1);
  check_numel(event_id, "event_id", B, "B");
  check_caps(caps, "caps", B);
  check_arg(n_caps, "n_caps", torch::kInt32, 1);
  check_numel(n_caps, "n_caps", B, "B");
  check_caps(fmt_caps, "fmt_caps", B);
  check_arg(n_fmt_caps, "n_fmt_caps", torch::kInt32, 1);
  check_numel(n_fmt_caps, "n_fmt_caps", B, "B");
  return {lines.data_ptr<uint8_t>(),     event_id.data_ptr<int32_t>(),
          caps.data_ptr<int32_t>(),      n_caps.data_ptr<int32_t>(),
          fmt_caps.data_ptr<int32_t>(),  n_fmt_caps.data_ptr<int32_t>(),
          (int)B,                        (int)lines.size(1),
          (int)caps.size(1),             (int)fmt_caps.size(1)};
}

// Device clause of the same six tensors, then of the binding's own (`more`).
DeviceScope parsed_batch_scope(const torch::Tensor& lines,
                               const torch::Tensor& event_id,
                               const torch::Tensor& caps,
                               const torch::Tensor& n_caps,
                               const torch::Tensor& fmt_caps,
                               const torch::Tensor& n_fmt_caps,
                               std::initializer_list<Arg> more) {
  return DeviceScope({{"lines", lines},
                      {"event_id", event_id},
                      {"caps", caps},
                      {"n_caps", n_caps},
                      {"fmt_caps", fmt_caps},
                      {"n_fmt_caps", n_fmt_caps}},
                     more);
}

torch::Tensor watch_hashes(torch::Tensor lines, torch::Tensor event_id,
                           torch::Tensor caps, torch::Tensor n_caps,
                           torch::Tensor fmt_caps, torch::Tensor n_fmt_caps,
                           torch::Tensor specs, bool lower) {
  const ParsedBatch batch =
      check_parsed_batch(lines, event_id, caps, n_caps, fmt_caps, n_fmt_caps);
  check_specs(specs, "specs", "W");
  const auto B = lines.size(0), W = specs.size(0);
  DeviceScope dev = parsed_batch_scope(lines, event_id, caps, n_caps, fmt_caps,
                                       n_fmt_caps, {{"specs", specs}});
  auto hashes = torch::zeros({B, W}, lines.options().dtype(torch::kInt64));
  if (B == 0 || W == 0) return hashes;
  dmx_launch_watch_hashes(batch, specs.data_ptr<int32_t>(), (int)W,
                          lower ? 1 : 0, hashes.data_ptr<int64_t>(),
                          dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return hashes;
}

// Watches and combinations in one launch: hashes [B, W + C]. The offsets'
// VALUES (start at 0, non-decreasing, no empty combination, end at M) are
// what ops.pack_combos guarantees before upload; this binding checks them
// only when combo_off is host-resident, where reading them is free, and
// never reads a device tensor. On device it checks what the shapes show
// (M >= C), and the kernel clamps each member range into [0, M].
torch::Tensor watch_combo_hashes(torch::Tensor lines, torch::Tensor event_id,
                                 torch::Tensor caps, torch::Tensor n_caps,
                                 torch::Tensor fmt_caps,
                                 torch::Tensor n_fmt_caps, torch::Tensor specs,
                                 torch::Tensor members,
                                 torch::Tensor combo_off, bool lower) {
  const ParsedBatch batch =
      check_parsed_batch(lines, event_id, caps, n_caps, fmt_caps, n_fmt_caps);
  check_specs(specs, "specs", "W");
  const auto B = lines.size(0), W = specs.size(0);
  check_specs(members, "members", "M");
  const auto M = members.size(0);
  check_arg(combo_off, "combo_off", torch::kInt32, 1);
  TORCH_CHECK(combo_off.numel() >= 1,
              "combo_off must hold at least one offset (C + 1 of them)");
  const auto C = combo_off.numel() - 1;
  TORCH_CHECK(M >= C, "combo_off: ", C, " combinations need at least ", C,
              " members (none may be empty), members has M = ", M);
  if (combo_off.is_cpu()) {
    const int32_t* off = combo_off.data_ptr<int32_t>();
    TORCH_CHECK(off[0] == 0, "combo_off must start at 0, got ", off[0]);
    for (int64_t c = 0; c < C; ++c)
      TORCH_CHECK(off[c + 1] > off[c], "combo_off: combination ", c,
                  " is empty or its offsets decrease (", off[c], " .. ",
                  off[c + 1], ")");
    TORCH_CHECK(off[C] == M, "combo_off must end at M = ", M,
                " (rows of members), got ", off[C]);
  }
  TORCH_CHECK(B * (W + C) < (int64_t(1) << 31), "lines: B * (W + C) = ", B,
              " * ", W + C, " must be below 2^31 (the kernel's flat index)");
  DeviceScope dev = parsed_batch_scope(
      lines, event_id, caps, n_caps, fmt_caps, n_fmt_caps,
      {{"specs", specs}, {"members", members}, {"combo_off", combo_off}});
  auto hashes = torch::zeros({B, W + C}, lines.options().dtype(torch::kInt64));
  if (B == 0 || W + C == 0) return hashes;
  dmx_launch_watch_combo_hashes(
      batch, specs.data_ptr<int32_t>(), (int)W, members.data_ptr<int32_t>(),
      (int)M, combo_off.data_ptr<int32_t>(), (int)C, lower ? 1 : 0,
      hashes.data_ptr<int64_t>(), dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return hashes;
}

// hashes [B, W] int64 against tables [W, capacity] int64
void check_hashset_args(const torch::Tensor& hashes,
                        const torch::Tensor& tables) {
  check_arg(hashes, "hashes", torch::kInt64, 2);
  check_arg(tables, "tables", torch::kInt64, 2);
  const auto W = hashes.size(1), cap = tables.size(1);
  TORCH_CHECK(tables.size(0) == W, "tables must be [W=", W,
              ", capacity] to match hashes [B, W], got ", tables.sizes());
  TORCH_CHECK(cap >= 1 && (cap & (cap - 1)) == 0,
              "tables: capacity must be a power of two, got ", cap);
}

void hashset_insert(torch::Tensor hashes, torch::Tensor tables) {
  check_hashset_args(hashes, tables);
  DeviceScope dev({{"hashes", hashes}, {"tables", tables}});
  const auto B = hashes.size(0), W = hashes.size(1);
  if (B == 0 || W == 0) return;
  dmx_launch_hashset_insert(hashes.data_ptr<int64_t>(),
                            tables.data_ptr<int64_t>(), (int)B, (int)W,
                            (int)tables.size(1), dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

torch::Tensor hashset_probe(torch::Tensor hashes, torch::Tensor tables) {
  check_hashset_args(hashes, tables);
  DeviceScope dev({{"hashes", hashes}, {"tables", tables}});
  const auto B = hashes.size(0), W = hashes.size(1);
  auto unseen = torch::zeros({B, W}, hashes.options().dtype(torch::kInt32));
  if (B == 0 || W == 0) return unseen;
  dmx_launch_hashset_probe(hashes.data_ptr<int64_t>(),
                           tables.data_ptr<int64_t>(), (int)B, (int)W,
                           (int)tables.size(1), unseen.data_ptr<int32_t>(),
                           dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return unseen;
}

// ---- event-rate windows (docs/kernels.md, "Event-rate windows") ---------------

py::dict event_rate_limits() {
  py::dict d;
  d["max_events"] = ER_MAX_EVENTS;
  d["max_cells"] = ER_MAX_CELLS;
  return d;
}

// One batch of the event-rate stage. The state tensors are updated in
// place; returns (rate_counts [NW, E], rate_z [NW, E], rate_hits [B],
// rate_slot [B]). n_valid, in_window and windows_seen stay on the device:
// nothing here reads a tensor's values.
std::vector<torch::Tensor> event_rate_step(
    torch::Tensor event_id, torch::Tensor n_valid, torch::Tensor mean,
    torch::Tensor var, torch::Tensor known, torch::Tensor open_counts,
    torch::Tensor ctl, int64_t train_upto, int64_t window_lines,
    double ewma_alpha, double z_threshold, int64_t min_windows) {
  check_arg(event_id, "event_id", torch::kInt32, 1);
  const auto B = event_id.size(0);
  check_arg(n_valid, "n_valid", torch::kInt32, 1);
  check_numel(n_valid, "n_valid", 1, "one count");
  check_arg(mean, "mean", torch::kFloat64, 1);
  const auto E = mean.size(0);
  TORCH_CHECK(E >= 1 && E <= ER_MAX_EVENTS, "mean: E = templates + 1 = ", E,
              " bins must be within 1 .. ER_MAX_EVENTS = ", ER_MAX_EVENTS);
  check_arg(var, "var", torch::kFloat64, 1);
  check_same_shape(var, "var", mean, "mean");
  check_arg(known, "known", torch::kInt32, 1);
  check_numel(known, "known", E, "E");
  check_arg(open_counts, "open_counts", torch::kInt32, 1);
  check_numel(open_counts, "open_counts", E, "E");
  check_arg(ctl, "ctl", torch::kInt32, 1);
  check_numel(ctl, "ctl", 2, "(in_window, windows_seen)");
  TORCH_CHECK(window_lines >= 1 && window_lines <= INT32_MAX,
              "window_lines must be within 1 .. 2^31 - 1, got ", window_lines);
  TORCH_CHECK(ewma_alpha > 0.0 && ewma_alpha <= 1.0,
              "ewma_alpha must be in (0, 1], got ", ewma_alpha);
  TORCH_CHECK(z_threshold >= 0.0, "z_threshold must be >= 0, got ",
              z_threshold);
  TORCH_CHECK(min_windows >= 0 && min_windows <= INT32_MAX,
              "min_windows must be within 0 .. 2^31 - 1, got ", min_windows);
  TORCH_CHECK(train_upto >= 0 && train_upto <= B,
              "train_upto must be within 0 .. B = ", B, ", got ", train_upto);
  TORCH_CHECK(B <= INT32_MAX, "event_id: B = ", B, " must be below 2^31");
  const int64_t NW = er_window_slots(B, window_lines);
  TORCH_CHECK(NW * E <= ER_MAX_CELLS, "event_id: NW * E = (B / window_lines",
              " + 2) * E = ", NW, " * ", E, " must not exceed ", ER_MAX_CELLS,
              " (raise window_lines or lower the batch)");
  DeviceScope dev({{"event_id", event_id},
                   {"n_valid", n_valid},
                   {"mean", mean},
                   {"var", var},
                   {"known", known},
                   {"open_counts", open_counts},
                   {"ctl", ctl}});
  const auto i32 = event_id.options();
  const auto f64 = event_id.options().dtype(torch::kFloat64);
  if (B == 0)
    return {torch::zeros({NW, E}, i32), torch::zeros({NW, E}, f64),
            torch::zeros({0}, i32), torch::zeros({0}, i32)};
  // every element of the four outputs is written by the two kernels
  auto rate_counts = torch::empty({NW, E}, i32);
  auto rate_z = torch::empty({NW, E}, f64);
  auto rate_hits = torch::empty({B}, i32);
  auto rate_slot = torch::empty({B}, i32);
  auto base = torch::empty({NW, E}, f64);  // scratch between the roll's passes
  dmx_launch_event_rate(
      event_id.data_ptr<int32_t>(), n_valid.data_ptr<int32_t>(), (int)B,
      (int)E, (int)window_lines, (int)train_upto, ewma_alpha, z_threshold,
      (int)min_windows, mean.data_ptr<double>(), var.data_ptr<double>(),
      known.data_ptr<int32_t>(), open_counts.data_ptr<int32_t>(),
      ctl.data_ptr<int32_t>(), base.data_ptr<double>(),
      rate_counts.data_ptr<int32_t>(),
      rate_z.data_ptr<double>(), rate_hits.data_ptr<int32_t>(),
      rate_slot.data_ptr<int32_t>(), dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {rate_counts, rate_z, rate_hits, rate_slot};
}

// ---- value ranges (docs/kernels.md, "Value ranges") ---------------------------

py::dict value_range_limits() {
  py::dict d;
  d["max_span"] = VR_MAX_SPAN;
  d["max_digits"] = VR_MAX_DIGITS;
  return d;
}

// One batch of the value-range stage. lo, hi and n are updated in place by
// the rows below train_upto; returns (range_code int32 [B, R], range_value
// f64 [B, R]). Nothing here reads a tensor's values.
std::vector<torch::Tensor> value_range_step(
    torch::Tensor lines, torch::Tensor event_id, torch::Tensor caps,
    torch::Tensor n_caps, torch::Tensor fmt_caps, torch::Tensor n_fmt_caps,
    torch::Tensor specs, torch::Tensor slack, torch::Tensor lo,
    torch::Tensor hi, torch::Tensor n, int64_t train_upto) {
  const ParsedBatch batch =
      check_parsed_batch(lines, event_id, caps, n_caps, fmt_caps, n_fmt_caps);
  check_specs(specs, "specs", "R");
  const auto B = lines.size(0), R = specs.size(0);
  TORCH_CHECK(R >= 1, "specs must hold at least one range, got ",
              specs.sizes());
  check_arg(slack, "slack", torch::kFloat64, 1);
  check_numel(slack, "slack", R, "R");
  check_arg(lo, "lo", torch::kFloat64, 1);
  check_numel(lo, "lo", R, "R");
  check_arg(hi, "hi", torch::kFloat64, 1);
  check_numel(hi, "hi", R, "R");
  check_arg(n, "n", torch::kInt64, 1);
  check_numel(n, "n", R, "R");
  TORCH_CHECK(train_upto >= 0 && train_upto <= B,
              "train_upto must be within 0 .. B = ", B, ", got ", train_upto);
  TORCH_CHECK(B * R < (int64_t(1) << 31), "lines: B * R = ", B, " * ", R,
              " must be below 2^31 (the kernel's flat index)");
  DeviceScope dev = parsed_batch_scope(
      lines, event_id, caps, n_caps, fmt_caps, n_fmt_caps,
      {{"specs", specs}, {"slack", slack}, {"lo", lo}, {"hi", hi}, {"n", n}});
  // every element of both outputs is written by the judge kernel
  auto range_code = torch::empty({B, R}, event_id.options());
  auto range_value =
      torch::empty({B, R}, event_id.options().dtype(torch::kFloat64));
  if (B == 0) return {range_code, range_value};
  dmx_launch_value_range(
      batch, specs.data_ptr<int32_t>(), (int)R, slack.data_ptr<double>(),
      lo.data_ptr<double>(), hi.data_ptr<double>(), n.data_ptr<int64_t>(),
      (int)train_upto, range_code.data_ptr<int32_t>(),
      range_value.data_ptr<double>(), dev.stream());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {range_code, range_value};
}

// ---- event sequences (docs/kernels.md, "Event sequences") ----------------------

py::dict event_sequence_limits() {
  py::dict d;
  d["max_len"] = SEQ_MAX_LEN;
  d["max_keys"] = SEQ_MAX_KEYS;
  d["max_events"] = SEQ_MAX_EVENTS;
  return d;
}

// One batch of the event-sequence stage. seq_key and seq_hist are updated in
// place; returns (seq_gram int64 [B], gram_hash int64 [B, 1]). The key field
// is (key_kind, key_event, key_pos) of a watch spec, key_kind < 0 = no key.
// The sort's scratch comes from torch's allocator, sized by rocPRIM's query
// call, which launches nothing. Nothing here reads a tensor's values.
std::vector<torch::Tensor> event_sequence_step(
    torch::Tensor lines, torch::Tensor event_id, torch::Tensor caps,
    torch::Tensor n_caps, torch::Tensor fmt_caps, torch::Tensor n_fmt_caps,
    int64_t key_kind, int64_t key_event, int64_t key_pos, bool lower,
    torch::Tensor n_valid, int64_t n_templates, torch::Tensor seq_key,
    torch::Tensor seq_hist, int64_t length) {
  const ParsedBatch batch =
      check_parsed_batch(lines, event_id, caps, n_caps, fmt_caps, n_fmt_caps);
  const auto B = lines.size(0);
  TORCH_CHECK(key_kind >= -1 && key_kind <= 1,
              "key_kind must be -1 (no key), 0 (variable) or 1 (header), got ",
              key_kind);
  TORCH_CHECK(key_kind < 0 || (key_pos >= 0 && key_pos <= INT32_MAX),
              "key_pos must be within 0 .. 2^31 - 1, got ", key_pos);
  TORCH_CHECK(key_event >= -1 && key_event <= INT32_MAX,
              "key_event must be within -1 .. 2^31 - 1, got ", key_event);
  check_arg(n_valid, "n_valid", torch::kInt32, 1);
  check_numel(n_valid, "n_valid", 1, "one count");
  TORCH_CHECK(n_templates >= 0 && n_templates <= SEQ_MAX_EVENTS,
              "n_templates must be within 0 .. SEQ_MAX_EVENTS = ",
              SEQ_MAX_EVENTS, " (a symbol is 16 bits), got ", n_templates);
  check_arg(seq_key, "seq_key", torch::kInt64, 1);
  const auto K = seq_key.size(0);
  TORCH_CHECK(K >= 1 && K <= SEQ_MAX_KEYS && (K & (K - 1)) == 0,
              "seq_key: K = max_keys must be a power of two within 1 .. ",
              "SEQ_MAX_KEYS = ", SEQ_MAX_KEYS, ", got ", K);
  check_arg(seq_hist, "seq_hist", torch::kInt64, 1);
  check_numel(seq_hist, "seq_hist", K, "K");
  TORCH_CHECK(length >= 2 && length <= SEQ_MAX_LEN,
              "length must be within 2 .. SEQ_MAX_LEN = ", SEQ_MAX_LEN,
              ", got ", length);
  TORCH_CHECK(B <= INT32_MAX, "lines: B = ", B, " must be below 2^31");
  DeviceScope dev = parsed_batch_scope(
      lines, event_id, caps, n_caps, fmt_caps, n_fmt_caps,
      {{"n_valid", n_valid}, {"seq_key", seq_key}, {"seq_hist", seq_hist}});
  const auto i64 = event_id.options().dtype(torch::kInt64);
  if (B == 0) return {torch::zeros({0}, i64), torch::zeros({0, 1}, i64)};
  size_t temp_bytes = 0;
  C10_HIP_CHECK(
      dmx_seq_sort_temp_bytes((int)B, (int)K, dev.stream(), &temp_bytes));
  // never empty: a null scratch pointer would turn the sort into a size query
  temp_bytes = std::max<size_t>(temp_bytes, 16);
  auto sort_temp = torch::empty({(int64_t)temp_bytes},
                                event_id.options().dtype(torch::kUInt8));
  auto kh = torch::empty({B}, i64);
  auto words = torch::empty({2, B}, i64);
  // every element of both outputs is written by the grams kernel
  auto seq_gram = torch::empty({B}, i64);
  auto gram_hash = torch::empty({B, 1}, i64);
  C10_HIP_CHECK(dmx_launch_event_sequence(
      batch, (int)key_kind, (int)key_event, (int)key_pos, lower ? 1 : 0,
      n_valid.data_ptr<int32_t>(), (int)n_templates, (int)K, (int)length,
      seq_key.data_ptr<int64_t>(), seq_hist.data_ptr<int64_t>(),
      kh.data_ptr<int64_t>(), words.data_ptr<int64_t>(), sort_temp.data_ptr(),
      temp_bytes, seq_gram.data_ptr<int64_t>(), gram_hash.data_ptr<int64_t>(),
      dev.stream()));
  return {seq_gram, gram_hash};
}

}  // namespace

void register_codec(py::module_& m);   // codec.cpp
void register_frame_reader(py::module_& m);  // frame_reader.cpp
void register_shm_ring(py::module_& m);      // shm_ring.cpp

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_codec(m);
  register_frame_reader(m);
  register_shm_ring(m);
  m.def("fused_linear_bf16", &fused_linear_bf16,
        "C = act(x @ wt^T + bias), bf16 MFMA (epilogue: 0 none, 1 gelu, 2 relu)");
  m.def("probe_mfma", &probe_mfma, "MFMA 16x16x32 bf16 layout probe");
  m.def("probe_mfma32", &probe_mfma32, "MFMA 32x32x16 bf16 layout probe");
  m.def("layernorm_bf16", &layernorm_bf16, "fused residual+LayerNorm bf16");
  m.def("attention_bf16", &attention_bf16, "fused short-seq MHA bf16");
  m.def("attention_qkv_bf16", &attention_qkv_bf16,
        "MFMA MHA reading fused QKV layout [B,S,3*H*Dh] -> [B,S,H*Dh]");
  m.def("bert_fused_bf16", &bert_fused_bf16,
        "whole-model BERT-tiny forward, one workgroup per line");
  m.def("bert_fused_embed", &bert_fused_embed,
        "fused BERT-tiny forward with the embedding / distance head",
        py::arg("lines"), py::arg("start"), py::arg("end"), py::arg("wb"),
        py::arg("fb"), py::arg("n_layers"), py::arg("eps"),
        py::arg("mu") = py::none(), py::arg("inv_var") = py::none(),
        py::arg("want_emb") = true);
  m.def("bert_fused_probe", &bert_fused_probe,
        "phase-masked probe variant of the fused BERT kernel");
  m.def("bert_fused_timed", &bert_fused_timed,
        "fused kernel with per-wave phase timestamps (diagnostic)");
  m.def("bert_fused_layout", &bert_fused_layout,
        "geometry, blob sizes and named offsets of the fused BERT kernel");
  m.def("template_match", &template_match, "batched wildcard template match");
  m.def("watch_hashes", &watch_hashes, "hash watched capture spans");
  m.def("watch_combo_hashes", &watch_combo_hashes,
        "hash watched capture spans and field combinations, [B, W + C]");
  m.def("hashset_insert", &hashset_insert, "insert hashes into GPU sets");
  m.def("hashset_probe", &hashset_probe, "probe hashes against GPU sets");
  m.def("event_rate_step", &event_rate_step,
        "event-rate windows: count one batch, roll the complete windows");
  m.def("event_rate_limits", &event_rate_limits,
        "limits of event_rate_step (max_events, max_cells)");
  m.def("value_range_step", &value_range_step,
        "value ranges: fit the training rows, judge every (line, range)");
  m.def("value_range_limits", &value_range_limits,
        "limits of the value-range grammar (max_span, max_digits)");
  m.def("event_sequence_step", &event_sequence_step,
        "event sequences: per-key n-grams of event ids and their hashes");
  m.def("event_sequence_limits", &event_sequence_limits,
        "limits of event_sequence_step (max_len, max_keys, max_events)");
  m.def("edit_distance", &edit_distance,
        "batched Levenshtein distances (wavefront DP in LDS)");
}
