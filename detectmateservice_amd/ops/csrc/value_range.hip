// Numeric value ranges for MI355X (gfx950): a captured field is read as a
// decimal number straight from the line bytes, the smallest and largest
// value seen in training are kept per range on the device, and every later
// value is judged against them.
//
// docs/kernels.md, "Value ranges", is the definition; this file and
// ops.value_range_step_cpu are its two implementations.
//
//   dmx_value_range_fit    only with training rows in the batch: one block
//                          per range folds min / max / count of the rows
//                          below train_upto into lo, hi, n
//   dmx_value_range_judge  one thread per (line, range): span lookup, parse,
//                          compare against lo / hi / slack read from device
//                          memory, two stores. The steady state is this one
//                          launch.
// Nothing is read back by the host and min / max / integer count do not
// depend on the order of their operands, so the state after a batch is the
// same for every schedule and the stage is graph-capturable.
#include <hip/hip_runtime.h>

#include "kernels.h"

// lo - slack * (hi - lo) and hi + slack * (hi - lo) must round like the CPU
// mirror's: every multiply, add and subtract below rounds on its own.
#pragma clang fp contract(off)

namespace {

constexpr int VR_THREADS = 256;
constexpr int VR_WAVES = VR_THREADS / 64;

// WatchSpec's layout (hashset.hip) with the pad word used as flags.
struct RangeSpec {
  int kind;   // 0 = content variable (caps), 1 = header variable (fmt_caps)
  int event;  // kind 0 only: < 0 = any event
  int pos;
  int flags;  // bit 0: a present field that is not a number gets code 3
};

struct Parsed {
  int present;  // the range is relevant for the line and the field is there
  int number;   // ... and the span matches the grammar
  double v;     // its value, 0 otherwise
};

// The span lookup of dmx_watch_hashes (this file keeps its own copy, as the
// combination kernel does), then the decimal parse.
//
// Grammar: [+-]?[0-9]+(\.[0-9]+)? over the whole span, at most VR_MAX_DIGITS
// digits, at most VR_MAX_SPAN bytes. Value: M / 10^k with M the integer of
// all digits and k the number of fraction digits. M < 10^15 < 2^53 and
// 10^k <= 10^14 are both exact in f64, so the one division is the correctly
// rounded value of the decimal string. -0 is never produced.
//
// Reads: pos is checked against both the row's capture count and the table
// width, the span against [0, max_len], and a span longer than VR_MAX_SPAN
// is rejected before its first byte is loaded.
__device__ __forceinline__ Parsed vr_parse(
    const RangeSpec s, int line, const unsigned char* __restrict__ lines,
    int max_len, const int* __restrict__ event_id,
    const int* __restrict__ caps, const int* __restrict__ n_caps, int max_caps,
    const int* __restrict__ fmt_caps, const int* __restrict__ n_fmt_caps,
    int max_fmt_caps) {
  Parsed out;
  out.present = 0;
  out.number = 0;
  out.v = 0.0;
  int start = -1, end = -1;
  if (s.pos >= 0) {
    if (s.kind == 0) {
      if ((s.event < 0 || event_id[line] == s.event) &&
          s.pos < min(n_caps[line], max_caps)) {
        start = caps[((long)line * max_caps + s.pos) * 2];
        end = caps[((long)line * max_caps + s.pos) * 2 + 1];
      }
    } else {
      if (s.pos < min(n_fmt_caps[line], max_fmt_caps)) {
        start = fmt_caps[((long)line * max_fmt_caps + s.pos) * 2];
        end = fmt_caps[((long)line * max_fmt_caps + s.pos) * 2 + 1];
      }
    }
  }
  if (start < 0 || end < start || end > max_len) return out;
  out.present = 1;
  const int len = end - start;
  if (len == 0 || len > VR_MAX_SPAN) return out;

  const unsigned char* p = lines + (long)line * max_len + start;
  int i = 0, negative = 0;
  const unsigned char c0 = p[0];
  if (c0 == '+' || c0 == '-') {
    negative = c0 == '-';
    i = 1;
  }
  unsigned long long M = 0, scale = 1;  // <= 17 digits: below 2^64
  int n_int = 0, n_frac = 0, dot = 0, ok = 1;
  for (; i < len; ++i) {
    const unsigned char c = p[i];
    if (c >= '0' && c <= '9') {
      M = M * 10 + (unsigned long long)(c - '0');
      if (dot) {
        ++n_frac;
        scale *= 10;
      } else {
        ++n_int;
      }
    } else if (c == '.' && !dot && n_int > 0) {
      dot = 1;
    } else {
      ok = 0;
      break;
    }
  }
  if (!ok || n_int == 0 || (dot && n_frac == 0) ||
      n_int + n_frac > VR_MAX_DIGITS)
    return out;
  out.number = 1;
  const double v = (double)M / (double)scale;
  out.v = (negative && M != 0) ? -v : v;
  return out;
}

}  // namespace

// Block r folds the training rows of range r. Each thread keeps min, max and
// count of the rows it strides over; lanes combine by shuffles, the four
// waves through LDS, and thread 0 folds the block's result into the state
// with plain stores. No other block touches range r.
extern "C" __global__ __launch_bounds__(VR_THREADS)
void dmx_value_range_fit(
    const unsigned char* __restrict__ lines, int max_len,
    const int* __restrict__ event_id,
    const int* __restrict__ caps, const int* __restrict__ n_caps, int max_caps,
    const int* __restrict__ fmt_caps, const int* __restrict__ n_fmt_caps,
    int max_fmt_caps,
    const RangeSpec* __restrict__ specs,
    int train_upto,                // <= B, checked by the binding
    double* __restrict__ lo,       // [R]
    double* __restrict__ hi,       // [R]
    long long* __restrict__ n) {   // [R]
  __shared__ double s_lo[VR_WAVES];
  __shared__ double s_hi[VR_WAVES];
  __shared__ int s_n[VR_WAVES];
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const RangeSpec s = specs[r];
  double t_lo = INFINITY, t_hi = -INFINITY;
  int t_n = 0;
  for (int line = tid; line < train_upto; line += VR_THREADS) {
    const Parsed f = vr_parse(s, line, lines, max_len, event_id, caps, n_caps,
                              max_caps, fmt_caps, n_fmt_caps, max_fmt_caps);
    if (f.number) {
      t_lo = f.v < t_lo ? f.v : t_lo;
      t_hi = f.v > t_hi ? f.v : t_hi;
      ++t_n;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double o_lo = __shfl_down(t_lo, off);
    const double o_hi = __shfl_down(t_hi, off);
    t_n += __shfl_down(t_n, off);
    t_lo = o_lo < t_lo ? o_lo : t_lo;
    t_hi = o_hi > t_hi ? o_hi : t_hi;
  }
  if ((tid & 63) == 0) {
    s_lo[tid >> 6] = t_lo;
    s_hi[tid >> 6] = t_hi;
    s_n[tid >> 6] = t_n;
  }
  __syncthreads();
  if (tid == 0) {
    double b_lo = lo[r], b_hi = hi[r];
    long long b_n = n[r];
    for (int w = 0; w < VR_WAVES; ++w) {
      b_lo = s_lo[w] < b_lo ? s_lo[w] : b_lo;
      b_hi = s_hi[w] > b_hi ? s_hi[w] : b_hi;
      b_n += s_n[w];
    }
    lo[r] = b_lo;
    hi[r] = b_hi;
    n[r] = b_n;
  }
}

extern "C" __global__ __launch_bounds__(VR_THREADS)
void dmx_value_range_judge(
    const unsigned char* __restrict__ lines, int max_len,
    const int* __restrict__ event_id,
    const int* __restrict__ caps, const int* __restrict__ n_caps, int max_caps,
    const int* __restrict__ fmt_caps, const int* __restrict__ n_fmt_caps,
    int max_fmt_caps,
    const RangeSpec* __restrict__ specs, int R,
    const double* __restrict__ slack,  // [R]
    const double* __restrict__ lo,     // [R]
    const double* __restrict__ hi,     // [R]
    int B, int train_upto,
    int* __restrict__ range_code,        // [B, R]
    double* __restrict__ range_value) {  // [B, R]
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)B * R) return;
  const int idx = (int)gid;  // B * R < 2^31, checked by the binding
  const int line = idx / R;
  const int r = idx % R;
  const RangeSpec s = specs[r];
  const Parsed f = vr_parse(s, line, lines, max_len, event_id, caps, n_caps,
                            max_caps, fmt_caps, n_fmt_caps, max_fmt_caps);
  int code = 0;
  if (line >= train_upto && f.present) {
    if (!f.number) {
      code = (s.flags & 1) ? 3 : 0;
    } else {
      const double l = lo[r], h = hi[r];
      if (l <= h) {  // armed
        const double w = h - l;
        const double m = slack[r] * w;
        if (f.v < l - m)
          code = 1;
        else if (f.v > h + m)
          code = 2;
      }
    }
  }
  range_code[idx] = code;
  range_value[idx] = f.v;
}

extern "C" void dmx_launch_value_range(
    const uint8_t* lines, int max_len, const int32_t* event_id,
    const int32_t* caps, const int32_t* n_caps, int max_caps,
    const int32_t* fmt_caps, const int32_t* n_fmt_caps, int max_fmt_caps,
    const int32_t* specs, int R, const double* slack, double* lo, double* hi,
    int64_t* n, int B, int train_upto, int32_t* range_code,
    double* range_value, hipStream_t stream) {
  if (train_upto > 0)
    hipLaunchKernelGGL(dmx_value_range_fit, dim3(R), dim3(VR_THREADS), 0,
                       stream, lines, max_len, event_id, caps, n_caps,
                       max_caps, fmt_caps, n_fmt_caps, max_fmt_caps,
                       (const RangeSpec*)specs, train_upto, lo, hi,
                       (long long*)n);
  const long total = (long)B * R;
  const int grid = (int)((total + VR_THREADS - 1) / VR_THREADS);
  hipLaunchKernelGGL(dmx_value_range_judge, dim3(grid), dim3(VR_THREADS), 0,
                     stream, lines, max_len, event_id, caps, n_caps, max_caps,
                     fmt_caps, n_fmt_caps, max_fmt_caps,
                     (const RangeSpec*)specs, R, slack, lo, hi, B, train_upto,
                     range_code, range_value);
}
