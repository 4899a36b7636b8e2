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

#include "field_span.h"
#include "kernels.h"

// lo - slack * (hi - lo) and hi + slack * (hi - lo) must round like the CPU
// mirror's: every multiply, add and subtract below rounds on its own.
#pragma clang fp contract(off)

namespace {

constexpr int VR_THREADS = 256;
constexpr int VR_WAVES = VR_THREADS / 64;

struct Parsed {
  int present;  // the range is relevant for the line and the field is there
  int number;   // ... and the span matches the grammar
  double v;     // its value, 0 otherwise
};

// The decimal number in p[0 .. len), len >= 0: whether the bytes match the
// grammar, and the value into *v when they do.
//
// Grammar: [+-]?[0-9]+(\.[0-9]+)? over the whole span, at most VR_MAX_DIGITS
// digits, at most VR_MAX_SPAN bytes. Value: M / 10^k with M the integer of
// all digits and k the number of fraction digits. M < 10^15 < 2^53 and
// 10^k <= 10^14 are both exact in f64, so the one division is the correctly
// rounded value of the decimal string. -0 is never produced.
//
// Reads: an empty span and one longer than VR_MAX_SPAN are rejected before
// their first byte is loaded.
__device__ __forceinline__ int parse_decimal(const unsigned char* p, int len,
                                             double* v) {
  if (len == 0 || len > VR_MAX_SPAN) return 0;

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
    return 0;
  const double q = (double)M / (double)scale;
  *v = (negative && M != 0) ? -q : q;
  return 1;
}

// The field that spec `s` names on `line` (field_span.h), read as a number.
__device__ __forceinline__ Parsed vr_parse(const ParsedBatch& batch,
                                           const FieldSpec s, int line) {
  Parsed out = {0, 0, 0.0};
  const FieldSpan f = field_span(batch, s, line);
  if (f.len < 0) return out;
  out.present = 1;
  out.number = parse_decimal(
      batch.lines + (long)line * batch.max_len + f.start, f.len, &out.v);
  return out;
}

}  // namespace

// Block r folds the training rows of range r. Each thread keeps min, max and
// count of the rows it strides over; lanes combine by shuffles, the four
// waves through LDS, and thread 0 folds the block's result into the state
// with plain stores. No other block touches range r.
extern "C" __global__ __launch_bounds__(VR_THREADS)
void dmx_value_range_fit(
    const ParsedBatch batch, const FieldSpec* __restrict__ specs,
    int train_upto,                // <= B, checked by the binding
    double* __restrict__ lo,       // [R]
    double* __restrict__ hi,       // [R]
    long long* __restrict__ n) {   // [R]
  __shared__ double s_lo[VR_WAVES];
  __shared__ double s_hi[VR_WAVES];
  __shared__ int s_n[VR_WAVES];
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const FieldSpec s = specs[r];
  double t_lo = INFINITY, t_hi = -INFINITY;
  int t_n = 0;
  for (int line = tid; line < train_upto; line += VR_THREADS) {
    const Parsed f = vr_parse(batch, s, line);
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
    const ParsedBatch batch, const FieldSpec* __restrict__ specs, int R,
    const double* __restrict__ slack,  // [R]
    const double* __restrict__ lo,     // [R]
    const double* __restrict__ hi,     // [R]
    int train_upto,
    int* __restrict__ range_code,        // [B, R]
    double* __restrict__ range_value) {  // [B, R]
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)batch.B * R) return;
  const int idx = (int)gid;  // B * R < 2^31, checked by the binding
  const int line = idx / R;
  const int r = idx % R;
  const FieldSpec s = specs[r];
  const Parsed f = vr_parse(batch, s, line);
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
    ParsedBatch batch, const int32_t* specs, int R, const double* slack,
    double* lo, double* hi, int64_t* n, int train_upto, int32_t* range_code,
    double* range_value, hipStream_t stream) {
  if (train_upto > 0)
    hipLaunchKernelGGL(dmx_value_range_fit, dim3(R), dim3(VR_THREADS), 0,
                       stream, batch, (const FieldSpec*)specs, train_upto, lo,
                       hi, (long long*)n);
  const long total = (long)batch.B * R;
  const int grid = (int)((total + VR_THREADS - 1) / VR_THREADS);
  hipLaunchKernelGGL(dmx_value_range_judge, dim3(grid), dim3(VR_THREADS), 0,
                     stream, batch, (const FieldSpec*)specs, R, slack, lo, hi,
                     train_upto, range_code, range_value);
}
