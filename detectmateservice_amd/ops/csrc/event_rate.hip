// Event-rate windows for MI355X (gfx950): per-event line counts in fixed
// windows of L valid lines against an EWMA baseline, with the stream state
// (open window, baseline, window count) resident on the device.
//
// docs/kernels.md, "Event-rate windows", is the definition; this file and
// ops.event_rate_step_cpu are its two implementations.
//
// Two launches per batch, no host read of any device value:
//   dmx_event_rate_count  one block per window slot: LDS histogram of the
//                         slot's contiguous run of lines, stored as one row
//   dmx_event_rate_roll   ONE block: walks the complete slots in order and
//                         rolls each bin's baseline in f64, judges every
//                         (slot, bin) cell against the baseline before it,
//                         then stores the open slot and the control words
// in_window, windows_seen and n_valid are read on the device, so the stage
// is graph-capturable and a call with n_valid = 0 rewrites every state word
// with the value it already holds.
#include <hip/hip_runtime.h>

#include "kernels.h"

// mean and var must match the CPU mirror to the bit: every multiply and add
// below rounds on its own.
#pragma clang fp contract(off)

namespace {

constexpr int ER_THREADS = 256;

// What both kernels derive from the device-side control words. Everything
// is clamped into the range the indexing below relies on, so a corrupt ctl
// or n_valid gives wrong counts, never an access outside a table.
struct ErSpan {
  int n;  // valid lines of this batch, 0 .. B
  int p;  // lines already in the open window, 0 .. L - 1
};

__device__ __forceinline__ ErSpan er_span(const int* __restrict__ n_valid,
                                          const int* __restrict__ ctl, int B,
                                          int L) {
  ErSpan sp;
  sp.n = min(max(n_valid[0], 0), B);
  sp.p = min(max(ctl[0], 0), L - 1);
  return sp;
}

}  // namespace

// Slot s holds the lines i with (p + i) / L == s, i < n: the contiguous run
// [s*L - p, (s+1)*L - p) cut to [0, n). Its boundary line, if the run
// reaches it, is (s+1)*L - p - 1.
extern "C" __global__ __launch_bounds__(ER_THREADS)
void dmx_event_rate_count(
    const int* __restrict__ event_id,     // [B]
    const int* __restrict__ n_valid,      // [1]
    const int* __restrict__ ctl,          // [2] in_window, windows_seen
    const int* __restrict__ open_counts,  // [E]
    int B, int E, int L, int NW,
    int* __restrict__ rate_counts,  // [NW, E]
    int* __restrict__ rate_hits,    // [B]
    int* __restrict__ rate_slot) {  // [B]
  extern __shared__ int hist[];  // [E]
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const ErSpan sp = er_span(n_valid, ctl, B, L);
  // s <= B / L + 1, so s * L <= B + L: 64-bit, L may be close to 2^31
  const long long first = (long long)s * L - sp.p;
  const long long last = first + L - 1;  // the boundary line
  const int lo = (int)min(max(first, 0LL), (long long)sp.n);
  const int hi = (int)min(last + 1, (long long)sp.n);  // may be <= lo: empty

  for (int e = tid; e < E; e += ER_THREADS)
    hist[e] = (s == 0) ? open_counts[e] : 0;
  __syncthreads();

  for (int i = lo + tid; i < hi; i += ER_THREADS) {
    const int ev = event_id[i];
    // bin 0 = unparsed (ev < 0), bin ev for 1 .. E - 1; ev == 0 and
    // ev >= E count nowhere. This is the only index into hist.
    const int bin = ev < 0 ? 0 : ev;
    if (ev != 0 && bin < E) atomicAdd(&hist[bin], 1);
    rate_hits[i] = 0;  // the roll kernel adds onto boundary lines
    rate_slot[i] = (i == last) ? s : -1;
  }
  // rows past n_valid belong to no slot: the blocks share them
  for (long long i = (long long)sp.n + (long long)s * ER_THREADS + tid; i < B;
       i += (long long)NW * ER_THREADS) {
    rate_hits[i] = 0;
    rate_slot[i] = -1;
  }
  __syncthreads();

  int* row = rate_counts + (size_t)s * E;  // s < NW, NW * E <= ER_MAX_CELLS
  for (int e = tid; e < E; e += ER_THREADS) row[e] = hist[e];
}

// One block, two passes over the nc complete slots.
//
// Pass 1 is the part that is sequential in the windows, and only that: thread
// t owns bins t, t + 256, ..., loads a bin's baseline once, walks the windows
// in order with the baseline in registers (two multiplies and an add per
// value; the whole block stages the counts in LDS beforehand, so that no step
// waits for memory) and stores it once. For every window it leaves what the
// window is judged against, the baseline BEFORE it: mean in rate_z's cell,
// max(var, 1) in base's cell, 0 there for a bin that was not known yet.
// Pass 2 has no order: each (window, bin) cell on its own thread computes z
// (the square root and the division, which are most of the arithmetic), the
// flag and the cell's final rate_z, and a flagged cell adds 1 to its boundary
// line's rate_hits, which the counting kernel has set to 0: integer adds, so
// the sum does not depend on their order. At B = 65536, L = 1000 and 16 bins
// that is 66 short dependent steps on one wave instead of 66 long ones
// (measured: docs/kernels.md).
//
// ctl is read by every thread at the top and written by thread 0 after the
// last barrier; no other block exists that could read it in between.
extern "C" __global__ __launch_bounds__(ER_THREADS)
void dmx_event_rate_roll(
    const int* __restrict__ n_valid,      // [1]
    int* __restrict__ ctl,                // [2]
    const int* __restrict__ rate_counts,  // [NW, E]
    int B, int E, int L, int NW, int train_upto, double alpha,
    double z_threshold, int min_windows,
    double* __restrict__ mean,      // [E]
    double* __restrict__ var,       // [E]
    int* __restrict__ known,        // [E]
    int* __restrict__ open_counts,  // [E]
    double* __restrict__ base,      // [NW, E] scratch between the passes
    double* __restrict__ rate_z,    // [NW, E]
    int* __restrict__ rate_hits) {  // [B]
  __shared__ int cnt[ER_MAX_EVENTS];  // counts of a run of complete slots
  const int tid = threadIdx.x;
  const ErSpan sp = er_span(n_valid, ctl, B, L);
  const int windows_seen = ctl[1];
  const long long total = (long long)sp.p + sp.n;
  // complete windows; <= NW - 1 by construction of NW = B / L + 2
  const int nc = (int)min(total / L, (long long)NW - 1);
  const double one_minus_alpha = 1.0 - alpha;

  // pass 1, over runs of as many complete slots as fit the staged counts
  const int per = max(ER_MAX_EVENTS / E, 1);  // E <= ER_MAX_EVENTS: >= 1 slot
  for (int s0 = 0; s0 < nc; s0 += per) {
    const int ns = min(per, nc - s0);
    __syncthreads();  // the run before this one has been read
    const int* run = rate_counts + (size_t)s0 * E;
    for (int i = tid; i < ns * E; i += ER_THREADS) cnt[i] = run[i];
    __syncthreads();
    for (int e = tid; e < E; e += ER_THREADS) {
      double m = mean[e], v = var[e];  // this thread's own stores, if any
      int k = known[e];
      for (int j = 0; j < ns; ++j) {
        const size_t at = (size_t)(s0 + j) * E + e;  // s0 + j < nc <= NW - 1
        const double c = (double)cnt[j * E + e];
        rate_z[at] = m;
        base[at] = k ? fmax(v, 1.0) : 0.0;
        if (k) {
          const double d = c - m;
          m = alpha * c + one_minus_alpha * m;
          v = alpha * (d * d) + one_minus_alpha * v;
        } else if (c > 0.0) {
          k = 1;
          m = c;
          v = fmax(c, 1.0);
        }
      }
      mean[e] = m;
      var[e] = v;
      known[e] = k;
    }
  }
  __syncthreads();

  const size_t cells = (size_t)nc * E;
  for (size_t at = tid; at < cells; at += ER_THREADS) {
    const int s = (int)(at / E);
    // 0 .. n - 1, since (s + 1) * L <= nc * L <= p + n
    const long long boundary = (long long)(s + 1) * L - sp.p - 1;
    const bool report = boundary >= train_upto &&
                        (long long)windows_seen + s >= min_windows;
    const double var_floor = base[at];
    double z_out = 0.0;
    if (report && var_floor > 0.0) {
      const double z = ((double)rate_counts[at] - rate_z[at]) / sqrt(var_floor);
      if (fabs(z) > z_threshold) {
        z_out = z;
        atomicAdd(&rate_hits[boundary], 1);
      }
    }
    rate_z[at] = z_out;
  }

  // the open slot and the slots behind it flag nothing
  for (size_t k = (size_t)nc * E + tid; k < (size_t)NW * E; k += ER_THREADS)
    rate_z[k] = 0.0;
  const int* open_row = rate_counts + (size_t)nc * E;
  for (int e = tid; e < E; e += ER_THREADS) open_counts[e] = open_row[e];
  __syncthreads();
  if (tid == 0) {
    ctl[0] = (int)(total % L);
    ctl[1] = windows_seen + nc;
  }
}

extern "C" void dmx_launch_event_rate(
    const int32_t* event_id, const int32_t* n_valid, int B, int E,
    int window_lines, int train_upto, double ewma_alpha, double z_threshold,
    int min_windows, double* mean, double* var, int32_t* known,
    int32_t* open_counts, int32_t* ctl, double* base, int32_t* rate_counts,
    double* rate_z, int32_t* rate_hits, int32_t* rate_slot,
    hipStream_t stream) {
  const int NW = er_window_slots(B, window_lines);
  hipLaunchKernelGGL(dmx_event_rate_count, dim3(NW), dim3(ER_THREADS),
                     (size_t)E * sizeof(int), stream, event_id, n_valid, ctl,
                     open_counts, B, E, window_lines, NW, rate_counts,
                     rate_hits, rate_slot);
  hipLaunchKernelGGL(dmx_event_rate_roll, dim3(1), dim3(ER_THREADS), 0, stream,
                     n_valid, ctl, rate_counts, B, E, window_lines, NW,
                     train_upto, ewma_alpha, z_threshold, min_windows, mean,
                     var, known, open_counts, base, rate_z, rate_hits);
}
