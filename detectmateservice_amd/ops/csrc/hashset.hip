// GPU hash-set probe/insert for the NewValue detector family.
//
// The reference's NewValueDetector keeps per-watched-field Python sets
// (docs/getting_started.md:421-511). Here the known-value
// sets are open-addressing u64 hash tables resident in HBM; a batch of
// parsed lines is scored with one kernel launch: for each (line, watch)
// the watched capture span is located, FNV-1a-64 hashed from the line
// bytes, and probed (detect) or inserted (train).
//
// Tables: [W, capacity] u64, 0 = empty (hashes are forced odd). Linear
// probing; capacity is a power of two sized >= 4x expected cardinality.
#include "common.h"
#include "kernels.h"

#define EMPTY_KEY 0ull

static __device__ __forceinline__ unsigned long long fnv1a64(
    const unsigned char* p, int n, int lower) {
  unsigned long long h = 1469598103934665603ull;
  for (int i = 0; i < n; ++i) {
    unsigned char c = p[i];
    if (lower && c >= 'A' && c <= 'Z') c += 32;
    h ^= (unsigned long long)c;
    h *= 1099511628211ull;
  }
  return h | 1ull;  // never EMPTY_KEY
}

// Watch spec (mirrors library/detectors/new_value.py::_WatchSpec):
//   kind 0 = content variable: capture index `pos` of lines whose
//            event_id == event (event < 0 -> any event)  [caps table]
//   kind 1 = header variable: format capture index `pos`  [fmt_caps table]
struct WatchSpec {
  int kind;
  int event;
  int pos;
  int _pad;
};

// For each (line, watch): compute the hash of the watched span (0 if the
// field is absent for that line).
extern "C" __global__ __launch_bounds__(256)
void dmx_watch_hashes(
    const unsigned char* __restrict__ lines, int max_len,
    const int* __restrict__ event_id,
    const int* __restrict__ caps, const int* __restrict__ n_caps, int max_caps,
    const int* __restrict__ fmt_caps, const int* __restrict__ n_fmt_caps,
    int max_fmt_caps,
    const WatchSpec* __restrict__ specs, int W,
    int B, int lower,
    unsigned long long* __restrict__ hashes) {  // [B, W]
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * W) return;
  const int line = idx / W;
  const int w = idx % W;
  const WatchSpec s = specs[w];
  unsigned long long h = 0ull;

  int start = -1, end = -1;
  if (s.kind == 0) {
    if ((s.event < 0 || event_id[line] == s.event) && s.pos < n_caps[line]) {
      start = caps[((long)line * max_caps + s.pos) * 2];
      end = caps[((long)line * max_caps + s.pos) * 2 + 1];
    }
  } else {
    if (n_fmt_caps && s.pos < n_fmt_caps[line]) {
      start = fmt_caps[((long)line * max_fmt_caps + s.pos) * 2];
      end = fmt_caps[((long)line * max_fmt_caps + s.pos) * 2 + 1];
    }
  }
  if (start >= 0 && end >= start)
    h = fnv1a64(lines + (long)line * max_len + start, end - start, lower);
  hashes[idx] = h;
}

// Whether spec `s` applies to a line of event `event`: a header variable
// always does, a content variable when it is scoped to no event or to this one.
static __device__ __forceinline__ int watch_relevant(const WatchSpec s,
                                                     int event) {
  return s.kind != 0 || s.event < 0 || event == s.event;
}

// Hash of the span that spec `s` watches on `line`: 0 when the spec is not
// relevant for the line or the field is absent. The same lookup as in
// dmx_watch_hashes, which keeps its own copy: routed through this helper it
// compiles to two more scalar instructions, and the watches-only path is
// kept instruction for instruction what it was.
static __device__ __forceinline__ unsigned long long watch_span_hash(
    const WatchSpec s, int line,
    const unsigned char* __restrict__ lines, int max_len,
    const int* __restrict__ event_id,
    const int* __restrict__ caps, const int* __restrict__ n_caps, int max_caps,
    const int* __restrict__ fmt_caps, const int* __restrict__ n_fmt_caps,
    int max_fmt_caps, int lower) {
  unsigned long long h = 0ull;
  int start = -1, end = -1;
  if (s.kind == 0) {
    if ((s.event < 0 || event_id[line] == s.event) && s.pos < n_caps[line]) {
      start = caps[((long)line * max_caps + s.pos) * 2];
      end = caps[((long)line * max_caps + s.pos) * 2 + 1];
    }
  } else {
    if (n_fmt_caps && s.pos < n_fmt_caps[line]) {
      start = fmt_caps[((long)line * max_fmt_caps + s.pos) * 2];
      end = fmt_caps[((long)line * max_fmt_caps + s.pos) * 2 + 1];
    }
  }
  if (start >= 0 && end >= start)
    h = fnv1a64(lines + (long)line * max_len + start, end - start, lower);
  return h;
}

// Watches and combinations in one launch. For each (line, column) of
// [B, W + C]: columns < W are dmx_watch_hashes' columns; column W + c is
// the hash of combination c (docs/kernels.md, "Combination hash"): every
// member's relevance bit and the 8 bytes of its span hash, low byte first,
// folded FNV-1a style in member order and forced odd, or 0 when no member
// is relevant for the line. members [M, 4] holds WatchSpec rows, combo c
// owns rows combo_off[c] .. combo_off[c + 1]; the host guarantees offsets
// in [0, M] (ops.pack_combos), the clamp keeps a broken promise in bounds.
extern "C" __global__ __launch_bounds__(256)
void dmx_watch_combo_hashes(
    const unsigned char* __restrict__ lines, int max_len,
    const int* __restrict__ event_id,
    const int* __restrict__ caps, const int* __restrict__ n_caps, int max_caps,
    const int* __restrict__ fmt_caps, const int* __restrict__ n_fmt_caps,
    int max_fmt_caps,
    const WatchSpec* __restrict__ specs, int W,
    const WatchSpec* __restrict__ members, int M,
    const int* __restrict__ combo_off, int C,
    int B, int lower,
    unsigned long long* __restrict__ hashes) {  // [B, W + C]
  const int cols = W + C;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)B * cols) return;
  const int idx = (int)gid;
  const int line = idx / cols;
  const int col = idx % cols;
  if (col < W) {
    hashes[idx] = watch_span_hash(specs[col], line, lines, max_len, event_id,
                                  caps, n_caps, max_caps, fmt_caps, n_fmt_caps,
                                  max_fmt_caps, lower);
    return;
  }
  const int event = event_id[line];
  const int m0 = max(combo_off[col - W], 0);
  const int m1 = min(combo_off[col - W + 1], M);
  unsigned long long h = 1469598103934665603ull;
  int any = 0;
  for (int m = m0; m < m1; ++m) {
    const WatchSpec s = members[m];
    const int relevant = watch_relevant(s, event);
    unsigned long long mh = watch_span_hash(
        s, line, lines, max_len, event_id, caps, n_caps, max_caps, fmt_caps,
        n_fmt_caps, max_fmt_caps, lower);
    any |= relevant;
    h = (h ^ (unsigned long long)relevant) * 1099511628211ull;
    for (int b = 0; b < 8; ++b) {
      h = (h ^ (mh & 0xffull)) * 1099511628211ull;
      mh >>= 8;
    }
  }
  hashes[idx] = any ? (h | 1ull) : 0ull;
}

extern "C" __global__ __launch_bounds__(256)
void dmx_hashset_insert(
    const unsigned long long* __restrict__ hashes,  // [B, W]
    unsigned long long* __restrict__ tables,        // [W, capacity]
    int B, int W, int capacity) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * W) return;
  const unsigned long long h = hashes[idx];
  if (h == EMPTY_KEY) return;
  const int w = idx % W;
  unsigned long long* table = tables + (long)w * capacity;
  unsigned int slot = (unsigned int)(h >> 32 ^ h) & (capacity - 1);
  for (int probe = 0; probe < capacity; ++probe) {
    unsigned long long prev = atomicCAS(
        (unsigned long long*)&table[slot], EMPTY_KEY, h);
    if (prev == EMPTY_KEY || prev == h) return;
    slot = (slot + 1) & (capacity - 1);
  }
  // table full: drop (host sizes capacity with 4x headroom and monitors fill)
}

extern "C" __global__ __launch_bounds__(256)
void dmx_hashset_probe(
    const unsigned long long* __restrict__ hashes,  // [B, W]
    const unsigned long long* __restrict__ tables,  // [W, capacity]
    int B, int W, int capacity,
    int* __restrict__ unseen) {  // [B, W]: 1 = value present but never seen
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)B * W) return;
  const unsigned long long h = hashes[idx];
  int flag = 0;
  if (h != EMPTY_KEY) {
    const int w = idx % W;
    const unsigned long long* table = tables + (long)w * capacity;
    unsigned int slot = (unsigned int)(h >> 32 ^ h) & (capacity - 1);
    flag = 1;
    for (int probe = 0; probe < capacity; ++probe) {
      const unsigned long long v = table[slot];
      if (v == h) { flag = 0; break; }      // known
      if (v == EMPTY_KEY) break;            // definitely unseen
      slot = (slot + 1) & (capacity - 1);
    }
  }
  unseen[idx] = flag;
}

extern "C" void dmx_launch_watch_hashes(
    const uint8_t* lines, int max_len, const int32_t* event_id,
    const int32_t* caps, const int32_t* n_caps, int max_caps,
    const int32_t* fmt_caps, const int32_t* n_fmt_caps, int max_fmt_caps,
    const int32_t* specs, int W, int B, int lower, int64_t* hashes,
    hipStream_t stream) {
  const long total = (long)B * W;
  const int grid = (int)((total + 255) / 256);
  hipLaunchKernelGGL(dmx_watch_hashes, dim3(grid), dim3(256), 0, stream,
                     lines, max_len, event_id, caps, n_caps, max_caps,
                     fmt_caps, n_fmt_caps, max_fmt_caps,
                     (const WatchSpec*)specs, W, B, lower,
                     (unsigned long long*)hashes);
}

extern "C" void dmx_launch_watch_combo_hashes(
    const uint8_t* lines, int max_len, const int32_t* event_id,
    const int32_t* caps, const int32_t* n_caps, int max_caps,
    const int32_t* fmt_caps, const int32_t* n_fmt_caps, int max_fmt_caps,
    const int32_t* specs, int W, const int32_t* members, int M,
    const int32_t* combo_off, int C, int B, int lower, int64_t* hashes,
    hipStream_t stream) {
  const long total = (long)B * (W + C);
  const int grid = (int)((total + 255) / 256);
  hipLaunchKernelGGL(dmx_watch_combo_hashes, dim3(grid), dim3(256), 0, stream,
                     lines, max_len, event_id, caps, n_caps, max_caps,
                     fmt_caps, n_fmt_caps, max_fmt_caps,
                     (const WatchSpec*)specs, W, (const WatchSpec*)members, M,
                     combo_off, C, B, lower, (unsigned long long*)hashes);
}

extern "C" void dmx_launch_hashset_insert(
    const int64_t* hashes, int64_t* tables, int B, int W, int capacity,
    hipStream_t stream) {
  const long total = (long)B * W;
  const int grid = (int)((total + 255) / 256);
  hipLaunchKernelGGL(dmx_hashset_insert, dim3(grid), dim3(256), 0, stream,
                     (const unsigned long long*)hashes,
                     (unsigned long long*)tables, B, W, capacity);
}

extern "C" void dmx_launch_hashset_probe(
    const int64_t* hashes, const int64_t* tables, int B, int W, int capacity,
    int32_t* unseen, hipStream_t stream) {
  const long total = (long)B * W;
  const int grid = (int)((total + 255) / 256);
  hipLaunchKernelGGL(dmx_hashset_probe, dim3(grid), dim3(256), 0, stream,
                     (const unsigned long long*)hashes,
                     (const unsigned long long*)tables, B, W, capacity,
                     unseen);
}
