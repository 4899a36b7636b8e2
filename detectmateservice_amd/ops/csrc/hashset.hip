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
#include "field_hash.h"
#include "kernels.h"

#define EMPTY_KEY 0ull

// For each (line, watch): the hash of the watched span.
extern "C" __global__ __launch_bounds__(256)
void dmx_watch_hashes(
    const ParsedBatch batch, const FieldSpec* __restrict__ specs, int W,
    int lower, unsigned long long* __restrict__ hashes) {  // [B, W]
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)batch.B * W) return;
  hashes[idx] = field_hash(batch, specs[idx % W], idx / W, lower);
}

// Watches and combinations in one launch. For each (line, column) of
// [B, W + C]: columns < W are dmx_watch_hashes' columns; column W + c is
// the hash of combination c (docs/kernels.md, "Combination hash"): every
// member's relevance bit and the 8 bytes of its span hash, low byte first,
// folded FNV-1a style in member order and forced odd, or 0 when no member
// is relevant for the line. members [M, 4] holds FieldSpec rows, combo c
// owns rows combo_off[c] .. combo_off[c + 1]; the host guarantees offsets
// in [0, M] (ops.pack_combos), the clamp keeps a broken promise in bounds.
extern "C" __global__ __launch_bounds__(256)
void dmx_watch_combo_hashes(
    const ParsedBatch batch, const FieldSpec* __restrict__ specs, int W,
    const FieldSpec* __restrict__ members, int M,
    const int* __restrict__ combo_off, int C, int lower,
    unsigned long long* __restrict__ hashes) {  // [B, W + C]
  const int cols = W + C;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)batch.B * cols) return;
  const int idx = (int)gid;
  const int line = idx / cols;
  const int col = idx % cols;
  if (col < W) {
    hashes[idx] = field_hash(batch, specs[col], line, lower);
    return;
  }
  const int event = batch.event_id[line];
  const int m0 = max(combo_off[col - W], 0);
  const int m1 = min(combo_off[col - W + 1], M);
  unsigned long long h = 1469598103934665603ull;
  int any = 0;
  for (int m = m0; m < m1; ++m) {
    const FieldSpec s = members[m];
    const int relevant = field_relevant(s, event);
    unsigned long long mh = field_hash(batch, s, line, lower);
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
  // table full: the value is dropped. Nothing watches the fill; the capacity
  // comes from the configuration (hashset_capacity), sized for >= 4x the
  // expected cardinality. A dropped value keeps probing as unseen.
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
    ParsedBatch batch, const int32_t* specs, int W, int lower, int64_t* hashes,
    hipStream_t stream) {
  const long total = (long)batch.B * W;
  const int grid = (int)((total + 255) / 256);
  hipLaunchKernelGGL(dmx_watch_hashes, dim3(grid), dim3(256), 0, stream, batch,
                     (const FieldSpec*)specs, W, lower,
                     (unsigned long long*)hashes);
}

extern "C" void dmx_launch_watch_combo_hashes(
    ParsedBatch batch, const int32_t* specs, int W, const int32_t* members,
    int M, const int32_t* combo_off, int C, int lower, int64_t* hashes,
    hipStream_t stream) {
  const long total = (long)batch.B * (W + C);
  const int grid = (int)((total + 255) / 256);
  hipLaunchKernelGGL(dmx_watch_combo_hashes, dim3(grid), dim3(256), 0, stream,
                     batch, (const FieldSpec*)specs, W,
                     (const FieldSpec*)members, M, combo_off, C, lower,
                     (unsigned long long*)hashes);
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
