// Event sequences for MI355X (gfx950): the n-gram of event ids that each line
// completes within its key's history (a session, a pid, or the whole stream),
// with the per-key history resident on the device in K buckets.
//
// docs/kernels.md, "Event sequences", is the definition: a sequential loop
// over the member rows. ops.event_sequence_step_cpu is that loop; this file
// evaluates it in parallel. Per batch, no atomics, no host read of a device
// value, nothing that depends on scheduling:
//   dmx_seq_keys    one thread per row: membership, key hash, and the sort
//                   word (bucket << 32 | row), bucket = K for a non-member
//   rocPRIM radix sort of the B words: rows grouped by bucket, in row order
//                   inside a bucket, the non-members last
//   dmx_seq_grams   one thread per sorted position: walks back over up to
//                   n - 1 earlier positions of its bucket with its key and
//                   takes what is still missing from the bucket's state
//   dmx_seq_commit  the last position of each bucket's run stores the new
//                   owner and history
// The state is read by dmx_seq_grams and written by dmx_seq_commit alone, so
// no thread reads a word that another thread of its launch writes. What the
// commit stores it takes from the outputs: the new owner is the row's key
// hash and the new history the low n - 1 symbols of the row's gram.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "field_hash.h"
#include "kernels.h"

namespace {

constexpr int SEQ_THREADS = 256;
using u64 = unsigned long long;

__device__ __forceinline__ u64 seq_mask(int symbols) {  // 1 .. 4 symbols
  return symbols >= 4 ? ~0ull : (1ull << (16 * symbols)) - 1ull;
}

// bits of the sort word in use: 32 of the row, log2(K) + 1 of the bucket
// (the value K itself marks a non-member)
int seq_sort_end_bit(int K) {
  int log2k = 0;
  while ((1 << log2k) < K) ++log2k;
  return 32 + log2k + 1;
}

}  // namespace

extern "C" __global__ __launch_bounds__(SEQ_THREADS)
void dmx_seq_keys(
    const ParsedBatch batch, const FieldSpec key, int has_key, int lower,
    const int* __restrict__ n_valid,  // [1]
    int T, int K,
    u64* __restrict__ kh,       // [B] key hash, 0 for a non-member
    u64* __restrict__ words) {  // [B] sort words
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch.B) return;
  const int n = min(max(n_valid[0], 0), batch.B);
  const int ev = batch.event_id[i];
  u64 h = 0ull;
  if (i < n && ev >= 1 && ev <= T)
    h = has_key ? field_hash(batch, key, i, lower) : 1ull;  // absent field: 0
  const u64 bucket =
      h ? (u64)((unsigned)(h >> 32 ^ h) & (unsigned)(K - 1)) : (u64)K;
  kh[i] = h;
  words[i] = bucket << 32 | (u64)(unsigned)i;
}

extern "C" __global__ __launch_bounds__(SEQ_THREADS)
void dmx_seq_grams(
    const u64* __restrict__ sorted,     // [B]
    const u64* __restrict__ kh,         // [B]
    const int* __restrict__ event_id,   // [B]
    const u64* __restrict__ seq_key,    // [K]
    const u64* __restrict__ seq_hist,   // [K]
    int B, int K, int length,
    u64* __restrict__ seq_gram,     // [B]
    u64* __restrict__ gram_hash) {  // [B]
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const u64 word = sorted[p];
  const unsigned row = (unsigned)word;
  const u64 bucket = word >> 32;
  if (row >= (unsigned)B) return;  // never for words dmx_seq_keys wrote
  if (bucket >= (u64)K) {          // non-member
    seq_gram[row] = 0ull;
    gram_hash[row] = 0ull;
    return;
  }
  const u64 mine = kh[row];
  u64 gram = (u64)(unsigned)event_id[row] & 0xffffull;
  int have = 1;
  bool taken_over = false;  // another key used the bucket before this row
  for (int q = p - 1; q >= 0 && have < length; --q) {
    const u64 w = sorted[q];
    if (w >> 32 != bucket) break;  // the start of the bucket's run
    const unsigned r = (unsigned)w;
    if (r >= (unsigned)B) break;
    if (kh[r] != mine) { taken_over = true; break; }
    gram |= ((u64)(unsigned)event_id[r] & 0xffffull) << (16 * have);
    ++have;
  }
  if (have < length && !taken_over && seq_key[bucket] == mine)
    gram |= seq_hist[bucket] << (16 * have);
  gram &= seq_mask(length);
  u64 h = FNV_OFFSET, g = gram;
  for (int b = 0; b < 8; ++b) {
    h = (h ^ (g & 0xffull)) * FNV_PRIME;
    g >>= 8;
  }
  seq_gram[row] = gram;
  gram_hash[row] = h | 1ull;
}

extern "C" __global__ __launch_bounds__(SEQ_THREADS)
void dmx_seq_commit(
    const u64* __restrict__ sorted,    // [B]
    const u64* __restrict__ kh,        // [B]
    const u64* __restrict__ seq_gram,  // [B]
    int B, int K, int length,
    u64* __restrict__ seq_key,     // [K]
    u64* __restrict__ seq_hist) {  // [K]
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= B) return;
  const u64 word = sorted[p];
  const unsigned row = (unsigned)word;
  const u64 bucket = word >> 32;
  if (bucket >= (u64)K || row >= (unsigned)B) return;
  if (p + 1 < B && sorted[p + 1] >> 32 == bucket) return;  // not the last
  seq_key[bucket] = kh[row];
  seq_hist[bucket] = seq_gram[row] & seq_mask(length - 1);
}

extern "C" hipError_t dmx_seq_sort_temp_bytes(int B, int K, hipStream_t stream,
                                              size_t* bytes) {
  *bytes = 0;
  const u64* none = nullptr;
  return rocprim::radix_sort_keys(nullptr, *bytes, none, (u64*)nullptr,
                                  (size_t)B, 0u, (unsigned)seq_sort_end_bit(K),
                                  stream);
}

extern "C" hipError_t dmx_launch_event_sequence(
    ParsedBatch batch, int key_kind, int key_event, int key_pos, int lower,
    const int32_t* n_valid, int T, int K, int length, int64_t* seq_key,
    int64_t* seq_hist, int64_t* kh, int64_t* words, void* sort_temp,
    size_t sort_temp_bytes, int64_t* seq_gram, int64_t* gram_hash,
    hipStream_t stream) {
  const int B = batch.B;
  const int grid = (B + SEQ_THREADS - 1) / SEQ_THREADS;
  const FieldSpec key = {key_kind < 0 ? 0 : key_kind, key_event, key_pos, 0};
  u64* unsorted = (u64*)words;
  u64* sorted = unsorted + B;
  hipLaunchKernelGGL(dmx_seq_keys, dim3(grid), dim3(SEQ_THREADS), 0, stream,
                     batch, key, key_kind >= 0 ? 1 : 0, lower, n_valid, T, K,
                     (u64*)kh, unsorted);
  const hipError_t err = rocprim::radix_sort_keys(
      sort_temp, sort_temp_bytes, (const u64*)unsorted, sorted, (size_t)B, 0u,
      (unsigned)seq_sort_end_bit(K), stream);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(dmx_seq_grams, dim3(grid), dim3(SEQ_THREADS), 0, stream,
                     (const u64*)sorted, (const u64*)kh, batch.event_id,
                     (const u64*)seq_key, (const u64*)seq_hist, B, K, length,
                     (u64*)seq_gram, (u64*)gram_hash);
  hipLaunchKernelGGL(dmx_seq_commit, dim3(grid), dim3(SEQ_THREADS), 0, stream,
                     (const u64*)sorted, (const u64*)kh,
                     (const u64*)seq_gram, B, K, length, (u64*)seq_key,
                     (u64*)seq_hist);
  return hipGetLastError();
}
