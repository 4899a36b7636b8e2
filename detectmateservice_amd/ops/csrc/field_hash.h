// The hash of a field of a parsed batch: FNV-1a-64 over the span's bytes,
// forced odd so that 0 stays "no value". One definition for the watch and
// combination hashes (hashset.hip) and the sequence key (event_sequence.hip);
// ops.fnv1a64 is its CPU mirror. Device code only.
#pragma once

#include "field_span.h"

constexpr unsigned long long FNV_OFFSET = 1469598103934665603ull;
constexpr unsigned long long FNV_PRIME = 1099511628211ull;

static __device__ __forceinline__ unsigned long long fnv1a64(
    const unsigned char* p, int n, int lower) {
  unsigned long long h = FNV_OFFSET;
  for (int i = 0; i < n; ++i) {
    unsigned char c = p[i];
    if (lower && c >= 'A' && c <= 'Z') c += 32;
    h ^= (unsigned long long)c;
    h *= FNV_PRIME;
  }
  return h | 1ull;  // never the empty key
}

// Hash of the span that spec `s` watches on `line`: 0 when the spec is not
// relevant for the line or the field is absent (field_span.h).
static __device__ __forceinline__ unsigned long long field_hash(
    const ParsedBatch& batch, const FieldSpec s, int line, int lower) {
  const FieldSpan f = field_span(batch, s, line);
  if (f.len < 0) return 0ull;
  return fnv1a64(batch.lines + (long)line * batch.max_len + f.start, f.len,
                 lower);
}
