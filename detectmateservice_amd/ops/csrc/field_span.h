// "The field that spec s names on line i" of a parsed batch: the one lookup
// behind the watch hashes, the combination hashes and the value ranges
// (docs/kernels.md, "Parsed batch and field span"; ops._field_span is its
// CPU mirror). Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"

// One row of a [n, 4] int32 spec table (ops.watch_spec_row, range_spec_row):
//   kind 0 = content variable: capture `pos` of the lines whose event_id is
//            `event` (event < 0: of every line)                [caps]
//   kind 1 = header variable: format capture `pos` of every line [fmt_caps]
struct FieldSpec {
  int kind;
  int event;
  int pos;
  int flags;  // watches: pad. ranges: bit 0 = a field that is no number alerts
};

// Whether spec `s` applies to a line of event `event`: a header variable
// always does, a content variable when it is scoped to no event or to this one.
static __device__ __forceinline__ int field_relevant(const FieldSpec s,
                                                     int event) {
  return s.kind != 0 || s.event < 0 || event == s.event;
}

struct FieldSpan {
  int start;  // byte offset into the line
  int len;    // < 0: the spec is not relevant for the line or the field is absent
};

// The span spec `s` names on `line`. Everything a hand-built batch could get
// wrong is decided here, before a caller loads a byte of the line: pos lies
// inside both the row's capture count and the table, the span inside the line.
static __device__ __forceinline__ FieldSpan field_span(const ParsedBatch& b,
                                                       const FieldSpec s,
                                                       int line) {
  const FieldSpan absent = {0, -1};
  if (!field_relevant(s, b.event_id[line]) || s.pos < 0) return absent;
  const bool header = s.kind != 0;
  const int32_t* table = header ? b.fmt_caps : b.caps;
  const int width = header ? b.max_fmt_caps : b.max_caps;
  const bool there = header ? s.pos < min(b.n_fmt_caps[line], width)
                            : s.pos < min(b.n_caps[line], width);
  if (!there) return absent;
  const int32_t* span = table + ((long)line * width + s.pos) * 2;
  const int start = span[0], end = span[1];
  if (start < 0 || end < start || end > b.max_len) return absent;
  const FieldSpan found = {start, end - start};
  return found;
}
