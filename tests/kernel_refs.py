"""Plain references and hostile inputs for the template match, hash set and
edit distance kernels. Nothing here imports a reference from
``detectmateservice_amd.ops``: the ``ops`` mirrors are implementations under
test, this module is the oracle.

* ``ref_match`` is the greedy-anchored wildcard match on ``bytes``, built on
  ``bytes.find`` (docs/kernels.md, "dmx_template_match").
* ``make_corpus`` is a seeded generator of lines at the lengths and offsets
  where the kernel takes another path, with a coverage guard that keeps a
  later edit from emptying the tests.
* ``levenshtein`` is the two-row DP.
* ``home_slot`` / ``keys_with_home`` serve the hash-set tests.
"""
from __future__ import annotations

import functools
import random
import re
from collections import Counter
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

#: candidate start positions one search step of the kernel covers (one wave)
STEP = 64

ASCII_ALPHABET = b"abcdxqzABCD =h"
BYTES_ALPHABET = ASCII_ALPHABET + bytes([0xC3, 0xA9, 0xFF, 0x00, 0x80])
ALPHABETS = {"ascii": ASCII_ALPHABET, "bytes": BYTES_ALPHABET}

LOG_FORMAT = "h=<Hd> <Content>"

#: A-Z -> a-z, every other byte unchanged
FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


# ---------------------------------------------------------------------------
# bytes reference of the matcher
# ---------------------------------------------------------------------------


def split_template(template: str) -> List[bytes]:
    return [s.encode("utf-8") for s in template.split("<*>")]


def format_segments(log_format: Optional[str]) -> Optional[List[bytes]]:
    if not log_format:
        return None
    return split_template(re.sub(r"<[A-Za-z_][A-Za-z0-9_]*>", "<*>", log_format))


def ref_segments(text: bytes, start: int, end: int, segs: Sequence[bytes],
                 finds: Optional[List[int]] = None,
                 partial: Optional[List[int]] = None):
    """Greedy-anchored match of ``segs`` on text[start:end]: the list of
    (start, end) capture spans, or None. An empty segment is skipped unless
    it is the last one, which captures [pos, end); segment 0, when not
    empty, must sit at ``start``; after the last segment pos == end.
    ``finds`` collects, per successful find, how far behind the search
    position the segment was found; ``partial`` collects, per failed match,
    how many captures it had filled before it failed."""
    spans = _ref_segments(text, start, end, segs, finds)
    if spans[1]:
        return spans[0]
    if partial is not None:
        partial.append(len(spans[0]))
    return None


def _ref_segments(text, start, end, segs, finds):
    pos, spans, n = start, [], len(segs)
    for i, seg in enumerate(segs):
        if not seg:
            if i == n - 1:
                spans.append((pos, end))
                return spans, True
            continue
        idx = text.find(seg, pos, end)
        if idx < 0:
            return spans, False
        if finds is not None:
            finds.append(idx - pos)
        if i == 0 and idx != start:
            return spans, False
        if i > 0:
            spans.append((pos, idx))
        pos = idx + len(seg)
    return spans, pos == end


class RefRow(NamedTuple):
    event_id: int                      # 1-based winner or -1
    caps: List[Tuple[int, int]]        # all captures of the winner, uncut
    fmt_caps: List[Tuple[int, int]]    # all header captures, uncut
    span_start: int
    span_end: int
    later_step: bool                   # a find beyond the first 64 candidates
    stale_caps: bool                   # a failed template filled more captures


def ref_match(row: bytes, line_len: int, max_len: int,
              fmt_segs: Optional[Sequence[bytes]],
              tpl_segs: Sequence[Sequence[bytes]], lowercase: bool) -> RefRow:
    """What the matcher owes for one stored row: the line is the row's first
    min(line_len, max_len) bytes; the format match never folds, the content
    match folds A-Z when ``lowercase``; the content span is the last header
    capture when the format matched, else the whole line."""
    text = row[: min(line_len, max_len)]
    start, end = 0, len(text)
    finds: List[int] = []
    partial: List[int] = []
    fmt_caps: List[Tuple[int, int]] = []
    if fmt_segs:
        spans = ref_segments(text, 0, len(text), fmt_segs, finds)
        if spans:
            fmt_caps = spans
            start, end = spans[-1]
    folded = text.translate(FOLD) if lowercase else text
    event_id, caps = -1, []
    for t, segs in enumerate(tpl_segs):
        spans = ref_segments(folded, start, end, segs, finds, partial)
        if spans is not None:
            event_id, caps = t + 1, spans
            break
    return RefRow(event_id, caps, fmt_caps, start, end,
                  any(d >= STEP for d in finds),
                  event_id > 0 and any(p >= 2 and p > len(caps) for p in partial))


# ---------------------------------------------------------------------------
# corpus
# ---------------------------------------------------------------------------

LIT70 = "q=" + "abcdx" * 13 + "zzz"            # one 70-byte segment
assert len(LIT70) == 70


def template_set(max_len: int, alphabet: str, catch_all: bool = False) -> List[str]:
    """The templates of a corpus. Order matters: the first match wins."""
    tpls = [
        "abq dx",                  # literal only
        "ab=<*> cd=<*>",           # lit <*> lit <*>
        "dz<*>a=<*>b=<*>zd",       # three captures; often finds dz, a=, b= and fails
        "dz<*>",                   # ... and then this one matches with one capture
        "xqx<*> zz <*>xqx",        # lit <*> lit <*> lit, same literal first and last
        "ba<*>abcabcabd<*>",       # a segment that overlaps itself
        "AB<*>cd",                 # upper case: never matches when lines are folded
        "<*><*>dq=",               # adjacent wildcards, literal flush at the end
    ]
    if max_len >= 100:
        tpls.append("cc<*>" + LIT70 + "<*>")   # longer than a wave's 64 lanes
    if alphabet == "bytes":
        tpls.append("c\u00e9=<*>")             # a literal that is not ASCII
    tpls.append("<*>qz=<*>")       # <*> lit <*>
    if catch_all:
        tpls.append("<*>")
    return tpls


def line_lengths(max_len: int) -> List[int]:
    """{0, 1, 2, 63..65, 127..129, 191..193, 255..257, max_len - 2 ..
    max_len} as far as max_len allows, and max_len + 88 (stored cut)."""
    cand = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257,
            max_len - 2, max_len - 1, max_len]
    return sorted({n for n in cand if 0 <= n <= max_len}) + [max_len + 88]


#: bytes between the search position and a planted segment
GAPS = (62, 63, 64, 65, 126, 127, 128, 129)


class Corpus(NamedTuple):
    rows: List[bytes]          # each exactly max_len bytes: line, then junk
    line_len: List[int]        # uncut lengths; some exceed max_len
    max_len: int
    templates: List[str]
    log_format: Optional[str]
    lowercase: bool
    ref: List[RefRow]
    counts: Dict[str, object]

    def lines_tensor(self) -> torch.Tensor:
        buf = torch.frombuffer(bytearray(b"".join(self.rows)), dtype=torch.uint8)
        return buf.view(len(self.rows), self.max_len).clone()

    def len_tensor(self) -> torch.Tensor:
        return torch.tensor(self.line_len, dtype=torch.int32)


def _fill(rng: random.Random, alphabet: bytes, n: int, avoid: bytes = b"") -> bytes:
    pool = bytes(c for c in alphabet if c not in avoid)
    return bytes(rng.choice(pool) for _ in range(max(n, 0)))


def _instantiate(rng, alphabet, template: str, want: int) -> bytes:
    """Content of about ``want`` bytes that follows ``template``: wildcards
    but the last get a planted gap (or a short one), the last takes the rest,
    so a trailing literal sits flush against the end."""
    segs = split_template(template)
    free = want - sum(len(s) for s in segs)
    holes = len(segs) - 1
    if holes == 0 or free < 0:
        return b"".join(segs)
    sizes = []
    for _ in range(holes - 1):
        fits = [g for g in GAPS if g <= free]
        g = rng.choice(fits) if fits and rng.random() < 0.6 else rng.randint(0, min(free, 5))
        sizes.append(g)
        free -= g
    # a template that ends in <*>: sometimes leave that capture empty, so
    # that its last literal ends the line
    sizes.append(0 if (not segs[-1] and rng.random() < 0.25) else free)
    if not segs[0] and len(sizes) > 1 and rng.random() < 0.5:
        sizes[0], sizes[-1] = sizes[-1], sizes[0]
    out = bytearray()
    for i, seg in enumerate(segs):
        out += seg
        if i < holes:
            out += _fill(rng, alphabet, sizes[i])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def make_corpus(seed: int, alphabet: str, max_len: int, with_format: bool,
                lowercase: bool, catch_all: bool = False, n_lines: int = 257,
                small_max_caps: Optional[int] = None) -> Corpus:
    """Deterministic corpus of ``n_lines`` stored rows. Treat the result as
    read-only: it is cached and shared between tests."""
    rng = random.Random(seed)
    alpha = ALPHABETS[alphabet]
    templates = template_set(max_len, alphabet, catch_all)
    log_format = LOG_FORMAT if with_format else None
    lengths = line_lengths(max_len)
    plans = list(range(len(templates))) + ["noise", "damaged", "stale"]
    rows, lens = [], []
    for i in range(n_lines):
        want = rng.choices(lengths, weights=[1 if n <= 2 else 4 for n in lengths])[0]
        plan = plans[i % len(plans)]
        header = b""
        if with_format:
            header = b"h=" + _fill(rng, alpha, rng.randint(0, 6), avoid=b" ") + b" "
            if rng.random() < 0.12:      # format miss: no "h=" at the start
                header = header[1:]
        room = max(want - len(header), 0)
        if plan == "noise":
            content = _fill(rng, alpha, room)
        elif plan == "stale":
            # "dz<*>a=<*>b=<*>zd" fills two captures here and fails on its
            # last segment; "dz<*>" then wins with one
            content = _instantiate(rng, alpha, "dz<*>a=<*>b=<*>", room).replace(b"zd", b"zq")
        else:
            t = plan if plan != "damaged" else rng.randrange(len(templates))
            content = _instantiate(rng, alpha, templates[t], room)
            if plan == "damaged" and content:
                k = rng.randrange(len(content))
                content = content[:k] + b"Z" + content[k + 1:]
            elif content and rng.random() < 0.25:
                # one letter in upper case: matches only when lines are folded
                k = rng.randrange(len(content))
                content = content[:k] + content[k:k + 1].upper() + content[k + 1:]
        line = header + content
        if want <= 2:
            line = line[:want]
        if want > max_len and len(line) <= max_len:
            line += _fill(rng, alpha, want - len(line))
        # the stored row: the line cut to max_len, then junk drawn from the
        # alphabet where a matcher that read past the length would find text
        row = line[:max_len] + _fill(rng, alpha, max_len - len(line))
        rows.append(row)
        lens.append(len(line))
    fmt_segs = format_segments(log_format)
    tpl_segs = [split_template(t) for t in templates]
    ref = [ref_match(r, n, max_len, fmt_segs, tpl_segs, lowercase)
           for r, n in zip(rows, lens)]
    counts = coverage_guard(ref, lens, templates, max_len, with_format,
                            lowercase, catch_all, small_max_caps)
    counts["seed"] = seed
    return Corpus(rows, lens, max_len, templates, log_format, lowercase, ref, counts)


def coverage_guard(ref, lens, templates, max_len, with_format, lowercase,
                   catch_all, small_max_caps) -> Dict[str, object]:
    """Conditions on a corpus, decided by the reference alone. They are not
    measurements of the code under test.

    * Every template wins on >= 2 lines. A template with an upper-case
      letter cannot match folded lines, so under ``lowercase`` it wins on
      none, and that is asserted instead.
    * >= 5% of the lines are unmatched. A catch-all ``<*>`` matches every
      line, so with one the condition is that the catch-all itself, i.e. no
      other template, wins on >= 5%.
    * With a format, >= 5% of the lines miss it.
    * >= 10 lines have a segment found in the second or a later 64-candidate
      step. This needs a find at 64 or more bytes behind the search position
      and a segment behind it, so it is asked only where max_len > 64 allows.
    * >= 3 lines have more captures than ``small_max_caps``, where given.
    * >= 2 lines are won by a template after an earlier one had filled two
      or more captures, more than the winner has, and then failed.
    * >= 1 row carries a length word above max_len.
    """
    n = len(ref)
    wins = Counter(r.event_id for r in ref)
    for t, tpl in enumerate(templates):
        if lowercase and tpl != tpl.lower():
            assert wins[t + 1] == 0, (tpl, wins[t + 1])
        else:
            assert wins[t + 1] >= 2, (tpl, wins[t + 1], dict(wins))
    unmatched = wins[len(templates)] if catch_all else wins[-1]
    assert unmatched * 20 >= n, ("unmatched / catch-all", unmatched, n)
    if catch_all:
        assert wins[-1] == 0
    fmt_miss = sum(1 for r in ref if not r.fmt_caps)
    if with_format:
        assert fmt_miss * 20 >= n, ("format misses", fmt_miss, n)
    later = sum(1 for r in ref if r.later_step)
    if max_len > STEP:
        assert later >= 10, ("later-step finds", later)
    overflow = None
    if small_max_caps is not None:
        overflow = sum(1 for r in ref if len(r.caps) > small_max_caps)
        assert overflow >= 3, ("capture overflows", overflow)
    stale = sum(1 for r in ref if r.stale_caps)
    assert stale >= 2, ("wins over stale captures", stale)
    overlong = sum(1 for x in lens if x > max_len)
    assert overlong >= 1
    return {"winners": [wins[t + 1] for t in range(len(templates))],
            "unmatched": wins[-1], "format_misses": fmt_miss,
            "later_step": later, "cap_overflows": overflow, "stale_caps": stale,
            "overlong": overlong, "lines": n}


#: The seed of every corpus the tests use, chosen so that the reference alone
#: meets the guard for all 48 combinations of alphabet, max_len, format, fold
#: and catch-all. ``Corpus.counts`` holds the figures; for the corpora of the
#: tests, 257 lines each, they are (winners per template in template order |
#: unmatched, format misses, later-step finds, capture overflows at max_caps
#: = 2, wins over stale captures, over-long length words):
#:
#: ascii 512 fmt exact -   | 13 20 10 33 16 16 12 21 17 24          |  75  41 137 10 26 15
#: bytes 512 fmt lower -   | 15 18 10 45 15 15  0 14 13 19 22       |  71  34 143 10 30 16
#: bytes 512 -   exact -   | 12 19  8 45 19 18 14 18 16 18 16       |  54   - 129  8 29 18
#: ascii 512 -   lower -   | 19 20  6 59 21 22  0 17 20 23          |  50   - 132  6 46 15
#: ascii 100 fmt lower -   | 13 17 10 32 13 15  0 15 13 23          | 106  70  51 10 17 30
#: ascii 100 -   exact -   | 12 17 12 46 18 18  5 18 17 19          |  75   -  58 12 24 27
#: bytes 100 fmt exact -   | 14 13 12 36 14 13  8 17 10 15 18       |  87  47  53 12 18 32
#: bytes 100 -   lower -   | 13 16 11 44 17 19  0 17 12 16 17       |  75   -  50 11 23 38
#: ascii  64 fmt exact -   |  6  9 12 34 12 18  6 14 17             | 129  74   0 12 15 52
#: bytes  64 -   lower -   |  8 17 12 48 17 19  0 10 19 16          |  91   -   0 12 19 55
#: bytes  64 fmt lower -   | 12 12  9 37 13 15  0 15 16 19          | 109  75   0  9 17 48
#: ascii  64 -   exact -   | 10 13 16 46 15 14  9 13 15             | 106   -   0 16 22 64
#: ascii 512 fmt exact all | 15 19 10 43 16 16  4 17 13 26 78       |   0  46 134 10 31 24
#: bytes 100 -   lower all | 15 15 11 43 13 14  0 15 12 17 17 85    |   0   -  44 11 22 31
#: bytes 512 fmt exact -   | 15 17 12 39 15 15 10 15 12 19 21       |  67  34 137 12 24 16
#: bytes 512 -   lower -   | 15 19  4 52 19 18  0 18 18 18 18       |  58   - 133  4 36 18
#: ascii 512 fmt lower -   | 18 20  8 37 16 17  0 19 22 25          |  75  41 134  8 31 15
#: ascii 512 -   exact -   | 16 20 12 50 21 22  8 19 18 21          |  50   - 136 12 31 15
#: bytes 100 fmt lower -   | 15 13 12 36 14 14  0 17 12 15 19       |  90  47  60 12 19 32
#: ascii 100 fmt exact -   | 10 17 13 29 12 12  7 15 12 21          | 109  70  49 13 12 30
#: ascii 100 -   lower -   | 16 17 11 48 18 19  0 17 18 19          |  74   -  48 11 31 27
#: bytes 100 -   exact -   |  7 15 14 40 17 18 15 17  9 15 17       |  73   -  49 14 20 38
#: ascii  64 fmt lower all | 10 17  9 39 13 15  0 12 16 126         |   0  61   0  9 19 43
#: ascii  64 -   exact all | 10 17  8 49 14 14  9 16 14 106         |   0   -   0  8 16 55
#: bytes  64 fmt lower all |  9 11  6 34 12 14  0 11 13 13 134      |   0  73   0  6 21 55
#: bytes  64 -   exact all |  9 18  7 44 14 17  7  8 15 13 105      |   0   -   0  7 16 73
#: bytes 512 fmt exact all | 13 17  7 40 11 12  5 16 13 14 15 94    |   0  43 129  7 28 11
#:
#: The 0 among the winners under "lower" is the upper-case template; the last
#: winner under "all" is the catch-all. Rows of 64 bytes cannot hold a find 64
#: bytes behind the search position, hence no later-step finds there.
SEED = 20


def expect_match(out: Dict[str, torch.Tensor], ref: Sequence[RefRow],
                 max_caps: int, max_fmt_caps: int, what: str = "") -> None:
    """Exact comparison of a matcher's seven outputs with the reference:
    event_id, the uncut counts, the first min(n, width) spans of each table,
    and the content span."""
    B = len(ref)
    got = {k: v.cpu() for k, v in out.items()}
    assert tuple(got["caps"].shape) == (B, max_caps, 2), got["caps"].shape
    assert tuple(got["fmt_caps"].shape) == (B, max_fmt_caps, 2), got["fmt_caps"].shape
    assert got["event_id"].tolist() == [r.event_id for r in ref], what
    assert got["n_caps"].tolist() == [len(r.caps) for r in ref], what
    assert got["n_fmt_caps"].tolist() == [len(r.fmt_caps) for r in ref], what
    assert got["span_start"].tolist() == [r.span_start for r in ref], what
    assert got["span_end"].tolist() == [r.span_end for r in ref], what
    caps, fmt_caps = got["caps"].tolist(), got["fmt_caps"].tolist()
    for i, r in enumerate(ref):
        want = [list(s) for s in r.caps[:max_caps]]
        assert caps[i][: len(want)] == want, (what, i, "caps")
        want = [list(s) for s in r.fmt_caps[:max_fmt_caps]]
        assert fmt_caps[i][: len(want)] == want, (what, i, "fmt_caps")


# ---------------------------------------------------------------------------
# Levenshtein
# ---------------------------------------------------------------------------


def levenshtein(a: bytes, b: bytes) -> int:
    """Two-row DP, unit costs."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, start=1):
        cur = [i] + [0] * len(b)
        for j, cb in enumerate(b, start=1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb))
        prev = cur
    return prev[len(b)]


assert levenshtein(b"kitten", b"sitting") == 3
assert levenshtein(b"", b"abc") == 3
assert levenshtein(b"abcabc", b"abcabc") == 0


def pack_rows(strings: Sequence[bytes], max_len: int, pad: int = 0x7E):
    """[N, max_len] u8 rows and int32 lengths; the padding is a byte no
    alphabet here holds, so a read past a length changes the result."""
    buf = bytearray()
    for s in strings:
        assert len(s) <= max_len
        buf += s + bytes([pad]) * (max_len - len(s))
    rows = torch.frombuffer(buf, dtype=torch.uint8).view(len(strings), max_len).clone()
    return rows, torch.tensor([len(s) for s in strings], dtype=torch.int32)


# ---------------------------------------------------------------------------
# hash sets
# ---------------------------------------------------------------------------

_U64 = (1 << 64) - 1


def home_slot(key: int, capacity: int) -> int:
    """Slot at which the probe chain of ``key`` starts."""
    h = key & _U64
    return ((h >> 32) ^ h) & (capacity - 1)


def as_i64(h: int) -> int:
    h &= _U64
    return h - (1 << 64) if h >> 63 else h


def keys_with_home(rng: random.Random, n: int, home: int, capacity: int,
                   taken: Optional[set] = None) -> List[int]:
    """``n`` distinct odd keys (as int64 values) whose home slot is ``home``;
    every second one has the top bit set, i.e. is negative as int64. None is
    in ``taken``, which is extended."""
    taken = set() if taken is None else taken
    mask = capacity - 1
    out: List[int] = []
    while len(out) < n:
        hi = rng.getrandbits(32)
        hi = (hi | 1 << 31) if len(taken) % 2 else (hi & ~(1 << 31))
        if not ((home ^ hi) & 1):
            hi ^= 1                      # so that the low word comes out odd
        lo = (rng.getrandbits(32) & ~mask) | ((home ^ hi) & mask)
        key = as_i64(hi << 32 | lo)
        assert key & 1 and home_slot(key, capacity) == home
        if key not in taken:
            taken.add(key)
            out.append(key)
    return out
