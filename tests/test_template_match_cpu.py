"""The CPU matcher paths against the bytes reference of kernel_refs.py:
``TemplateMatcher(device="cpu")`` (the C++ twin when the extension is built,
the pure-Python mirror otherwise), the pure-Python mirror on its own, and
the two against each other. Exact integer comparison throughout."""
import random

import pytest
import torch

from detectmateservice_amd import ops
from kernel_refs import (
    LOG_FORMAT,
    SEED,
    expect_match,
    format_segments,
    keys_with_home,
    home_slot,
    levenshtein,
    make_corpus,
    ref_match,
    ref_segments,
    split_template,
)

CASES = [
    pytest.param(alphabet, max_len, with_format, lowercase,
                 id=f"{alphabet}-{max_len}-{'fmt' if with_format else 'nofmt'}-"
                    f"{'lower' if lowercase else 'exact'}")
    for alphabet in ("ascii", "bytes")
    for max_len in (100, 512)
    for with_format in (False, True)
    for lowercase in (False, True)
]


def _matcher(corpus, templates=None):
    return ops.TemplateMatcher(
        corpus.templates if templates is None else templates,
        log_format=corpus.log_format, lowercase=corpus.lowercase,
        device="cpu", max_len=corpus.max_len)


def _python_path(m, lines, lens):
    out = m._match_cpu(lines, lens)
    m._add_spans(out, lens, lines.shape[1])
    return out


# -- the reference itself -------------------------------------------------------


def test_reference_by_hand():
    """The greedy-anchored rule on lines small enough to work out by hand."""
    seg = split_template
    assert ref_segments(b"ab=1 cd=2", 0, 9, seg("ab=<*> cd=<*>")) == [(3, 4), (8, 9)]
    assert ref_segments(b"xab=1", 0, 5, seg("ab=<*>")) is None          # anchored at start
    assert ref_segments(b"ab=1", 0, 4, seg("ab=<*>z")) is None
    assert ref_segments(b"aXbXc", 0, 5, seg("a<*>X<*>c")) == [(1, 1), (2, 4)]  # first X
    assert ref_segments(b"abc", 0, 3, seg("<*>")) == [(0, 3)]
    assert ref_segments(b"", 0, 0, seg("<*>")) == [(0, 0)]
    assert ref_segments(b"abc", 0, 3, seg("<*><*>c")) == [(0, 2)]
    assert ref_segments(b"cabc", 0, 4, seg("<*><*>c")) is None          # first c, not last
    assert ref_segments(b"abcabcabcabd!", 0, 13, seg("<*>abcabcabd<*>")) == [(0, 3), (12, 13)]
    assert ref_segments(b"abc", 0, 3, seg("abc")) == []
    assert ref_segments(b"abcd", 0, 4, seg("abc")) is None
    assert ref_segments(b"..abc..", 2, 5, seg("abc")) == []             # inside a span
    # format, fold and cut
    fmt = format_segments(LOG_FORMAT)
    r = ref_match(b"h=Q AB=x cd=y", 13, 64, fmt, [seg("ab=<*> cd=<*>")], True)
    assert (r.event_id, r.caps, r.fmt_caps) == (1, [(7, 8), (12, 13)], [(2, 3), (4, 13)])
    assert (r.span_start, r.span_end) == (4, 13)
    r = ref_match(b"H=Q ab=x cd=y", 13, 64, fmt, [seg("ab=<*> cd=<*>")], True)
    assert (r.event_id, r.fmt_caps, r.span_start, r.span_end) == (-1, [], 0, 13)
    r = ref_match(b"abcdef", 200, 4, None, [seg("abcd")], False)
    assert (r.event_id, r.span_end) == (1, 4)
    # 0xC9 is not an upper-case letter, whatever a code page says
    r = ref_match(b"\xc9", 1, 8, None, [seg("é")], True)
    assert r.event_id == -1


def test_levenshtein_reference():
    assert levenshtein(b"kitten", b"sitting") == 3
    assert levenshtein(b"", b"abc") == 3
    assert levenshtein(b"same", b"same") == 0
    assert levenshtein(b"abc", b"") == 3
    assert levenshtein(b"flaw", b"lawn") == 2


def test_hash_key_helper():
    rng = random.Random(1)
    for capacity in (8, 16, 64):
        for home in (0, 3, capacity - 1):
            keys = keys_with_home(rng, 10, home, capacity)
            assert len(set(keys)) == 10
            assert all(k & 1 and home_slot(k, capacity) == home for k in keys)
            assert sum(k < 0 for k in keys) == 5
            assert all(-(1 << 63) <= k < (1 << 63) for k in keys)


# -- the matcher paths ------------------------------------------------------------


@pytest.mark.parametrize("alphabet,max_len,with_format,lowercase", CASES)
def test_cpu_matcher_vs_reference(alphabet, max_len, with_format, lowercase):
    c = make_corpus(SEED, alphabet, max_len, with_format, lowercase)
    m = _matcher(c)
    out = m.match_packed(c.lines_tensor(), c.len_tensor())
    expect_match(out, c.ref, m.max_caps, m.max_fmt_caps, "match_packed")


@pytest.mark.parametrize("alphabet,max_len,with_format,lowercase", CASES)
def test_python_mirror_vs_reference(alphabet, max_len, with_format, lowercase):
    """The path a CPU-only install runs, whether or not the extension is
    built here."""
    c = make_corpus(SEED, alphabet, max_len, with_format, lowercase)
    m = _matcher(c)
    out = _python_path(m, c.lines_tensor(), c.len_tensor())
    expect_match(out, c.ref, m.max_caps, m.max_fmt_caps, "_match_cpu")


@pytest.mark.parametrize("alphabet", ["ascii", "bytes"])
def test_cpu_matcher_catch_all_and_short_rows(alphabet):
    """A catch-all last: no line is unmatched. Rows of 64 bytes."""
    for max_len, with_format, lowercase in ((64, True, True), (64, False, False),
                                            (512, True, False)):
        c = make_corpus(SEED, alphabet, max_len, with_format, lowercase, True)
        m = _matcher(c)
        for out in (m.match_packed(c.lines_tensor(), c.len_tensor()),
                    _python_path(m, c.lines_tensor(), c.len_tensor())):
            expect_match(out, c.ref, m.max_caps, m.max_fmt_caps)
            assert int(out["event_id"].min()) >= 1


@pytest.mark.parametrize("with_format", [False, True])
def test_cpu_matcher_small_max_caps(with_format):
    """A table narrower than the widest template: the counts stay uncut,
    the first ``max_caps`` spans are written."""
    c = make_corpus(SEED, "bytes", 512, with_format, False, False, 257, 2)
    m = _matcher(c)
    assert m.max_caps > 2
    m.max_caps = 2
    for out in (m.match_packed(c.lines_tensor(), c.len_tensor()),
                _python_path(m, c.lines_tensor(), c.len_tensor())):
        assert int(out["n_caps"].max()) > 2
        expect_match(out, c.ref, 2, m.max_fmt_caps)


@pytest.mark.parametrize("with_format", [False, True])
def test_cpu_matcher_no_templates(with_format):
    c = make_corpus(SEED, "bytes", 100, with_format, False)
    m = _matcher(c, templates=[])
    assert m.tpl_seg_start.tolist() == [0]
    ref = [r._replace(event_id=-1, caps=[]) for r in c.ref]
    for out in (m.match_packed(c.lines_tensor(), c.len_tensor()),
                _python_path(m, c.lines_tensor(), c.len_tensor())):
        expect_match(out, ref, m.max_caps, m.max_fmt_caps)
        assert out["event_id"].tolist() == [-1] * len(ref)
        assert out["n_caps"].tolist() == [0] * len(ref)


def test_cpu_matcher_cuts_line_len_to_max_len():
    """A length word above max_len reads as max_len, in every output."""
    c = make_corpus(SEED, "bytes", 100, True, True)
    m = _matcher(c)
    lens = c.len_tensor()
    assert int((lens > c.max_len).sum()) >= 1
    cut = lens.clamp(max=c.max_len)
    for path in (m.match_packed, lambda a, b: _python_path(m, a, b)):
        a, b = path(c.lines_tensor(), lens), path(c.lines_tensor(), cut)
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.skipif(not ops.have_extension(), reason="compares with the C++ twin")
@pytest.mark.parametrize("alphabet,max_len,with_format,lowercase", CASES)
def test_python_mirror_vs_cpp_twin(alphabet, max_len, with_format, lowercase):
    c = make_corpus(SEED, alphabet, max_len, with_format, lowercase)
    m = _matcher(c)
    lines, lens = c.lines_tensor(), c.len_tensor()
    py = m._match_cpu(lines, lens)
    ev, fc, nfc, caps, ncaps = ops._C.template_match_cpu(
        lines, lens, m.fmt_bytes, m.fmt_seg_off, m.seg_bytes, m.seg_off,
        m.tpl_seg_start, m.lowercase, m.max_fmt_caps, m.max_caps)
    assert torch.equal(py["event_id"], ev)
    assert torch.equal(py["n_fmt_caps"], nfc)
    assert torch.equal(py["n_caps"], ncaps)
    for i in range(len(c.rows)):
        n = min(int(ncaps[i]), m.max_caps)
        assert torch.equal(py["caps"][i, :n], caps[i, :n]), i
        n = min(int(nfc[i]), m.max_fmt_caps)
        assert torch.equal(py["fmt_caps"][i, :n], fc[i, :n]), i
