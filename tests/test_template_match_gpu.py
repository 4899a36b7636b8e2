"""dmx_template_match against the bytes reference of kernel_refs.py, and
against the C++ twin on the same tensors, on the corpora of
test_template_match_cpu.py: batch sizes around the four-lines-per-workgroup
boundary, rows of 64, 100 and 512 bytes, with and without a format and a
fold, both alphabets, no templates, over-long length words, a narrow capture
table and a segment blob at the LDS limit. Exact integer comparison; one
launch of at most 257 lines per case."""
import pytest
import torch

from detectmateservice_amd import ops
from kernel_refs import (
    SEED,
    Corpus,
    expect_match,
    format_segments,
    make_corpus,
    ref_match,
    split_template,
)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_extension(), "HIP extension _dmx_C not built/loadable"
    yield


KEYS = ("event_id", "fmt_caps", "n_fmt_caps", "caps", "n_caps", "span_start", "span_end")


def _args(m, max_caps=None):
    return (m.fmt_bytes, m.fmt_seg_off, m.seg_bytes, m.seg_off, m.tpl_seg_start,
            m.lowercase, m.max_fmt_caps, m.max_caps if max_caps is None else max_caps)


def _kernel(m, lines, lens, max_caps=None):
    """One launch through the binding; ``m`` holds cuda tensors."""
    out = ops._C.template_match(lines.cuda(), lens.cuda(), *_args(m, max_caps))
    return {k: v.cpu() for k, v in zip(KEYS, out)}


def _twin(m_cpu, lines, lens, max_caps=None):
    out = ops._C.template_match_cpu(lines, lens, *_args(m_cpu, max_caps))
    return dict(zip(KEYS, out))


def _matchers(templates, log_format, lowercase, max_len):
    return [ops.TemplateMatcher(templates, log_format=log_format, lowercase=lowercase,
                                device=d, max_len=max_len) for d in ("cuda", "cpu")]


def _check(c: Corpus, rows=None, max_caps=None, templates=None):
    """Kernel vs reference and vs the C++ twin on ``rows`` of corpus ``c``."""
    rows = list(range(len(c.rows))) if rows is None else rows
    templates = c.templates if templates is None else templates
    mg, mc = _matchers(templates, c.log_format, c.lowercase, c.max_len)
    lines, lens = c.lines_tensor()[rows], c.len_tensor()[rows]
    ref = [c.ref[i] for i in rows]
    if not templates:
        ref = [r._replace(event_id=-1, caps=[]) for r in ref]
    width = mg.max_caps if max_caps is None else max_caps
    got = _kernel(mg, lines, lens, max_caps)
    expect_match(got, ref, width, mg.max_fmt_caps, "kernel")
    twin = _twin(mc, lines, lens, max_caps)
    for k in ("event_id", "n_caps", "n_fmt_caps"):
        assert torch.equal(got[k], twin[k]), k
    for i in range(len(rows)):
        n = min(int(twin["n_caps"][i]), width)
        assert torch.equal(got["caps"][i, :n], twin["caps"][i, :n]), i
        n = min(int(twin["n_fmt_caps"][i]), mg.max_fmt_caps)
        assert torch.equal(got["fmt_caps"][i, :n], twin["fmt_caps"][i, :n]), i
    return got


def _id(alphabet, max_len, with_format, lowercase):
    return (f"{alphabet}-{max_len}-{'fmt' if with_format else 'nofmt'}-"
            f"{'lower' if lowercase else 'exact'}")


FULL = [("ascii", 512, True, False), ("bytes", 512, True, True),
        ("bytes", 512, False, False), ("ascii", 512, False, True),
        ("ascii", 100, True, True), ("ascii", 100, False, False),
        ("bytes", 100, True, False), ("bytes", 100, False, True),
        ("ascii", 64, True, False), ("bytes", 64, False, True),
        ("bytes", 64, True, True), ("ascii", 64, False, False)]


@pytest.mark.parametrize("alphabet,max_len,with_format,lowercase",
                         [pytest.param(*p, id=_id(*p)) for p in FULL])
def test_kernel_vs_reference_257_lines(alphabet, max_len, with_format, lowercase):
    """257 lines: 64 full workgroups and one with a single line."""
    _check(make_corpus(SEED, alphabet, max_len, with_format, lowercase))


@pytest.mark.parametrize("B", [1, 3, 4, 5])
@pytest.mark.parametrize("alphabet,max_len,with_format,lowercase",
                         [pytest.param("bytes", 512, True, True, id="bytes-512-fmt-lower"),
                          pytest.param("ascii", 100, False, False, id="ascii-100-nofmt-exact")])
def test_kernel_vs_reference_small_batches(B, alphabet, max_len, with_format, lowercase):
    """Batches around the four-lines-per-workgroup boundary; the rows are
    spread over the corpus so that they differ in outcome."""
    c = make_corpus(SEED, alphabet, max_len, with_format, lowercase)
    _check(c, rows=[(7 + 53 * k) % len(c.rows) for k in range(B)])


@pytest.mark.parametrize("alphabet,max_len,with_format,lowercase",
                         [pytest.param("ascii", 512, True, False, id="ascii-512-fmt-exact"),
                          pytest.param("bytes", 100, False, True, id="bytes-100-nofmt-lower")])
def test_kernel_catch_all_last(alphabet, max_len, with_format, lowercase):
    c = make_corpus(SEED, alphabet, max_len, with_format, lowercase, True)
    got = _check(c)
    assert int(got["event_id"].min()) >= 1


@pytest.mark.parametrize("with_format", [False, True])
def test_kernel_no_templates(with_format):
    """tpl_seg_start == [0]: nothing matches, the content span still stands."""
    c = make_corpus(SEED, "bytes", 100, with_format, False)
    got = _check(c, templates=[])
    assert got["event_id"].tolist() == [-1] * len(c.rows)
    assert got["n_caps"].tolist() == [0] * len(c.rows)


@pytest.mark.parametrize("max_len", [64, 100, 512])
def test_kernel_cuts_line_len_to_max_len(max_len):
    """A length word above max_len gives what the same bytes give with the
    length word at max_len, in all seven outputs."""
    c = make_corpus(SEED, "bytes", max_len, True, True)
    mg, _ = _matchers(c.templates, c.log_format, c.lowercase, max_len)
    lens = c.len_tensor()
    assert int((lens > max_len).sum()) >= 1
    a = _kernel(mg, c.lines_tensor(), lens)
    b = _kernel(mg, c.lines_tensor(), lens.clamp(max=max_len))
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    expect_match(a, c.ref, mg.max_caps, mg.max_fmt_caps)


@pytest.mark.parametrize("alphabet,max_len,with_format",
                         [("bytes", 512, True), ("ascii", 100, False)])
def test_kernel_small_max_caps(alphabet, max_len, with_format):
    """max_caps below the widest template: n_caps is the uncut count, caps
    has the passed width and holds the first max_caps spans."""
    c = make_corpus(SEED, alphabet, max_len, with_format, False, False, 257, 2)
    got = _check(c, max_caps=2)
    assert tuple(got["caps"].shape) == (257, 2, 2)
    assert int(got["n_caps"].max()) == 3


def _lds_case(n_full, tail_len):
    """``n_full`` distinct 70-byte literal templates that differ only near
    their end, then one of ``tail_len`` bytes; five lines that match the
    first, the last and none of them."""
    stem = "k=" + "abcdx" * 11 + "zz"                     # 59 bytes
    tpls = [f"{stem}{i:04d}" + "qzqzqzq" for i in range(n_full)]
    assert all(len(t) == 70 for t in tpls) and len(set(tpls)) == n_full
    last = ("T" * tail_len)
    tpls.append(last)
    lines = [tpls[0].encode(), last.encode(), tpls[n_full - 1].encode()[:-1] + b"!",
             tpls[0].encode() + b"x", last.encode()]
    return tpls, lines


@pytest.mark.parametrize("n_full,tail_len", [(906, 68), (100, 3)],
                         ids=["at-the-limit", "blob-not-16-aligned"])
def test_kernel_segment_blob_at_lds_limit(n_full, tail_len):
    """The accepting twin of the rejecting case in test_kernel_contracts.py:
    a segment blob whose LDS need is exactly the 64 KiB a launch may ask for,
    and one whose length is no multiple of 16."""
    tpls, raw = _lds_case(n_full, tail_len)
    mg, mc = _matchers(tpls, None, False, 512)
    blob = int(mg.seg_bytes.numel())
    assert blob == 70 * n_full + tail_len
    if n_full == 906:
        # tm_lds_bytes: the blob rounded up to 16, plus four staged lines
        assert ((blob + 15) & ~15) + 4 * 512 == 64 * 1024
    else:
        assert blob % 16 != 0
    lines, lens = ops.pack_lines(raw, 512)
    segs = [split_template(t) for t in tpls]
    ref = [ref_match(bytes(lines[i].tolist()), int(lens[i]), 512, None, segs, False)
           for i in range(len(raw))]
    assert [r.event_id for r in ref] == [1, n_full + 1, -1, -1, n_full + 1]
    got = _kernel(mg, lines, lens)
    expect_match(got, ref, mg.max_caps, mg.max_fmt_caps, "kernel")
    twin = _twin(mc, lines, lens)
    assert torch.equal(got["event_id"], twin["event_id"])


def test_kernel_rows_are_independent():
    """A line's outputs do not depend on its row or on its neighbours: row 0
    of a one-line batch equals the line's row in the 257-line batch."""
    c = make_corpus(SEED, "bytes", 512, True, True)
    mg, _ = _matchers(c.templates, c.log_format, c.lowercase, 512)
    lines, lens = c.lines_tensor(), c.len_tensor()
    full = _kernel(mg, lines, lens)
    overlong = next(i for i, n in enumerate(c.line_len) if n > 512)
    for i in (0, 3, 130, 255, 256, overlong):
        one = _kernel(mg, lines[i:i + 1], lens[i:i + 1])
        expect_match(one, [c.ref[i]], mg.max_caps, mg.max_fmt_caps, f"row {i}")
        for k in ("event_id", "n_caps", "n_fmt_caps", "span_start", "span_end"):
            assert one[k][0] == full[k][i], (i, k)
        n = min(int(full["n_caps"][i]), mg.max_caps)
        assert torch.equal(one["caps"][0, :n], full["caps"][i, :n]), i
        n = min(int(full["n_fmt_caps"][i]), mg.max_fmt_caps)
        assert torch.equal(one["fmt_caps"][0, :n], full["fmt_caps"][i, :n]), i
