"""Value ranges on the GPU: the two HIP kernels against the CPU mirror
(ops.value_range_step_cpu), and the stage inside GpuPipeline on cuda, eager, as
a captured graph with a partial replay and after a restored checkpoint,
against the same pipeline on CPU.

Everything must be equal to the bit: range_code, lo, hi and n because min, max
and the compares are exact, range_value (compared by bit pattern) because the
one f64 division of the parse is correctly rounded on the device as in
float()."""
import random

import pytest
import torch

from detectmateservice_amd import ops
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig

pytestmark = pytest.mark.gpu

MAX_LEN = 64
#: where a field's text is written: at column 0, in the middle, and ending
#: flush against max_len (18 bytes each, the longest text below)
REGIONS = [(0, "left"), (23, "left"), (MAX_LEN, "right")]

EDGE = [
    b"0", b"-0", b"-0.00", b"+5", b"007", b"1.", b".5", b"--5", b"1e5",
    b"1,000", b" 1", b"", b"123456789012345", b"1234567890123456",
    b"123456789012.345", b"1234567890123.456", b"1234567890.1234567",
    b"999999999999999", b"0.99999999999999", b"-99999999999999.9",
    b"9.99999999999999", b"+", b"-", b".", b"12-3", b"4.5.6",
]
assert max(len(s) for s in EDGE) == 18


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _number(rng) -> bytes:
    digits = rng.randrange(1, 16)
    frac = rng.randrange(0, digits)
    text = "".join(rng.choice("0123456789") for _ in range(digits))
    if frac:
        text = text[:digits - frac] + "." + text[digits - frac:]
    return (rng.choice(["", "", "-", "+"]) + text).encode()


def _batch(rng, B):
    """A parsed batch built by hand: three fields per line (captures 0 and 1
    and format capture 1), each an edge string or a random number, written
    into one of the three regions of the line; some lines lack captures, and
    events are drawn from {-1, 1, 2}."""
    lines = torch.zeros((B, MAX_LEN), dtype=torch.uint8)
    caps = torch.full((B, 3, 2), -1, dtype=torch.int32)
    fmt_caps = torch.full((B, 2, 2), -1, dtype=torch.int32)
    n_caps = torch.zeros(B, dtype=torch.int32)
    n_fmt = torch.zeros(B, dtype=torch.int32)
    event_id = torch.zeros(B, dtype=torch.int32)
    for i in range(B):
        # line 0 has every field and numbers in them: one training row arms
        # every range
        event_id[i] = rng.choice([-1, 1, 1, 2]) if i else 1
        n_caps[i] = rng.choice([0, 1, 2, 2, 3, 3]) if i else 3
        n_fmt[i] = rng.choice([0, 2, 2, 2]) if i else 2
        order = rng.sample(REGIONS, 3)
        for (table, pos), (at, side) in zip(((caps, 0), (caps, 1), (fmt_caps, 1)), order):
            text = rng.choice(EDGE) if i and rng.random() < 0.35 else _number(rng)
            start = at if side == "left" else at - len(text)
            lines[i, start:start + len(text)] = torch.tensor(list(text), dtype=torch.uint8)
            table[i, pos, 0], table[i, pos, 1] = start, start + len(text)
    match = {"event_id": event_id, "caps": caps, "n_caps": n_caps,
             "fmt_caps": fmt_caps, "n_fmt_caps": n_fmt}
    return lines, match


RANGES = [
    {"kind": "variable", "pos": 0, "non_numeric": "alert"},
    {"kind": "header", "pos": 1, "slack": 0.25, "min": -1e6, "max": 1e9},
    {"kind": "variable", "pos": 1, "event": 1, "slack": 1e-3},
]


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_kernels_match_mirror(B, R):
    rng = random.Random(B * 101 + R)
    flagged = {1: 0, 2: 0, 3: 0}
    for train_upto in sorted({0, 1, B - 1, B}):
        cpu = ops.ValueRangeState(RANGES[:R], device="cpu")
        gpu = ops.ValueRangeState(RANGES[:R], device="cuda")
        for call in range(2):  # the second call starts from the first's state
            lines, match = _batch(rng, B)
            want_code, want_value = cpu.step(lines, match, train_upto)
            got_code, got_value = gpu.step(
                lines.cuda(), {k: v.cuda() for k, v in match.items()}, train_upto)
            where = (train_upto, call)
            assert torch.equal(got_code.cpu(), want_code), where
            assert torch.equal(_bits(got_value.cpu()), _bits(want_value)), where
            sg, sc = gpu.state_dict(), cpu.state_dict()
            for k in ops.ValueRangeState._STATE:
                assert torch.equal(_bits(sg[k]), _bits(sc[k])), (k, where)
            for c in flagged:
                flagged[c] += int((want_code == c).sum())
        if train_upto > 1:
            assert int(cpu.n.sum()) > 0
    if B >= 255:
        assert all(flagged.values()), flagged  # every code was exercised


def test_long_span_is_rejected_unread_and_bounds_hold():
    """A span longer than 17 bytes, a span reaching past max_len and captures
    beyond the table are "not a number" / absent, on both sides alike."""
    lines = torch.full((4, MAX_LEN), ord("7"), dtype=torch.uint8)
    caps = torch.tensor([[[0, MAX_LEN]], [[60, MAX_LEN + 4]], [[5, 4]], [[0, 15]]],
                        dtype=torch.int32)
    match = {"event_id": torch.ones(4, dtype=torch.int32), "caps": caps,
             "n_caps": torch.tensor([1, 1, 1, 9], dtype=torch.int32),
             "fmt_caps": torch.full((4, 1, 2), -1, dtype=torch.int32),
             "n_fmt_caps": torch.zeros(4, dtype=torch.int32)}
    ranges = [{"pos": 0, "non_numeric": "alert"}, {"pos": 5, "non_numeric": "alert"}]
    cpu = ops.ValueRangeState(ranges, device="cpu")
    gpu = ops.ValueRangeState(ranges, device="cuda")
    want = cpu.step(lines, match, 0)
    got = gpu.step(lines.cuda(), {k: v.cuda() for k, v in match.items()}, 0)
    assert want[0].tolist() == [[3, 0], [0, 0], [0, 0], [0, 0]]
    assert want[1][3].tolist() == [777777777777777.0, 0.0]
    assert torch.equal(got[0].cpu(), want[0])
    assert torch.equal(_bits(got[1].cpu()), _bits(want[1]))


# ---------------------------------------------------------------------------
# pipeline: cuda (eager, captured graph, partial replay, restored state)
# against CPU
# ---------------------------------------------------------------------------

TEMPLATES = ["bytes <*> dur <*>", "status <*>"]
FORMAT = "<Level> <Port>: <Content>"
PIPE_RANGES = [
    {"kind": "variable", "pos": 0, "event": 1, "name": "bytes", "slack": 0.05},
    {"kind": "variable", "pos": 1, "event": 1, "name": "dur", "non_numeric": "alert"},
    {"kind": "header", "pos": 1, "name": "port", "non_numeric": "alert"},
    {"kind": "variable", "pos": 0, "event": 2, "min": 100, "max": 599},
]


def _log_lines(rng, n, wide):
    """`wide` widens the value distributions, so that lines drawn with it
    fall outside what lines drawn without it taught."""
    out = []
    for _ in range(n):
        port = "http" if rng.random() < 0.02 else str(rng.randrange(1, 9000 if wide else 1024))
        if rng.random() < 0.7:
            size = rng.randrange(0, 3_000_000 if wide else 1_000_000)
            dur = "n/a" if rng.random() < 0.02 else f"{rng.random() * (3 if wide else 1):.3f}"
            out.append(f"INFO {port}: bytes {size} dur {dur}".encode())
        elif rng.random() < 0.9:
            status = rng.randrange(50, 700) if wide else rng.randrange(100, 600)
            out.append(f"INFO {port}: status {status}".encode())
        else:
            out.append(b"unparsed line")
    return out


def test_pipeline_cuda_matches_cpu_eager_graph_partial_restore():
    G = 512
    rng = random.Random(11)
    cfg = dict(templates=TEMPLATES, log_format=FORMAT, use_transformer=False,
               max_len=MAX_LEN, train_lines=G + 200, ranges=PIPE_RANGES)
    dev = GpuPipeline(PipelineConfig(**cfg), device="cuda")
    ref = GpuPipeline(PipelineConfig(**cfg), device="cpu")

    def same_state(where):
        sg, sc = dev.value_ranges.state_dict(), ref.value_ranges.state_dict()
        for k in ops.ValueRangeState._STATE:
            assert torch.equal(_bits(sg[k]), _bits(sc[k])), (k, where)

    def step(raw, how, where):
        packed = ops.pack_lines(raw, MAX_LEN)
        want = ref.process_packed(*packed)
        got = getattr(dev, how)(packed[0].cuda(), packed[1].cuda())
        n = len(raw)
        for k in ("range_code", "range_value", "anomaly", "event_id"):
            assert got[k].shape[0] == n, (k, where)
            assert torch.equal(_bits(got[k].cpu()), _bits(want[k])), (k, where)
        assert torch.equal(want["anomaly"], (want["range_code"] != 0).any(dim=1))
        same_state(where)
        return want

    # training batch, straddling batch, detect batch
    w = step(_log_lines(rng, G, False), "process_packed", "train")
    assert not w["range_code"].any()
    w = step(_log_lines(rng, 200, False) + _log_lines(rng, G - 200, True),
             "process_packed", "straddle")
    assert not w["range_code"][:200].any() and w["range_code"][200:].any()
    w = step(_log_lines(rng, G, True), "process_packed", "detect")
    assert {1, 2, 3} <= set(w["range_code"].unique().tolist())
    learnt = ref.value_ranges.state_dict()
    assert int(learnt["n"][0]) > 300 and int(learnt["n"][3]) > 50

    # captured graph: a full replay and a 100-row partial replay
    assert dev.enable_graph(G)
    same_state("capture")  # warm-ups and capture learnt nothing
    raw = _log_lines(rng, G, True)
    before = step(raw, "process_packed_graph", "replay")["range_code"].clone()
    step(_log_lines(rng, 100, True), "process_packed_graph_partial", "partial")

    # another state, restored into the tensors the graph reads: the same
    # lines are now judged against the restored bounds
    state = {"lo": torch.tensor([4000.0, 0.25, 100.0, 200.0], dtype=torch.float64),
             "hi": torch.tensor([50000.0, 0.5, 200.0, 299.0], dtype=torch.float64),
             "n": torch.tensor([7, 7, 7, 7])}
    dev.value_ranges.load_state_dict(state)
    ref.value_ranges.load_state_dict(state)
    after = step(raw, "process_packed_graph", "restored")["range_code"]
    # the restored ranges lie inside the learnt ones: what was flagged stays
    # flagged, and values between the two sets of bounds are flagged now
    assert bool((after != 0)[before != 0].all())
    assert int((after != 0).sum()) > int((before != 0).sum())
    assert dev.seen_lines == ref.seen_lines == 5 * G + 100
