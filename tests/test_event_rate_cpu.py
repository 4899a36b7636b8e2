"""Event-rate windows without a GPU (docs/kernels.md, "Event-rate windows"):
the CPU mirror against the host FrequencyDetector, invariance under how the
stream is cut into batches, the binding's contract clauses, and the stage
inside GpuPipeline and FusedPipelineDetector on a CPU device."""
import math
import random

import pytest
import torch

from detectmateservice_amd import ops
from detectmateservice_amd.library.detectors import FrequencyDetector
from detectmateservice_amd.library.detectors.fused_pipeline import (
    FusedPipelineDetector,
)
from detectmateservice_amd.library.parsers.template_matcher import MatcherParser
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig
from detectmateservice_amd.schemas import DetectorSchema, LogSchema, ParserSchema

T = 6  # templates of the synthetic stream: events 1 .. 6, -1 = unparsed
N_WINDOWS = 16


def _stream(L: int, seed: int = 5):
    """Event ids of N_WINDOWS windows of exactly L lines. Events 1 .. 4 are
    steady at about L / 12 per window (50 at L = 600) with a small
    deterministic wobble; event 2 floods 5x in windows 8 and 9, event 3
    drops to 0 from window 12 on, event 5 first appears in window 10, about
    L / 60 lines per window are unparsed and event 6 fills the window."""
    rng = random.Random(seed)
    per = max(L // 12, 1)
    out = []
    for w in range(N_WINDOWS):
        counts = {}
        for e in (1, 2, 3, 4):
            counts[e] = per + ((w * 7 + e * 3) % 5 - 2 if per >= 5 else 0)
        if w in (8, 9):
            counts[2] = 5 * per
        if w >= 12:
            counts[3] = 0
        if w >= 10:
            counts[5] = per // 2 + 1
        counts[-1] = max(L // 60, 1) + w % 2
        used = sum(counts.values())
        assert used < L
        counts[6] = L - used
        window = [e for e, c in counts.items() for _ in range(c)]
        rng.shuffle(window)
        out.extend(window)
    return out


def _state(L, **kw):
    return ops.EventRateState(T, window_lines=L, device="cpu", **kw)


def _run(state, ids, batch, train_lines=0):
    """Feed ids in batches of `batch`; returns [(global line, hits)] of the
    boundary lines that carry hits and the list of all boundary lines."""
    alerts, boundaries = [], []
    for at in range(0, len(ids), batch):
        chunk = torch.tensor(ids[at:at + batch], dtype=torch.int32)
        train_upto = min(len(chunk), max(0, train_lines - at))
        out = state.step(chunk, train_upto=train_upto)
        slot, hits = out["rate_slot"], out["rate_hits"]
        for i in torch.nonzero(slot >= 0).flatten().tolist():
            boundaries.append(at + i)
            assert int(slot[i]) == len([b for b in boundaries if b >= at]) - 1
        for i in torch.nonzero(hits).flatten().tolist():
            alerts.append((at + i, int(hits[i])))
    return alerts, boundaries


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    for k in ("mean", "var", "known", "open_counts", "ctl"):
        # bit for bit: compare the f64 words as integers
        xa = sa[k].view(torch.int64) if sa[k].dtype == torch.float64 else sa[k]
        xb = sb[k].view(torch.int64) if sb[k].dtype == torch.float64 else sb[k]
        assert torch.equal(xa, xb), k


# ---------------------------------------------------------------------------
# mirror against FrequencyDetector
# ---------------------------------------------------------------------------


def test_mirror_matches_frequency_detector():
    L, train = 600, 1500  # training ends mid-window, after two rolls
    conf = {"window_lines": L, "ewma_alpha": 0.3, "z_threshold": 4.0,
            "min_windows": 3}
    ids = _stream(L)
    det = FrequencyDetector({"data_use_training": train, **conf})

    # the detector's own z values, taken from its state as it rolls
    zs = []
    roll = det._roll_window

    def spy():
        for ev, mean in det._mean.items():
            c = float(det._counts.get(ev, 0))
            zs.append((c - mean) / math.sqrt(max(det._var[ev], 1.0)))
        return roll()

    det._roll_window = spy
    frames = [ParserSchema(logID=str(i), log="x", EventID=e).serialize()
              for i, e in enumerate(ids)]
    want = {}
    for at in range(0, len(frames), 1000):
        for i, o in enumerate(det.process_batch(frames[at:at + 1000])):
            if o is not None:
                want[at + i] = DetectorSchema.deserialize(o).score
    # a condition on the inputs, not a tolerance: no verdict hangs on the
    # last bits of z
    assert zs and min(abs(abs(z) - conf["z_threshold"]) for z in zs) > 1e-6
    # the stream shows what it was built to show
    assert any(b // L in (8, 9) for b in want), want
    assert any(b // L >= 12 for b in want), want

    state = _state(L, **{k: v for k, v in conf.items() if k != "window_lines"})
    alerts, boundaries = _run(state, ids, 1000, train_lines=train)
    assert boundaries == [L * (w + 1) - 1 for w in range(N_WINDOWS)]
    assert {i for i, _ in alerts} == set(want)
    assert all(float(h) == want[i] for i, h in alerts)

    assert int(state.ctl[1]) == det._windows_seen == N_WINDOWS
    known = {(-1 if e == 0 else e) for e in torch.nonzero(state.known).flatten().tolist()}
    assert known == set(det._mean)
    for ev in det._mean:
        e = 0 if ev == -1 else ev
        # ** 2 is not guaranteed to be d * d to the bit; each update adds a
        # few ulp and the (1 - a) contraction keeps the sum under few / a ulp
        assert float(state.mean[e]) == pytest.approx(det._mean[ev], rel=1e-12, abs=0)
        assert float(state.var[e]) == pytest.approx(det._var[ev], rel=1e-12, abs=0)


def test_event_zero_and_out_of_range_count_nowhere():
    st = _state(4, min_windows=0)
    ev = torch.tensor([0, T + 1, 2**31 - 1, 1, -7, -1, 1, 1, 1], dtype=torch.int32)
    out = st.step(ev)
    # all 9 rows are valid lines of the stream (two windows of 4 complete),
    # but only ids -7, -1 (bin 0) and 1 are counted
    assert out["rate_counts"].shape == (9 // 4 + 2, T + 1)
    assert out["rate_counts"].sum(dim=1).tolist() == [1, 4, 1, 0]
    assert out["rate_counts"][1].tolist() == [2, 2, 0, 0, 0, 0, 0]
    assert out["rate_slot"].tolist() == [-1, -1, -1, 0, -1, -1, -1, 1, -1]
    assert st.ctl.tolist() == [1, 2]
    assert st.open_counts.tolist() == [0, 1, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------
# batch-split invariance
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("batch", ["1", "L", "L-1", "L+1", "L//3"])
def test_batch_split_invariance(batch):
    L = 60
    ids = _stream(L)
    whole = _state(L)
    ref, ref_bounds = _run(whole, ids, len(ids), train_lines=150)
    assert ref, "the stream must raise rate alerts"
    split = _state(L)
    got, bounds = _run(split, ids, eval(batch, {"L": L}), train_lines=150)
    assert got == ref and bounds == ref_bounds
    _same_state(split, whole)


def test_n_valid_zero_is_a_noop_and_n_valid_cuts_the_tail():
    L = 60
    ids = _stream(L)
    a, b = _state(L), _state(L)
    _run(a, ids[:200], 200)
    _run(b, ids[:200], 200)
    out = b.step(torch.tensor(ids[200:500], dtype=torch.int32), n_valid=0)
    _same_state(a, b)
    assert not out["rate_hits"].any() and (out["rate_slot"] == -1).all()
    assert torch.equal(out["rate_counts"][0], b.open_counts)

    chunk = torch.tensor(ids[200:500], dtype=torch.int32)
    oa = a.step(chunk[:170])
    ob = b.step(chunk, n_valid=170)
    _same_state(a, b)
    assert torch.equal(ob["rate_hits"][:170], oa["rate_hits"])
    assert torch.equal(ob["rate_slot"][:170], oa["rate_slot"])
    assert not ob["rate_hits"][170:].any() and (ob["rate_slot"][170:] == -1).all()
    rows = oa["rate_counts"].shape[0]
    assert torch.equal(ob["rate_counts"][:rows], oa["rate_counts"])
    assert torch.equal(ob["rate_z"][:rows], oa["rate_z"])


def test_empty_batch():
    st = _state(5)
    st.step(torch.tensor([1, 1, 2], dtype=torch.int32))
    before = st.state_dict()
    out = st.step(torch.zeros(0, dtype=torch.int32))
    assert out["rate_counts"].shape == (2, T + 1) and out["rate_hits"].shape == (0,)
    after = st.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in st._STATE)


def test_state_holder_checks_shapes_and_parameters():
    st = _state(10)
    with pytest.raises(ValueError, match="window_lines"):
        _state(20).load_state_dict(st.state_dict())
    other = ops.EventRateState(T + 1, window_lines=10)
    with pytest.raises(ValueError, match="mean"):
        other.load_state_dict(st.state_dict())
    with pytest.raises(ValueError, match="ER_MAX_EVENTS"):
        ops.EventRateState(ops.ER_MAX_EVENTS)
    ops.EventRateState(ops.ER_MAX_EVENTS - 1)
    for bad in ({"window_lines": 0}, {"ewma_alpha": 0.0}, {"ewma_alpha": 1.5},
                {"z_threshold": -1.0}, {"min_windows": -1}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            ops.EventRateState(T, **bad)


# ---------------------------------------------------------------------------
# contract clauses of the binding, reached with CPU tensors
# ---------------------------------------------------------------------------

needs_ext = pytest.mark.skipif(
    not ops.have_extension(), reason="HIP extension _dmx_C not built")


def _args(B=8, E=T + 1, **over):
    a = {
        "event_id": torch.zeros(B, dtype=torch.int32),
        "n_valid": torch.full((1,), B, dtype=torch.int32),
        "mean": torch.zeros(E, dtype=torch.float64),
        "var": torch.zeros(E, dtype=torch.float64),
        "known": torch.zeros(E, dtype=torch.int32),
        "open_counts": torch.zeros(E, dtype=torch.int32),
        "ctl": torch.zeros(2, dtype=torch.int32),
        "train_upto": 0, "window_lines": 4, "ewma_alpha": 0.3,
        "z_threshold": 4.0, "min_windows": 3,
    }
    a.update(over)
    return list(a.values())


@needs_ext
def test_binding_limits_match_python():
    lim = ops._C.event_rate_limits()
    assert lim["max_events"] == ops.ER_MAX_EVENTS
    assert lim["max_cells"] == ops.ER_MAX_CELLS


@needs_ext
def test_binding_device_clause_comes_last():
    with pytest.raises(RuntimeError, match="event_id must be on a GPU"):
        ops._C.event_rate_step(*_args())
    with pytest.raises(RuntimeError, match="event_id must be on a GPU"):
        ops._C.event_rate_step(*_args(B=0))


E_ = T + 1
BAD = [
    ("event_id", dict(event_id=torch.zeros(8, dtype=torch.int64))),
    ("event_id", dict(event_id=torch.zeros((8, 1), dtype=torch.int32))),
    ("event_id", dict(event_id=torch.zeros(16, dtype=torch.int32)[::2])),
    ("n_valid", dict(n_valid=torch.zeros(1, dtype=torch.int64))),
    ("n_valid", dict(n_valid=torch.zeros(2, dtype=torch.int32))),
    ("n_valid", dict(n_valid=torch.zeros((), dtype=torch.int32))),
    ("mean", dict(mean=torch.zeros(E_, dtype=torch.float32))),
    ("mean", dict(mean=torch.zeros((E_, 1), dtype=torch.float64))),
    ("mean", dict(mean=torch.zeros(0, dtype=torch.float64),
                  var=torch.zeros(0, dtype=torch.float64))),
    ("var", dict(var=torch.zeros(E_ + 1, dtype=torch.float64))),
    ("var", dict(var=torch.zeros(E_, dtype=torch.float32))),
    ("known", dict(known=torch.zeros(E_ - 1, dtype=torch.int32))),
    ("known", dict(known=torch.zeros(E_, dtype=torch.bool))),
    ("open_counts", dict(open_counts=torch.zeros(E_ + 1, dtype=torch.int32))),
    ("open_counts", dict(open_counts=torch.zeros(E_, dtype=torch.int64))),
    ("ctl", dict(ctl=torch.zeros(3, dtype=torch.int32))),
    ("ctl", dict(ctl=torch.zeros(2, dtype=torch.int64))),
    ("window_lines", dict(window_lines=0)),
    ("window_lines", dict(window_lines=2**31)),
    ("ewma_alpha", dict(ewma_alpha=0.0)),
    ("ewma_alpha", dict(ewma_alpha=1.0000001)),
    ("ewma_alpha", dict(ewma_alpha=float("nan"))),
    ("z_threshold", dict(z_threshold=-0.5)),
    ("z_threshold", dict(z_threshold=float("nan"))),
    ("min_windows", dict(min_windows=-1)),
    ("train_upto", dict(train_upto=-1)),
    ("train_upto", dict(train_upto=9)),
]


@needs_ext
@pytest.mark.parametrize("name,over", BAD, ids=[f"{n}-{i}" for i, (n, _) in enumerate(BAD)])
def test_binding_rejects_and_names_the_argument(name, over):
    with pytest.raises(RuntimeError) as ei:
        ops._C.event_rate_step(*_args(**over))
    msg = str(ei.value).splitlines()[0]
    assert msg.startswith(name), msg
    assert "must be on a GPU" not in msg


@needs_ext
def test_binding_caps():
    E = ops.ER_MAX_EVENTS + 1
    with pytest.raises(RuntimeError, match=r"^mean: E .* ER_MAX_EVENTS"):
        ops._C.event_rate_step(*_args(
            E=E, mean=torch.zeros(E, dtype=torch.float64)))
    # NW * E: 8192 bins x (4096 / 1 + 2) slots is above 2^24 cells
    E, B = ops.ER_MAX_EVENTS, 4096
    assert (B + 2) * E > ops.ER_MAX_CELLS
    with pytest.raises(RuntimeError, match=r"^event_id: NW \* E"):
        ops._C.event_rate_step(*_args(B=B, E=E, window_lines=1))
    # the same shapes with a longer window pass every clause but the device's
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops._C.event_rate_step(*_args(B=B, E=E, window_lines=1000))


# ---------------------------------------------------------------------------
# pipeline and service on a CPU device
# ---------------------------------------------------------------------------

TEMPLATES = ["alpha <*>", "beta <*>", "gamma <*>", "delta <*>"]
RATE = {"window_lines": 20, "min_windows": 2}


def _window_lines(w, counts):
    """One window of 20 log lines with the given per-word counts, in a
    fixed interleaved order."""
    words = [k for k, c in counts.items() for _ in range(c)]
    assert len(words) == 20
    random.Random(w).shuffle(words)
    return [f"{word} v{w}" for word in words]


STEADY = {"alpha": 8, "beta": 6, "gamma": 4, "zzz": 2}


def _log_stream():
    """12 windows: steady, beta floods in window 6, gamma stops from window
    9 on and delta first shows up in window 8."""
    lines = []
    for w in range(12):
        c = dict(STEADY)
        if w == 6:
            c.update(alpha=2, beta=16, gamma=0)
        if w >= 9:
            c.update(gamma=0, alpha=12)
        if w == 8:
            c.update(alpha=6, delta=2)
        lines.extend(_window_lines(w, c))
    return lines


def _fused(train=0, **kw):
    conf = {"templates": TEMPLATES, "event_rate": dict(RATE),
            "data_use_training": train, "use_transformer": False,
            "max_len": 32, "device": "cpu"}
    conf.update(kw)
    return FusedPipelineDetector(conf)


def _frames(lines, start=0):
    return [LogSchema(logID=f"id{start + i}", log=t).serialize()
            for i, t in enumerate(lines)]


def _alert_ids(det, frames, batch):
    got = {}
    for at in range(0, len(frames), batch):
        for o in det.process_batch(frames[at:at + batch]):
            if o is not None:
                a = DetectorSchema.deserialize(o)
                got[a.logIDs[0]] = a
    return got


def test_pipeline_outputs_and_training_phase():
    lines = _log_stream()
    packed = ops.pack_lines([t.encode() for t in lines], 32)

    def run(train):
        pipe = GpuPipeline(PipelineConfig(
            templates=TEMPLATES, use_transformer=False, max_len=32,
            train_lines=train, event_rate=dict(RATE)))
        return pipe, pipe.process_packed(*packed)

    pipe, out = run(0)
    B, E = len(lines), len(TEMPLATES) + 1
    assert out["rate_hits"].shape == (B,) and out["rate_slot"].shape == (B,)
    assert out["rate_counts"].shape == out["rate_z"].shape == (B // 20 + 2, E)
    bounds = torch.nonzero(out["rate_slot"] >= 0).flatten().tolist()
    assert bounds == [20 * (w + 1) - 1 for w in range(12)]
    assert out["rate_counts"][6].tolist() == [2, 2, 16, 0, 0]
    hit_rows = torch.nonzero(out["rate_hits"]).flatten().tolist()
    assert 139 in hit_rows and set(hit_rows) <= set(bounds)
    assert torch.equal(out["anomaly"], out["rate_hits"] > 0)

    # training up to line 150: window 6 (boundary 139) still moves the
    # baseline but raises nothing
    pipe_t, out_t = run(150)
    assert not out_t["rate_hits"][:150].any()
    assert not out_t["anomaly"][:150].any()
    assert torch.equal(out_t["rate_hits"][150:], out["rate_hits"][150:])
    assert torch.equal(out_t["rate_counts"], out["rate_counts"])
    assert out_t["rate_z"][6].abs().sum() == 0 and out["rate_z"][6].abs().sum() > 0
    _same_state(pipe_t.event_rate, pipe.event_rate)

    # stage off: the result is what it always was, .get() gives None
    off = GpuPipeline(PipelineConfig(templates=TEMPLATES, use_transformer=False,
                                     max_len=32)).process_packed(*packed)
    assert all(k not in off and off.get(k) is None for k in GpuPipeline._RATE_KEYS)
    assert not off["anomaly"].any()
    # stage skipped for one call (a rescore): keys there, None, state unmoved
    before = pipe.event_rate.state_dict()
    skipped = pipe.process_packed(*packed, rate=False)
    assert all(skipped[k] is None for k in GpuPipeline._RATE_KEYS)
    after = pipe.event_rate.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in pipe.event_rate._STATE)


def test_fused_detector_matches_parser_frequency_chain():
    lines = _log_stream()
    frames = _frames(lines)
    det = _fused(train=50)
    got = _alert_ids(det, frames, 64)

    parser = MatcherParser({"templates": TEMPLATES})
    freq = FrequencyDetector({"data_use_training": 50, "window_lines": 20,
                              "ewma_alpha": 0.3, "z_threshold": 4.0,
                              "min_windows": 2})
    want = {}
    for at in range(0, len(frames), 64):
        for o in freq.process_batch(parser.process_batch(frames[at:at + 64])):
            if o is not None:
                a = DetectorSchema.deserialize(o)
                want[a.logIDs[0]] = a
    assert want and set(got) == set(want)
    # alert frames sit exactly on boundary lines
    assert all((int(k[2:]) + 1) % 20 == 0 for k in got)
    assert "id139" in got
    for k, a in got.items():
        assert a.description.startswith("Anomaly: event rate: "), a.description
        # one "<who>: <count>/window" entry per anomaly of the host detector
        assert a.description.count("/window") == int(want[k].score)
        assert a.score == 0.0  # score stays the transformer score
    assert "event 2: 16/window (z=+" in got["id139"].description
    assert "unparsed" not in got["id139"].description


def test_unparsed_flood_is_named():
    det = _fused()
    lines = []
    for w in range(6):
        c = dict(STEADY) if w < 5 else {"alpha": 4, "beta": 4, "gamma": 2, "zzz": 10}
        lines.extend(_window_lines(w, c))
    got = _alert_ids(det, _frames(lines), 50)
    assert list(got) == ["id119"]
    assert "unparsed: 10/window (z=+" in got["id119"].description


def test_checkpoint_mid_window_continues():
    frames = _frames(_log_stream())
    whole = _fused(train=50)
    want = _alert_ids(whole, frames, 30)

    first = _fused(train=50)
    got = _alert_ids(first, frames[:130], 30)  # 130 = 6.5 windows
    state = first.state_dict()
    assert state["event_rate"]["ctl"].tolist() == [10, 6]
    second = _fused(train=50)
    second.load_state_dict(state)
    got.update(_alert_ids(second, frames[130:], 30))
    assert set(got) == set(want) and "id139" in got
    assert all(got[k].description == want[k].description for k in want)
    _same_state(second.pipe.event_rate, whole.pipe.event_rate)


def test_rescore_and_dist_sync_leave_rate_state():
    frames = _frames(_log_stream())
    det = _fused(line_buffer_bytes=1 << 20)
    _alert_ids(det, frames[:130], 30)
    before = det.state_dict()["event_rate"]
    res = det.rescore_window(130)
    assert res["rescored"] == 130 and res["anomalies"] == 0
    det.dist_sync()
    after = det.state_dict()["event_rate"]
    assert set(before) == set(after)
    for k in before:
        assert (torch.equal(before[k], after[k]) if torch.is_tensor(before[k])
                else before[k] == after[k]), k
    # and the live stream goes on as if nothing had happened
    ref = _fused()
    _alert_ids(ref, frames[:130], 30)
    assert (set(_alert_ids(det, frames[130:], 30))
            == set(_alert_ids(ref, frames[130:], 30)) != set())


def test_config_errors():
    with pytest.raises(ValueError, match="window_line"):
        _fused(event_rate={"window_line": 20})
    with pytest.raises(ValueError, match="ewma_alpha"):
        _fused(event_rate={"ewma_alpha": 0})
    with pytest.raises(ValueError, match="ER_MAX_EVENTS"):
        GpuPipeline(PipelineConfig(
            templates=[f"t{i} <*>" for i in range(ops.ER_MAX_EVENTS)],
            use_transformer=False, event_rate={}))
    # defaults are FrequencyDetectorConfig's
    st = _fused(event_rate={}).pipe.event_rate
    ref = FrequencyDetector({}).config
    assert (st.window_lines, st.ewma_alpha, st.z_threshold, st.min_windows) == (
        ref.window_lines, ref.ewma_alpha, ref.z_threshold, ref.min_windows)
    assert _fused(event_rate=None).pipe.event_rate is None
