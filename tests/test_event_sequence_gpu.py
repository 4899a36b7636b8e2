"""Event sequences on the GPU: the three HIP kernels and the sort between them
against the CPU mirror (ops.event_sequence_step_cpu, the sequential loop), and
the stage inside GpuPipeline on cuda, eager, as a captured graph with a
partial replay and after a restored checkpoint, against the same pipeline on
CPU.

Everything is integers, so everything must be equal to the bit: seq_gram, the
gram hashes, seq_key and seq_hist."""
import random

import numpy as np
import pytest
import torch

from detectmateservice_amd import ops
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig

MAX_LEN = 32
T = 3
KEYS = [b"ses-%d" % i for i in range(7)] + [b""]  # 8 keys; an empty span is a key
MODES = {
    "header": {"kind": "header", "pos": 1},
    "scoped": {"kind": "variable", "pos": 0, "event": 2},
    "none": None,
}


def _batch(rng, B):
    """A parsed batch built by hand: a key in capture 0 (column 0) and one in
    format capture 1 (flush against max_len); some lines lack the captures,
    events are drawn from -1 .. T + 1. Returns the tensors and, per row, what
    the bookkeeping needs: (event, capture key or None, header key or None)."""
    lines = np.zeros((B, MAX_LEN), dtype=np.uint8)
    caps = np.full((B, 2, 2), -1, dtype=np.int32)
    fmt_caps = np.full((B, 2, 2), -1, dtype=np.int32)
    n_caps = np.zeros(B, dtype=np.int32)
    n_fmt = np.zeros(B, dtype=np.int32)
    event_id = np.zeros(B, dtype=np.int32)
    rows = []
    for i in range(B):
        ev = rng.choice([-1, 0, 1, 1, 2, 2, 2, 2, 3, 3, T + 1])
        # runs of one key, so that grams lie inside a batch even when n = 4
        if rows and rng.random() < 0.5:
            _, ck, hk = rows[-1]
            ck = rng.choice(KEYS) if ck is None else ck
            hk = rng.choice(KEYS) if hk is None else hk
        else:
            ck, hk = rng.choice(KEYS), rng.choice(KEYS)
        event_id[i] = ev
        lines[i, :len(ck)] = list(ck)
        caps[i, 0] = (0, len(ck))
        lines[i, MAX_LEN - len(hk):] = list(hk)
        fmt_caps[i, 1] = (MAX_LEN - len(hk), MAX_LEN)
        n_caps[i] = rng.choice([0, 1, 2, 2, 2, 2])
        n_fmt[i] = rng.choice([0, 2, 2, 2, 2])
        rows.append((ev, ck if n_caps[i] > 0 else None, hk if n_fmt[i] > 1 else None))
    match = {"event_id": event_id, "caps": caps, "n_caps": n_caps,
             "fmt_caps": fmt_caps, "n_fmt_caps": n_fmt}
    return (torch.from_numpy(lines),
            {k: torch.from_numpy(v) for k, v in match.items()}, rows)


class Book:
    """The test's own account of which situations a chain of calls went
    through, kept per bucket from the rows alone: who used the bucket last,
    how many of its events are on record, and how many of those this call."""

    def __init__(self, mode, K, length):
        self.mode, self.K, self.n = mode, K, length
        self.owner = {}    # bucket -> key hash
        self.depth = {}    # bucket -> events of the owner on record, <= n - 1
        self.seen = dict.fromkeys(
            ("inside", "carried", "walk_ended", "taken_over", "behind_n_valid",
             "event_below_1", "event_above_T", "key_absent"), 0)

    def _key(self, ev, ck, hk):
        if self.mode == "none":
            return 1
        if self.mode == "header":
            return None if hk is None else ops.fnv1a64(hk)
        return None if ck is None or ev != 2 else ops.fnv1a64(ck)

    def call(self, rows, n_valid):
        in_call = {}  # bucket -> (key hash, rows of it in a row in this call)
        for i, (ev, ck, hk) in enumerate(rows):
            if i >= n_valid:
                self.seen["behind_n_valid"] += 1
                continue
            if ev < 1:
                self.seen["event_below_1"] += 1
                continue
            if ev > T:
                self.seen["event_above_T"] += 1
                continue
            kh = self._key(ev, ck, hk)
            if kh is None:
                self.seen["key_absent"] += 1
                continue
            b = ops.sequence_bucket(kh, self.K)
            if b not in in_call:
                if self.owner.get(b) == kh and self.depth[b] >= self.n - 1:
                    self.seen["carried"] += 1
                elif b in self.owner and self.owner[b] != kh:
                    self.seen["taken_over"] += 1
                in_call[b] = (kh, 1)
            elif in_call[b][0] != kh:
                self.seen["walk_ended"] += 1
                in_call[b] = (kh, 1)
            else:
                if in_call[b][1] >= self.n - 1:
                    self.seen["inside"] += 1
                in_call[b] = (kh, in_call[b][1] + 1)
            if self.owner.get(b) != kh:
                self.owner[b], self.depth[b] = kh, 0
            self.depth[b] = min(self.depth[b] + 1, self.n - 1)


def _chains(B):
    """Every (mode, K, length, n_valid) chain of three calls for batch size B,
    as (mode, K, length, n_valid, [batch, batch, batch])."""
    rng = random.Random(1000 + B)
    for mode in MODES:
        batches = [_batch(rng, B) for _ in range(3)]
        for K in (1, 4, 64):
            for length in (2, 3, 4):
                for n_valid in sorted({0, B - 1, B}):
                    yield mode, K, length, n_valid, batches


def situations(B):
    """What the chains of batch size B went through, by the test's own books:
    {situation: count}, summed over the chains."""
    total = {}
    for mode, K, length, n_valid, batches in _chains(B):
        book = Book(mode, K, length)
        for _, _, rows in batches:
            book.call(rows, n_valid)
        for k, v in book.seen.items():
            total[k] = total.get(k, 0) + v
    return total


def _cuda(match):
    return {k: v.cuda() for k, v in match.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257])
def test_kernels_match_mirror(B):
    for mode, K, length, n_valid, batches in _chains(B):
        kw = dict(length=length, max_keys=K, key=MODES[mode])
        cpu = ops.EventSequenceState(T, device="cpu", **kw)
        gpu = ops.EventSequenceState(T, device="cuda", **kw)
        for call, (lines, match, _) in enumerate(batches):
            where = (mode, K, length, n_valid, call)
            want_gram, want_hash = cpu.step(lines, match, n_valid)
            got_gram, got_hash = gpu.step(lines.cuda(), _cuda(match), n_valid)
            assert got_hash.shape == (B, 1), where
            assert torch.equal(got_gram.cpu(), want_gram), where
            assert torch.equal(got_hash.cpu(), want_hash), where
            assert torch.equal(gpu.seq_key.cpu(), cpu.seq_key), where
            assert torch.equal(gpu.seq_hist.cpu(), cpu.seq_hist), where
        if n_valid == 0:
            assert not gpu.seq_key.any() and not gpu.seq_hist.any()
        elif B >= 255:
            assert int((cpu.seq_key != 0).sum()) >= 1
    if B >= 255:
        seen = situations(B)
        assert all(seen.values()), seen  # every situation was exercised


def test_chosen_seeds_reach_every_situation():
    """No GPU needed: the batches the kernel test draws at B >= 255 hold
    every situation its docstring names."""
    for B in (255, 256, 257):
        seen = situations(B)
        assert all(seen.values()), (B, seen)


@pytest.mark.gpu
def test_empty_batch_launches_nothing_and_returns_empty():
    gpu = ops.EventSequenceState(T, device="cuda", max_keys=4)
    lines, match, _ = _batch(random.Random(0), 0)
    gram, hashes = gpu.step(lines.cuda(), _cuda(match))
    assert gram.shape == (0,) and hashes.shape == (0, 1)
    assert gram.dtype == hashes.dtype == torch.int64 and gram.is_cuda


# ---------------------------------------------------------------------------
# pipeline: cuda (eager, captured graph, partial replay, restored state)
# against CPU
# ---------------------------------------------------------------------------

#: the last template matches every line, the empty pad rows of a partial
#: replay included: without a key those rows would be members
TEMPLATES = ["open <*>", "cmd <*> <*>", "close <*>", "<*>"]
CONFIGS = {
    "per_session": {"length": 3, "max_keys": 64, "capacity": 1024,
                    "key": {"kind": "variable", "pos": 0, "name": "ses"}},
    "whole_stream": {"length": 2, "max_keys": 1, "capacity": 1024},
}


def _log_lines(rng, n, odd):
    """n lines of interleaved sessions; with ``odd`` some sessions skip or
    repeat a step and some lines match only the catch-all template."""
    live, out, next_id = [], [], rng.randrange(1000)
    while len(out) < n:
        if len(live) < 12:
            sid, next_id = f"s{next_id}", next_id + 1
            steps = [f"open {sid}"] + [f"cmd {sid} x"] * rng.randrange(1, 4) + [f"close {sid}"]
            if odd and rng.random() < 0.3:
                steps.pop(rng.randrange(len(steps)))
            if odd and rng.random() < 0.2:
                steps.insert(rng.randrange(len(steps)), rng.choice(steps))
            live.append(steps)
        q = rng.choice(live)
        out.append(q.pop(0))
        if not q:
            live.remove(q)
        if odd and rng.random() < 0.03:
            out.append("something else")
    return [t.encode() for t in out[:n]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_pipeline_cuda_matches_cpu_eager_graph_partial_restore(name):
    G = 512
    rng = random.Random(17)
    cfg = dict(templates=TEMPLATES, use_transformer=False, max_len=MAX_LEN,
               train_lines=G + 200, event_sequence=CONFIGS[name])
    dev = GpuPipeline(PipelineConfig(**cfg), device="cuda")
    ref = GpuPipeline(PipelineConfig(**cfg), device="cpu")

    def same_state(where):
        sg, sc = dev.event_sequence.state_dict(), ref.event_sequence.state_dict()
        for k in ops.EventSequenceState._STATE:
            assert torch.equal(sg[k], sc[k]), (k, where)
        table = dev.sequence_grams.tables[0].cpu()
        assert sorted(table[table != 0].tolist()) == sorted(ref.sequence_grams.sets[0]), where

    def step(raw, how, where):
        packed = ops.pack_lines(raw, MAX_LEN)
        want = ref.process_packed(*packed)
        got = getattr(dev, how)(packed[0].cuda(), packed[1].cuda())
        for k in ("seq_unseen", "seq_gram", "anomaly", "event_id"):
            assert got[k].shape[0] == len(raw), (k, where)
            assert torch.equal(got[k].cpu(), want[k]), (k, where)
        assert torch.equal(want["anomaly"], want["seq_unseen"] > 0)
        same_state(where)
        return want

    # training batch, straddling batch, detect batch
    w = step(_log_lines(rng, G, False), "process_packed", "train")
    assert not w["seq_unseen"].any()
    w = step(_log_lines(rng, 200, False) + _log_lines(rng, G - 200, True),
             "process_packed", "straddle")
    assert not w["seq_unseen"][:200].any() and w["seq_unseen"][200:].any()
    learnt = len(ref.sequence_grams.sets[0])
    assert learnt >= 4
    saved = ref.state_dict()
    detect_raw = _log_lines(rng, G, True)
    w = first = step(detect_raw, "process_packed", "detect")
    assert 0 < int(w["seq_unseen"].sum()) < G // 2
    assert len(ref.sequence_grams.sets[0]) == learnt  # detect learns nothing

    # captured graph: a full replay and a 100-row partial replay, whose pad
    # rows match "<*>" and would enter the history without n_valid
    assert dev.enable_graph(G)
    same_state("capture")  # warm-ups and capture moved nothing
    step(_log_lines(rng, G, True), "process_packed_graph", "replay")
    step(_log_lines(rng, 100, True), "process_packed_graph_partial", "partial")
    step(_log_lines(rng, G, True), "process_packed_graph", "after partial")

    # the state from before the detect batch, restored into the tensors the
    # graph reads: that batch continues the sessions that were open back then
    # and gets the grams it got the first time
    for pipe in (dev, ref):
        pipe.stages[0].load_state_dict(saved)  # the stage alone: seen_lines stays
    same_state("restored")
    again = step(detect_raw, "process_packed_graph", "restored replay")
    assert torch.equal(again["seq_gram"], first["seq_gram"])
    assert torch.equal(again["seq_unseen"], first["seq_unseen"])
    assert dev.seen_lines == ref.seen_lines == 6 * G + 100
