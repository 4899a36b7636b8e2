"""GpuPipeline: fused reader→parser→detector on one device.

The MI355X-native fast path: when pipeline stages are
co-located, frames never round-trip through protobuf between stages —
lines live in a [B, max_len] u8 SoA tensor on the GPU and flow
parser-kernel → hash-probe / transformer-scoring as device tensors on one
HIP stream. The socket Service path (core.py) remains for distributed /
edge deployment; this class is what bench.py drives and what a
TransformerDetector service uses internally per batch.

Per batch, all on `device`: the template_match kernel (log_format header
split + template match: event_id + capture spans), then the configured stages
of stages.py, ``pipe.stages``, in this order: new value (watches and
combinations), event rate, event sequence, value ranges, transformer score.
Launches, alert reasons and checkpoint keys follow that list; each stage class
says what it computes.
Anomaly = NewValue unseen-value hit OR unseen combination OR transformer
score > threshold OR, on a window's boundary line, a flagged event rate OR an
n-gram of event ids never seen for the line's key OR a numeric field outside
its learned range.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, Optional, Sequence

import torch

from . import ops
from .models.bert_tiny import BertTinyConfig
from .stages import (EventRateStage, EventSequenceStage, NewValueStage,
                     TransformerStage, ValueRangeStage, marked)


@dataclass
class PipelineConfig:
    templates: Sequence[str] = ()
    log_format: Optional[str] = None
    lowercase: bool = False
    max_len: int = 512
    #: watched fields: list of dicts {kind: "variable"|"header", pos: int,
    #: event: int (-1 = any)} — mirrors NewValueDetector specs
    watches: Sequence[dict] = ()
    #: watched combinations: each a list of members written like `watches`
    #: entries; a line alerts when the tuple of its member values is new
    #: (NewValueComboDetector). hashset_capacity applies per combination.
    combos: Sequence[Sequence[dict]] = ()
    hashset_capacity: int = 1 << 16
    #: transformer detector on/off + threshold
    use_transformer: bool = True
    score_threshold: float = 3.0
    #: "head": the model's score head. "embedding": distance from the
    #: Gaussian fitted to the embeddings of the first train_lines rows.
    score_mode: str = "head"
    train_lines: int = 0  # training-phase length (data_use_training)
    #: event-rate windows (FrequencyDetector's keys and defaults:
    #: window_lines 1000, ewma_alpha 0.3, z_threshold 4.0, min_windows 3);
    #: None = stage off, {} = on with the defaults
    event_rate: Optional[dict] = None
    #: event sequences: {length, key, max_keys, capacity} (docs/kernels.md,
    #: "Event sequences"): the n-gram of event ids that a line completes in
    #: the history of its key (a field written like a `watches` entry; no
    #: key = the whole stream) alerts when training never saw it. None =
    #: stage off, {} = on with the defaults
    event_sequence: Optional[dict] = None
    #: numeric value ranges: list of dicts written like `watches` entries
    #: plus the optional keys name, slack, non_numeric ("ignore" | "alert")
    #: and min / max (docs/kernels.md, "Value ranges"). The smallest and
    #: largest value of the field over the first train_lines rows are kept
    #: on the device; a later value outside them alerts.
    ranges: Sequence[dict] = ()
    bert: BertTinyConfig = field(default_factory=BertTinyConfig)
    seed: int = 1234


class GpuPipeline:
    _RATE_KEYS = EventRateStage.keys

    def __init__(self, config: PipelineConfig, device: str | torch.device = "cpu") -> None:
        self.config = config
        self.device = torch.device(device)
        self.matcher = ops.TemplateMatcher(
            config.templates, log_format=config.log_format,
            lowercase=config.lowercase, device=self.device, max_len=config.max_len)
        if config.score_mode not in ("head", "embedding"):
            raise ValueError(
                f"score_mode must be 'head' or 'embedding', got {config.score_mode!r}")
        if config.score_mode == "embedding" and not config.use_transformer:
            raise ValueError("score_mode 'embedding' needs use_transformer")
        nv = NewValueStage(config, self.device)
        rate = (EventRateStage(config, self.device, len(self.matcher.templates))
                if config.event_rate is not None else None)
        seq = (EventSequenceStage(config, self.device, len(self.matcher.templates))
               if config.event_sequence is not None else None)
        ranges = ValueRangeStage(config, self.device) if len(config.ranges) else None
        bert = TransformerStage(config, self.device) if config.use_transformer else None
        # the state objects under their public names (None = not configured)
        self.specs, self.members, self.combo_off, self.n_combos = (
            nv.specs, nv.members, nv.combo_off, nv.n_combos)
        (self.hashsets, self.event_rate, self.event_sequence,
         self.value_ranges, self.model) = (
            s.state if s else None for s in (nv, rate, seq, ranges, bert))
        self.sequence_grams = seq.grams if seq else None
        self.embedding_stats = bert.stats if bert else None
        self.stages = [s for s in (nv if nv.state is not None else None,
                                   rate, seq, ranges, bert) if s is not None]
        self.seen_lines = 0
        # hipGraph capture state (enable_graph(); steady-state detect only)
        self._graph = self._graph_in = self._graph_out = None

    def process_packed(self, lines: torch.Tensor, line_len: torch.Tensor,
                       n_valid: Optional[int] = None, rate: bool = True) -> dict:
        """lines [B, max_len] u8 + lengths on self.device → result tensors.

        Returns event_id [B], anomaly [B] (bool), scores [B] (f32, 0 when
        transformer off), nv_unseen [B, W] (None without watches),
        combo_unseen [B, C] (None without combos) and, with event_rate
        configured, rate_hits [B], rate_slot [B], rate_counts [NW, E] and
        rate_z [NW, E] (absent otherwise: ``out.get("rate_hits")`` is None).
        With ranges configured (and only then) range_code int32 [B, R] (0 =
        nothing, 1 = below, 2 = above, 3 = not a number) and range_value f64
        [B, R]. With event_sequence configured seq_unseen int32 [B] and
        seq_gram int64 [B] (the line's n-gram, 16 bits per event id).

        ``n_valid`` and ``rate`` concern the two stages with stream state,
        event rate and event sequence: only the first n_valid rows (default:
        all) enter the windows and the histories, and ``rate=False`` skips
        both, so the call neither moves that state nor reports their alerts
        (their keys are None). The first ``train_lines`` rows of the stream
        train; the stream position ``seen_lines`` moves only here and in a
        graph replay."""
        B = lines.shape[0]
        train_upto = min(B, max(0, self.config.train_lines - self.seen_lines))
        out = self._run(lines, line_len, train_upto, n_valid, rate,
                        self.config.score_threshold)
        self.seen_lines += B
        return out

    def rescore(self, lines: torch.Tensor, lens: torch.Tensor,
                threshold: Optional[float] = None) -> Dict[str, torch.Tensor]:
        """Judge old lines as the detect phase would, with ``threshold`` in
        place of the configured one if given: nothing trains, the event-rate
        and event-sequence stages are skipped, the stream position stays."""
        return self._run(lines, lens, 0, None, False, float(
            self.config.score_threshold if threshold is None else threshold))

    def _run(self, lines, line_len, train_upto: int, n_valid: Optional[int],
             rate: bool, threshold: float) -> Dict[str, torch.Tensor]:
        """Parse, every stage, OR of the flags. Reads and writes neither
        seen_lines nor config.score_threshold."""
        B, dev = lines.shape[0], lines.device
        match = (marked("dmx::parse", dev, self.matcher.match_packed, lines, line_len)
                 if B else None)
        out = {
            "event_id": (match["event_id"] if B
                         else torch.zeros(0, dtype=torch.int32, device=dev)),
            "anomaly": None,
            "scores": torch.zeros(B, dtype=torch.float32, device=dev),
            "nv_unseen": None, "combo_unseen": None,
            "match": match,
        }
        # a stage's keys are there whenever it is configured: those of an
        # empty batch for B == 0, None when it is skipped (read with .get())
        for s in self.stages:
            skip = B == 0 or (s.windowed and not rate)
            out.update(s.empty(dev) if skip else marked(
                "dmx::" + s.name, dev, s.run, lines, match, train_upto, n_valid))
        anomaly = out["scores"] > threshold
        for s in self.stages if B else ():
            flag = s.flags(out)
            if flag is not None:
                anomaly = anomaly | flag
        out["anomaly"] = anomaly
        return out

    def process_lines(self, raw_lines: Sequence[bytes]) -> Dict[str, torch.Tensor]:
        lines, lens = ops.pack_lines(raw_lines, self.config.max_len, device=self.device)
        return self.process_packed(lines, lens)

    # state: seen_lines plus each stage's, under its checkpoint key. A key with
    # no configured stage is ignored; a stage with no key keeps its start state.
    def state_dict(self) -> Dict[str, Any]:
        state: Dict[str, Any] = {"seen_lines": self.seen_lines}
        for s in self.stages:
            state.update(s.state_dict())
        return state

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self.seen_lines = int(state.get("seen_lines", 0))
        for s in self.stages:
            s.load_state_dict(state)

    def dist_sync(self, group=None) -> None:
        """COLLECTIVE merge of the data-parallel state of every stage that
        has one: hash sets by union, value ranges by MIN / MAX / SUM."""
        import torch.distributed as tdist
        if not tdist.is_initialized() or tdist.get_world_size(group) <= 1:
            return
        for s in self.stages:
            s.dist_sync(group)

    # hipGraph capture (HIP graphs for the launch-bound steady state —
    # SURVEY.md build mandate). Valid only AFTER the training phase: the
    # captured graph replays the detect-only path at fixed batch size.
    @property
    def graph_enabled(self) -> bool:
        return self._graph is not None

    def enable_graph(self, batch_size: int) -> bool:
        if self.device.type != "cuda":
            return False
        if self.seen_lines < self.config.train_lines:
            raise RuntimeError("enable_graph() requires the training phase done")
        static_lines = torch.zeros(
            (batch_size, self.config.max_len), dtype=torch.uint8, device=self.device)
        static_lens = torch.zeros((batch_size,), dtype=torch.int32, device=self.device)
        # warm up allocator/kernels on the same shapes, then capture. The
        # event-rate and event-sequence stages read their row count from a
        # device word: 0 makes the warm-ups leave their state as it is, and
        # the captured launches read whatever the word holds at replay.
        args = (static_lines, static_lens, 0, 0, True, self.config.score_threshold)
        for _ in range(2):
            self._run(*args)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._run(*args)
        self._graph, self._graph_in, self._graph_out = graph, args[:2], out
        return True

    def _replay(self, lines: torch.Tensor, lens: torch.Tensor) -> int:
        """Copy B <= captured rows in (pad rows get len 0), replay."""
        assert self._graph is not None, "call enable_graph() first"
        sl, sn = self._graph_in
        B = lines.shape[0]
        assert B <= sl.shape[0]
        full = B == sl.shape[0]
        (sl if full else sl[:B]).copy_(lines, non_blocking=True)
        (sn if full else sn[:B]).copy_(lens, non_blocking=True)
        if not full:
            sn[B:].zero_()
        for s in self.stages:
            s.before_replay(B)
        self._graph.replay()
        self.seen_lines += B
        return B

    def process_packed_graph(self, lines: torch.Tensor, lens: torch.Tensor) -> dict:
        """Replay the captured graph on a new batch (same B, max_len)."""
        self._replay(lines, lens)
        return self._graph_out

    def process_packed_graph_partial(self, lines: torch.Tensor, lens: torch.Tensor) -> dict:
        """Replay on a batch SMALLER than the captured size: pad rows get
        len 0 (their kernels no-op on the span but the transformer still
        runs them — acceptable when partial batches are rare stream
        edges). Outputs are sliced back to the true batch size."""
        B = self._replay(lines, lens)
        whole = {k for s in self.stages for k in s.per_slot_keys}

        def cut(v):
            if torch.is_tensor(v):
                return v[:B]
            if isinstance(v, dict):
                return {k: cut(x) for k, x in v.items()}
            return v

        return {k: (v if k in whole else cut(v)) for k, v in self._graph_out.items()}
