"""GpuPipeline: fused reader→parser→detector on one device.

The MI355X-native fast path: when pipeline stages are
co-located, frames never round-trip through protobuf between stages —
lines live in a [B, max_len] u8 SoA tensor on the GPU and flow
parser-kernel → hash-probe / transformer-scoring as device tensors on one
HIP stream. The socket Service path (core.py) remains for distributed /
edge deployment; this class is what bench.py drives and what a
TransformerDetector service uses internally per batch.

Stage structure per batch (all on `device`):
  1. template_match kernel: log_format header split + template match
     (event_id + capture spans)
  2. NewValue watch: hash watched spans (kernel) -> probe GPU hash sets
     (training batches insert instead). With ``combos`` configured the same
     launch also hashes each combination of fields (docs/kernels.md,
     "Combination hash") and the same probe covers watches and combos.
  3. Transformer scorer (BERT-tiny bf16 MFMA) over content-span byte tokens
  4. With ``event_rate`` configured: per-event line counts in windows of
     ``window_lines`` lines against an EWMA baseline (docs/kernels.md,
     "Event-rate windows"). The only stage whose verdict is about the stream
     and not about one line: its state lives on the device and the line that
     completes a window carries the alert.
  5. With ``ranges`` configured: each range's field is parsed as a decimal
     number from the line bytes and judged against the smallest and largest
     value seen in training (docs/kernels.md, "Value ranges"); one launch in
     the steady state, state on the device.
Anomaly = NewValue unseen-value hit OR unseen combination OR transformer
score > threshold OR, on a window's boundary line, a flagged event rate OR a
numeric field outside its learned range.

``score_mode`` says what the transformer score is. ``"head"`` (default) is
the model's linear score head. ``"embedding"`` is the distance of the line's
mean-pooled embedding from a diagonal Gaussian fitted to the training-phase
rows (``EmbeddingStats``): those rows update the moments and score 0, later
rows score ``sqrt(mean_i((x_i - mu_i)^2 / var_i))``, one launch of the fused
kernel's distance head per batch and no [B, hidden] write. An empty content
span is far from any trained distribution, so it alerts (about 11.5 on the
audit-log generator against a normal maximum of about 1.3).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .models.bert_tiny import (
    BertTinyConfig,
    BertTinyDetectorModel,
    EmbeddingStats,
)


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
    #: numeric value ranges: list of dicts written like `watches` entries
    #: plus the optional keys name, slack, non_numeric ("ignore" | "alert")
    #: and min / max (docs/kernels.md, "Value ranges"). The smallest and
    #: largest value of the field over the first train_lines rows are kept
    #: on the device; a later value outside them alerts.
    ranges: Sequence[dict] = ()
    bert: BertTinyConfig = field(default_factory=BertTinyConfig)
    seed: int = 1234


class GpuPipeline:
    #: event-rate outputs; the last two are per window slot, [NW, E], not per
    #: line
    _RATE_KEYS = ("rate_hits", "rate_slot", "rate_counts", "rate_z")
    _PER_SLOT_KEYS = ("rate_counts", "rate_z")

    def __init__(self, config: PipelineConfig, device: str | torch.device = "cpu") -> None:
        self.config = config
        self.device = torch.device(device)
        self.matcher = ops.TemplateMatcher(
            config.templates,
            log_format=config.log_format,
            lowercase=config.lowercase,
            device=self.device,
            max_len=config.max_len,
        )
        specs = [ops.watch_spec_row(w) for w in config.watches]
        self.specs = (
            torch.tensor(specs, dtype=torch.int32, device=self.device)
            if specs
            else torch.zeros((0, 4), dtype=torch.int32, device=self.device)
        )
        # combinations: CSR member table, validated on the host before upload
        self.n_combos = len(config.combos)
        self.members = self.combo_off = None
        if self.n_combos:
            members, combo_off = ops.pack_combos(config.combos)
            self.members = members.to(self.device)
            self.combo_off = combo_off.to(self.device)
        # one table per watch, then one per combination
        n_tables = len(specs) + self.n_combos
        self.hashsets = (
            ops.GpuHashSets(n_tables, config.hashset_capacity, device=self.device)
            if n_tables
            else None
        )
        self.model = (
            BertTinyDetectorModel(config.bert, device=self.device, seed=config.seed)
            if config.use_transformer
            else None
        )
        if config.score_mode not in ("head", "embedding"):
            raise ValueError(
                f"score_mode must be 'head' or 'embedding', got {config.score_mode!r}")
        if config.score_mode == "embedding" and self.model is None:
            raise ValueError("score_mode 'embedding' needs use_transformer")
        self.embedding_stats = (
            EmbeddingStats(config.bert.hidden, device=self.device)
            if config.score_mode == "embedding"
            else None
        )
        self.event_rate: Optional[ops.EventRateState] = None
        if config.event_rate is not None:
            unknown = set(config.event_rate) - set(ops.EVENT_RATE_DEFAULTS)
            if unknown:
                raise ValueError(
                    f"unknown event_rate key(s) {sorted(unknown)}; valid keys: "
                    f"{sorted(ops.EVENT_RATE_DEFAULTS)}")
            self.event_rate = ops.EventRateState(
                len(self.matcher.templates), device=self.device,
                **{**ops.EVENT_RATE_DEFAULTS, **config.event_rate})
        self.value_ranges: Optional[ops.ValueRangeState] = (
            ops.ValueRangeState(list(config.ranges), device=self.device)
            if len(config.ranges) else None
        )
        self.seen_lines = 0
        # hipGraph capture state (enable_graph(); steady-state detect only)
        self._graph = None
        self._graph_in: Optional[tuple] = None
        self._graph_out: Optional[Dict[str, torch.Tensor]] = None

    # ------------------------------------------------------------------
    def process_packed(
        self, lines: torch.Tensor, line_len: torch.Tensor,
        n_valid: Optional[int] = None, rate: bool = True,
    ) -> Dict[str, torch.Tensor]:
        """lines [B, max_len] u8 + lengths on self.device → result tensors.

        Returns event_id [B], anomaly [B] (bool), scores [B] (f32, 0 when
        transformer off), nv_unseen [B, W] (None without watches),
        combo_unseen [B, C] (None without combos) and, with event_rate
        configured, rate_hits [B], rate_slot [B], rate_counts [NW, E] and
        rate_z [NW, E] (absent otherwise: ``out.get("rate_hits")`` is None).
        With ranges configured (and only then) range_code int32 [B, R] (0 =
        nothing, 1 = below, 2 = above, 3 = not a number) and range_value f64
        [B, R].

        ``n_valid`` and ``rate`` concern the event-rate stage alone, the one
        stage with stream state: only the first n_valid rows (default: all)
        enter its windows, and ``rate=False`` skips it, so the call neither
        moves that state nor reports rate alerts (a re-score of old lines)."""
        B = lines.shape[0]
        if B == 0:
            return {
                "event_id": torch.zeros(0, dtype=torch.int32, device=lines.device),
                "anomaly": torch.zeros(0, dtype=torch.bool, device=lines.device),
                "scores": torch.zeros(0, dtype=torch.float32, device=lines.device),
                "nv_unseen": None,
                "combo_unseen": None,
                "match": None,
                **(dict.fromkeys(self._RATE_KEYS)
                   if self.event_rate is not None else {}),
                **self._empty_range_out(lines.device),
            }
        # roctx-visible stage ranges (torch.cuda.nvtx maps to rocTracer
        # markers on ROCm — SURVEY.md §5.1 tracing requirement)
        _rng = torch.cuda.nvtx.range if lines.is_cuda else None
        if _rng:
            torch.cuda.nvtx.range_push("dmx::parse")
        match = self.matcher.match_packed(lines, line_len)
        if _rng:
            torch.cuda.nvtx.range_pop()

        n_train_left = max(0, self.config.train_lines - self.seen_lines)
        train_upto = min(B, n_train_left)
        self.seen_lines += B

        # without event_rate the result holds exactly the keys it always
        # held; with it the four keys are there, None when the stage is
        # skipped (read them with .get())
        rate_out = (dict.fromkeys(self._RATE_KEYS)
                    if self.event_rate is not None else {})
        if self.event_rate is not None and rate:
            if _rng:
                torch.cuda.nvtx.range_push("dmx::event_rate")
            rate_out = self.event_rate.step(match["event_id"], n_valid, train_upto)
            if _rng:
                torch.cuda.nvtx.range_pop()

        # value ranges: rows below train_upto move lo / hi / n, every row is
        # judged against the state after them; the two keys exist only with
        # ranges configured
        range_out: Dict[str, torch.Tensor] = {}
        if self.value_ranges is not None:
            if _rng:
                torch.cuda.nvtx.range_push("dmx::value_range")
            code, value = self.value_ranges.step(lines, match, train_upto)
            range_out = {"range_code": code, "range_value": value}
            if _rng:
                torch.cuda.nvtx.range_pop()

        nv_unseen = None  # here [B, W + C]; split into its two views below
        W = self.specs.shape[0]
        if _rng:
            torch.cuda.nvtx.range_push("dmx::new_value")
        if self.hashsets is not None:
            if self.n_combos:
                hashes = ops.watch_combo_hashes(
                    lines, match, self.specs, self.members, self.combo_off,
                    self.config.lowercase)
            else:
                hashes = ops.watch_hashes(lines, match, self.specs, self.config.lowercase)
            if train_upto > 0:
                self.hashsets.insert(hashes[:train_upto])
            if train_upto == 0:
                # steady state: probe output IS the result (a zeros +
                # full-copy here cost 2 kernel launches per batch)
                nv_unseen = self.hashsets.probe(hashes)
            elif train_upto < B:
                unseen_tail = self.hashsets.probe(hashes[train_upto:])
                nv_unseen = torch.zeros(
                    (B, W + self.n_combos), dtype=torch.int32, device=lines.device
                )
                nv_unseen[train_upto:] = unseen_tail
            else:
                nv_unseen = torch.zeros(
                    (B, W + self.n_combos), dtype=torch.int32, device=lines.device
                )

        if _rng:
            torch.cuda.nvtx.range_pop()

        scores = torch.zeros(B, dtype=torch.float32, device=lines.device)
        if _rng:
            torch.cuda.nvtx.range_push("dmx::transformer")
        if self.model is not None:
            # content span comes straight from the match kernel
            # (span_start/span_end outputs — the former gather/where
            # chain here was ~6 kernel launches per batch, profiles/r10)
            if self.embedding_stats is not None:
                scores = self._embedding_scores(
                    lines, match["span_start"], match["span_end"], train_upto)
            else:
                scores = self.model.score_spans(
                    lines, match["span_start"], match["span_end"])
        if _rng:
            torch.cuda.nvtx.range_pop()

        anomaly = scores > self.config.score_threshold
        combo_unseen = None
        if nv_unseen is not None:
            # one reduction over watch and combination columns alike
            anomaly = anomaly | (nv_unseen.sum(dim=1) > 0)
            if self.n_combos:
                combo_unseen = nv_unseen[:, W:]
                nv_unseen = nv_unseen[:, :W] if W else None
        if rate_out.get("rate_hits") is not None:
            # non-zero only on a boundary line outside the training phase
            anomaly = anomaly | (rate_out["rate_hits"] > 0)
        if range_out:
            anomaly = anomaly | (range_out["range_code"] != 0).any(dim=1)
        return {
            "event_id": match["event_id"],
            "anomaly": anomaly,
            "scores": scores,
            "nv_unseen": nv_unseen,
            "combo_unseen": combo_unseen,
            "match": match,
            **rate_out,
            **range_out,
        }

    def _empty_range_out(self, device) -> Dict[str, torch.Tensor]:
        """The value-range keys of an empty batch ({} without ranges)."""
        if self.value_ranges is None:
            return {}
        R = self.value_ranges.R
        return {
            "range_code": torch.zeros((0, R), dtype=torch.int32, device=device),
            "range_value": torch.zeros((0, R), dtype=torch.float64, device=device),
        }

    def _embedding_scores(
        self, lines: torch.Tensor, start: torch.Tensor, end: torch.Tensor,
        train_upto: int,
    ) -> torch.Tensor:
        """score_mode "embedding": rows below train_upto update the moments
        and score 0, the rest score their distance. A batch that straddles
        the boundary takes a second launch on its tail; steady state is one
        distance-only launch."""
        stats = self.embedding_stats
        B = lines.shape[0]
        if train_upto > 0:
            stats.update(self.model.embed_spans(
                lines[:train_upto], start[:train_upto], end[:train_upto]))
        if train_upto == B or stats.n == 0:  # nothing fitted: no distance
            return torch.zeros(B, dtype=torch.float32, device=lines.device)
        if train_upto == 0:
            return self.model.embed_distance_spans(
                lines, start, end, stats.mu, stats.inv_var)
        scores = torch.zeros(B, dtype=torch.float32, device=lines.device)
        scores[train_upto:] = self.model.embed_distance_spans(
            lines[train_upto:], start[train_upto:], end[train_upto:],
            stats.mu, stats.inv_var)
        return scores

    def process_lines(self, raw_lines: Sequence[bytes]) -> Dict[str, torch.Tensor]:
        lines, lens = ops.pack_lines(raw_lines, self.config.max_len, device=self.device)
        return self.process_packed(lines, lens)

    # ------------------------------------------------------------------
    # hipGraph capture (HIP graphs for the launch-bound steady state —
    # SURVEY.md build mandate). Valid only AFTER the training phase: the
    # captured graph replays the detect-only path at fixed batch size.
    # ------------------------------------------------------------------
    def enable_graph(self, batch_size: int) -> bool:
        if self.device.type != "cuda":
            return False
        if self.seen_lines < self.config.train_lines:
            raise RuntimeError("enable_graph() requires the training phase done")
        B = batch_size
        static_lines = torch.zeros(
            (B, self.config.max_len), dtype=torch.uint8, device=self.device
        )
        static_lens = torch.zeros((B,), dtype=torch.int32, device=self.device)
        # warm up allocator/kernels on the same shapes, then capture. The
        # event-rate stage reads its row count from a device word: 0 makes
        # the warm-ups rewrite its state with the values it holds, and the
        # captured launches read whatever the word holds at replay.
        for _ in range(2):
            self.process_packed(static_lines, static_lens, n_valid=0)
            self.seen_lines -= B  # warmups must not advance stream state
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self.process_packed(static_lines, static_lens, n_valid=0)
        self.seen_lines -= B
        self._graph = graph
        self._graph_in = (static_lines, static_lens)
        self._graph_out = out
        return True

    def process_packed_graph(
        self, lines: torch.Tensor, lens: torch.Tensor
    ) -> Dict[str, torch.Tensor]:
        """Replay the captured graph on a new batch (same B, max_len)."""
        assert self._graph is not None, "call enable_graph() first"
        sl, sn = self._graph_in
        sl.copy_(lines, non_blocking=True)
        sn.copy_(lens, non_blocking=True)
        if self.event_rate is not None:
            self.event_rate.set_n_valid(lines.shape[0])
        self._graph.replay()
        self.seen_lines += lines.shape[0]
        return self._graph_out

    def process_packed_graph_partial(
        self, lines: torch.Tensor, lens: torch.Tensor
    ) -> Dict[str, torch.Tensor]:
        """Replay on a batch SMALLER than the captured size: pad rows get
        len 0 (their kernels no-op on the span but the transformer still
        runs them — acceptable when partial batches are rare stream
        edges). Outputs are sliced back to the true batch size."""
        assert self._graph is not None, "call enable_graph() first"
        sl, sn = self._graph_in
        B = lines.shape[0]
        assert B <= sl.shape[0]
        sl[:B].copy_(lines, non_blocking=True)
        sn[:B].copy_(lens, non_blocking=True)
        if B < sn.shape[0]:
            sn[B:].zero_()
        if self.event_rate is not None:
            # pad rows parse as unparsed lines; they must not be counted
            self.event_rate.set_n_valid(B)
        self._graph.replay()
        self.seen_lines += B

        def cut(v):
            if torch.is_tensor(v):
                return v[:B]
            if isinstance(v, dict):
                return {k: cut(x) for k, x in v.items()}
            return v

        return {k: (v if k in self._PER_SLOT_KEYS else cut(v))
                for k, v in self._graph_out.items()}
