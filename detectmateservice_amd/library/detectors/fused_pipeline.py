"""FusedPipelineDetector: the whole GPU pipeline as ONE service component.

Deployment collapse of parser→detector: LogSchema frames in, DetectorSchema
alerts out, with everything between — template matching, NewValue hash
probing, BERT-tiny scoring — running as the fused GPU pipeline
(detectmateservice_amd.pipeline.GpuPipeline) on device tensors. The C++
batched codec decodes frames straight into the packed SoA buffer; Python
objects are built only for the (rare) alert frames.

This is the highest-throughput single-service deployment (config:
``detectors: {FusedPipelineDetector: {...}}`` mirrors PipelineConfig).
"""
from __future__ import annotations

import time
from typing import Any, Dict, List, Optional

import torch

from ...components.base import CoreComponent, CoreConfig
from ...schemas import DetectorSchema, LogSchema
from ... import ops
from ...pipeline import GpuPipeline, PipelineConfig


class FusedPipelineDetectorConfig(CoreConfig):
    method_type: str = "fused_pipeline_detector"
    templates: List[str] = []
    path_templates: Optional[str] = None
    log_format: Optional[str] = None
    lowercase: bool = False
    max_len: int = 256
    #: [{kind: variable|header, pos: int, event: int}]
    watches: List[Dict[str, Any]] = []
    #: combinations of fields, each a list of members written like watches;
    #: a line whose tuple of member values is new alerts (one more hash
    #: table of hashset_capacity slots per combination)
    combos: List[List[Dict[str, Any]]] = []
    hashset_capacity: int = 1 << 16
    use_transformer: bool = True
    score_threshold: float = 3.0
    #: "head": the model's score head. "embedding": distance from the
    #: Gaussian fitted to the embeddings of the data_use_training rows.
    score_mode: str = "head"
    data_use_training: int = 0
    #: event-rate windows: {window_lines, ewma_alpha, z_threshold,
    #: min_windows}, FrequencyDetector's keys and defaults ({} = defaults).
    #: The line that completes a window alerts when an event's count in it
    #: is z_threshold sigmas off its EWMA baseline. None = off.
    event_rate: Optional[Dict[str, Any]] = None
    #: numeric value ranges: [{kind, pos, event, name, slack, non_numeric,
    #: min, max}], the first three as in watches. The field is read as a
    #: decimal number; its smallest and largest value over the
    #: data_use_training rows (or min / max) bound what is normal later.
    ranges: List[Dict[str, Any]] = []
    device: Optional[str] = None
    seed: int = 1234
    #: capture the detect path as ONE hipGraph at this batch size (0 = off).
    #: Smaller batches replay padded; set to the engine batch size.
    graph_batch: int = 0
    #: BASELINE config 5: retain every ingested packed batch in the
    #: capacity-managed HBM line buffer. 0 = off; -1 = size from free
    #: device memory (>500M resident 256-byte lines on a 288 GB part);
    #: >0 = byte budget. History is re-scorable via rescore_window()
    #: (admin: POST /admin/rescore).
    line_buffer_bytes: int = 0


class FusedPipelineDetector(CoreComponent):
    CONFIG_CLASS = FusedPipelineDetectorConfig

    def __init__(self, config=None) -> None:
        super().__init__(config)
        cfg = self.config
        templates = list(cfg.templates or [])
        if cfg.path_templates:
            with open(cfg.path_templates, "r", encoding="utf-8") as fh:
                templates.extend(l.rstrip("\n") for l in fh if l.strip())
        device = cfg.device or ("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(device)
        self.pipe = GpuPipeline(
            PipelineConfig(
                templates=templates,
                log_format=cfg.log_format,
                lowercase=cfg.lowercase,
                max_len=cfg.max_len,
                watches=list(cfg.watches or []),
                combos=[list(c) for c in (cfg.combos or [])],
                hashset_capacity=cfg.hashset_capacity,
                use_transformer=cfg.use_transformer,
                score_threshold=cfg.score_threshold,
                score_mode=cfg.score_mode,
                train_lines=cfg.data_use_training,
                event_rate=(dict(cfg.event_rate)
                            if cfg.event_rate is not None else None),
                ranges=[dict(r) for r in (cfg.ranges or [])],
                seed=cfg.seed,
            ),
            device=self.device,
        )
        self.detector_id = f"fused_pipeline-{id(self):x}"
        self.line_buffer = None
        if cfg.line_buffer_bytes:
            from ...line_buffer import GpuLineBuffer

            kw = ({"budget_fraction": 0.5} if cfg.line_buffer_bytes < 0
                  else {"budget_bytes": cfg.line_buffer_bytes})
            self.line_buffer = GpuLineBuffer(
                max_len=cfg.max_len, device=self.device, **kw)

    def process(self, data: bytes) -> Optional[bytes]:
        return self.process_batch([data])[0]

    # -- packed data plane (engine_packed_mode) ------------------------
    def packed_max_len(self) -> int:
        return int(self.config.max_len)

    def packed_pin_memory(self) -> bool:
        import os as _os

        # DMX_PACKED_PIN=0 disables pinned staging (A/B: pinned-cache
        # event syncs vs pageable H2D)
        if _os.environ.get("DMX_PACKED_PIN") == "0":
            return False
        return self.device.type == "cuda"

    def rescore_window(self, lines_back: int,
                       threshold: Optional[float] = None) -> Dict[str, Any]:
        """Re-score the newest ``lines_back`` resident lines of the HBM
        line buffer — post-hoc analysis with a NEW threshold (or model
        state) at HBM bandwidth, the config-5 use case. Returns summary
        counts (the alert path stays with the live stream). The event-rate
        stage is skipped: old lines belong to no window of the live stream,
        so its state stays as it is and no rate alert is counted."""
        if self.line_buffer is None:
            return {"rescored": 0, "reason": "line buffer disabled"}
        lines, lens = self.line_buffer.window(lines_back)
        if lines.shape[0] == 0:
            return {"rescored": 0, "anomalies": 0}
        old_thr = self.pipe.config.score_threshold
        if threshold is not None:
            self.pipe.config.score_threshold = float(threshold)
        try:
            seen = self.pipe.seen_lines  # rescoring must not advance
            # force detect mode: a rescore during the training phase must
            # not INSERT window values into the live hash sets
            self.pipe.seen_lines = max(seen, self.pipe.config.train_lines)
            out = self.pipe.process_packed(lines, lens, rate=False)
        finally:
            self.pipe.seen_lines = seen
            self.pipe.config.score_threshold = old_thr
        n = int(lines.shape[0])
        return {
            "rescored": n,
            "anomalies": int(out["anomaly"].sum()),
            "score_mean": float(out["scores"].float().mean()),
            "score_max": float(out["scores"].float().max()),
            "watermark": self.line_buffer.watermark(),
        }

    def _score_packed(self, lines: torch.Tensor, lens: torch.Tensor):
        """Run the pipeline (graph replay when enabled) on a CPU-packed
        batch; returns the output dict."""
        gb = self.config.graph_batch
        if (gb > 0 and self.device.type == "cuda"
                and self.pipe.seen_lines >= self.config.data_use_training
                and lines.shape[0] <= gb):
            if self.pipe._graph is None:
                self.pipe.enable_graph(gb)
            if self.line_buffer is not None:
                self.line_buffer.append(lines.to(self.device, non_blocking=True),
                                        lens.to(self.device, non_blocking=True))
            return self.pipe.process_packed_graph_partial(lines, lens)
        dl = lines.to(self.device, non_blocking=True)
        dn = lens.to(self.device, non_blocking=True)
        if self.line_buffer is not None:
            self.line_buffer.append(dl, dn)
        return self.pipe.process_packed(dl, dn)

    def _alerts(self, out, id_of) -> List:
        """[(idx, DetectorSchema bytes)] for anomalous rows; ``id_of(i)``
        resolves a row's logID lazily (alerts are rare)."""
        anomaly = out["anomaly"]
        if not bool(anomaly.any()):
            return []
        idxs = torch.nonzero(anomaly, as_tuple=False).flatten().cpu().tolist()
        scores = out["scores"].float().cpu()
        nv = out["nv_unseen"].cpu() if out["nv_unseen"] is not None else None
        combo = out.get("combo_unseen")
        combo = combo.cpu() if combo is not None else None
        rate_hits = out.get("rate_hits")
        rate_hits = rate_hits.cpu() if rate_hits is not None else None
        range_code = out.get("range_code")
        range_code = range_code.cpu() if range_code is not None else None
        now = int(time.time())
        alerts = []
        for i in idxs:
            reasons = []
            if nv is not None and int(nv[i].sum()) > 0:
                reasons.append("unknown watched value")
            if combo is not None and int(combo[i].sum()) > 0:
                reasons.append("unknown combination")
            if rate_hits is not None and int(rate_hits[i]) > 0:
                reasons.append(self._rate_reason(out, i))
            if range_code is not None and bool(range_code[i].any()):
                reasons.extend(self._range_reasons(out, range_code, i))
            if (self.pipe.model is not None
                    and float(scores[i]) > self.config.score_threshold):
                what = ("embedding distance"
                        if self.pipe.embedding_stats is not None else "score")
                reasons.append(f"{what} {float(scores[i]):.3f}")
            lid = id_of(i)
            alerts.append((i, DetectorSchema(
                detectorID=self.detector_id,
                detectorType="fused_pipeline_detector",
                alertID=f"fp-{lid}",
                detectionTimestamp=now,
                logIDs=[lid] if lid else [],
                score=float(scores[i]),
                description="Anomaly: " + "; ".join(reasons),
            ).serialize()))
        return alerts

    @staticmethod
    def _rate_reason(out, i: int) -> str:
        """"event rate: event 3: 950/window (z=+12.3); ..." for boundary row
        i: the flagged bins of the window that row completed."""
        slot = int(out["rate_slot"][i])
        counts = out["rate_counts"][slot].cpu()
        z = out["rate_z"][slot].cpu()
        parts = []
        for e in torch.nonzero(z, as_tuple=False).flatten().tolist():
            who = "unparsed" if e == 0 else f"event {e}"
            parts.append(f"{who}: {int(counts[e])}/window (z={float(z[e]):+.1f})")
        return "event rate: " + "; ".join(parts)

    def _range_reasons(self, out, range_code, i: int) -> List[str]:
        """"value out of range: bytes = 18234511 above [0, 1048576]" or "not
        a number: bytes" for every flagged range of row i. The bounds are
        read from the device state here, when an alert is worded, and
        nowhere on the hot path."""
        state = self.pipe.value_ranges
        lo, hi = state.lo.cpu(), state.hi.cpu()
        reasons = []
        for r in torch.nonzero(range_code[i], as_tuple=False).flatten().tolist():
            code, name = int(range_code[i, r]), state.names[r]
            if code == 3:
                reasons.append(f"not a number: {name}")
                continue
            side = "below" if code == 1 else "above"
            reasons.append(
                f"value out of range: {name} = {float(out['range_value'][i, r]):.15g} "
                f"{side} [{float(lo[r]):.15g}, {float(hi[r]):.15g}]")
        return reasons

    def process_packed_frames(self, lines, lens, ids_blob, ids_off) -> List:
        """Engine packed-loop entry: tensors in (already decoded by the
        C++ socket reader), [(idx, alert bytes)] out."""
        if lines.shape[0] == 0:
            return []
        out = self._score_packed(lines, lens)
        return self._alerts(
            out,
            lambda i: ids_blob[int(ids_off[i]):int(ids_off[i + 1])].decode(
                "utf-8", "replace"),
        )

    # -- pipelined packed path (submit/collect) ------------------------
    # The engine overlaps batch N's GPU work with batch N+1's recv+decode:
    # submit launches the pipeline WITHOUT synchronizing; collect performs
    # the one device sync (anomaly readback) and builds the alerts.
    def submit_packed_frames(self, lines, lens, ids_blob, ids_off):
        if lines.shape[0] == 0:
            return None
        out = self._score_packed(lines, lens)  # async: kernels queued
        if self.pipe._graph is not None:
            # graph replay writes into STATIC buffers: clone (async) so
            # the next submit's replay can't clobber this batch's outputs
            out = {
                k: (v.clone() if torch.is_tensor(v) else v)
                for k, v in out.items() if k != "match"
            }
        # keep `lines` alive until the async H2D copy completes (the
        # pinned block would otherwise return to the cache mid-copy)
        return (out, ids_blob, ids_off, lines)

    def collect_packed_frames(self, token) -> List:
        if token is None:
            return []
        out, ids_blob, ids_off, _lines = token
        return self._alerts(
            out,
            lambda i: ids_blob[int(ids_off[i]):int(ids_off[i + 1])].decode(
                "utf-8", "replace"),
        )

    def process_batch(self, frames: List[bytes]) -> List[Optional[bytes]]:
        if not frames:
            return []
        import os as _os
        _stats = _os.environ.get("DMX_ENGINE_STATS") == "1"
        _t0 = time.perf_counter() if _stats else 0.0
        if ops.have_extension():
            from ...ops import _dmx_C  # type: ignore[attr-defined]

            # packed decode: GIL-released parse, ONE ids blob instead of
            # B py::bytes, pinned lines buffer for async H2D (fp-stats
            # showed the py-object path at ~20 ms/8192 under GIL pressure)
            lines, lens, ids_blob, ids_off = _dmx_C.decode_log_batch_packed(
                list(frames), self.config.max_len,
                self.device.type == "cuda",
            )
            log_ids_raw = (ids_blob, ids_off)
            log_ids = None  # decoded lazily, only for alert frames
        else:
            logs = [LogSchema.deserialize(f) for f in frames]
            lines, lens = ops.pack_lines(
                [(l.log or "").encode() for l in logs], self.config.max_len
            )
            log_ids_raw = None
            log_ids = [l.logID for l in logs]
        _t1 = time.perf_counter() if _stats else 0.0
        out = self._score_packed(lines, lens)
        if _stats:
            if out["anomaly"].is_cuda:
                torch.cuda.synchronize()
            _t2 = time.perf_counter()
            self._stat_acc = getattr(self, "_stat_acc", [0, 0.0, 0.0])
            self._stat_acc[0] += 1
            self._stat_acc[1] += _t1 - _t0
            self._stat_acc[2] += _t2 - _t1
            if self._stat_acc[0] % 16 == 0:
                import logging as _logging
                _logging.getLogger(__name__).info(
                    "[fp-stats] decode %.2fms/b gpu %.2fms/b",
                    self._stat_acc[1] * 1e3 / self._stat_acc[0],
                    self._stat_acc[2] * 1e3 / self._stat_acc[0],
                )
        if log_ids is None:
            blob, off = log_ids_raw
            id_of = lambda i: blob[int(off[i]):int(off[i + 1])].decode(  # noqa: E731
                "utf-8", "replace")
        else:
            id_of = lambda i: log_ids[i]  # noqa: E731
        results: List[Optional[bytes]] = [None] * len(frames)
        for i, alert in self._alerts(out, id_of):
            results[i] = alert
        return results

    # -- checkpoint -----------------------------------------------------
    def dist_sync(self, group=None) -> None:
        """COLLECTIVE merge of the data-parallel GPU hash sets (one
        batched insert-kernel call per peer table —
        parallel/dist.py::all_reduce_hashsets). Event-rate state is left
        alone: each rank judges the rate of its own shard of the stream.
        Value ranges are merged: lo by MIN, hi by MAX, n by SUM."""
        import torch.distributed as tdist

        if not tdist.is_initialized() or tdist.get_world_size(group) <= 1:
            return
        self._sync_value_ranges(group)
        if self.pipe.hashsets is None:
            return
        hs = self.pipe.hashsets
        if hasattr(hs, "tables"):  # GPU open-addressing tables
            from ...parallel import dist as dmx_dist

            dmx_dist.all_reduce_hashsets(hs.tables, group=group)
        else:  # CPU fallback keeps Python sets
            world = tdist.get_world_size(group)
            local = [sorted(s) for s in hs.sets]
            gathered: list = [None] * world
            tdist.all_gather_object(gathered, local, group=group)
            me = tdist.get_rank(group)
            for r, other in enumerate(gathered):
                if r == me or not other:
                    continue
                for w, values in enumerate(other):
                    hs.sets[w].update(values)

    def _sync_value_ranges(self, group=None) -> None:
        """COLLECTIVE: every rank ends with the smallest lo, the largest hi
        and the summed n of all ranks, written into the tensors the kernels
        (and a captured graph) read."""
        import torch.distributed as tdist

        state = self.pipe.value_ranges
        if state is None:
            return
        lo, hi, n = state.lo.clone(), state.hi.clone(), state.n.clone()
        tdist.all_reduce(lo, op=tdist.ReduceOp.MIN, group=group)
        tdist.all_reduce(hi, op=tdist.ReduceOp.MAX, group=group)
        tdist.all_reduce(n, op=tdist.ReduceOp.SUM, group=group)
        state.merge_(lo, hi, n - state.n)  # n: the other ranks' share

    def state_dict(self) -> Dict[str, Any]:
        state: Dict[str, Any] = {"seen_lines": self.pipe.seen_lines}
        if self.pipe.hashsets is not None:
            state["hashsets"] = self.pipe.hashsets.state_dict()
        if self.pipe.model is not None:
            state["model"] = self.pipe.model.state_dict()
        if self.pipe.embedding_stats is not None:
            state["embedding_stats"] = self.pipe.embedding_stats.state_dict()
        if self.pipe.event_rate is not None:
            state["event_rate"] = self.pipe.event_rate.state_dict()
        if self.pipe.value_ranges is not None:
            state["value_ranges"] = self.pipe.value_ranges.state_dict()
        return state

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self.pipe.seen_lines = int(state.get("seen_lines", 0))
        if "hashsets" in state and self.pipe.hashsets is not None:
            self.pipe.hashsets.load_state_dict(state["hashsets"])
        if "model" in state and self.pipe.model is not None:
            self.pipe.model.load_state_dict(state["model"])
        if "embedding_stats" in state and self.pipe.embedding_stats is not None:
            self.pipe.embedding_stats.load_state_dict(state["embedding_stats"])
        if "event_rate" in state and self.pipe.event_rate is not None:
            self.pipe.event_rate.load_state_dict(state["event_rate"])
        if "value_ranges" in state and self.pipe.value_ranges is not None:
            self.pipe.value_ranges.load_state_dict(state["value_ranges"])
