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
    #: event sequences: {length, key, max_keys, capacity}. A line alerts
    #: when the n-gram of event ids it completes in the history of its key
    #: (a field written like a watch, e.g. the session id; no key = the
    #: whole stream) never occurred in the data_use_training rows. None = off.
    event_sequence: Optional[Dict[str, Any]] = None
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


def _id_of(ids_blob, ids_off):
    """i -> logID of row i, decoded lazily from the packed ids (alerts are
    rare)."""
    return lambda i: ids_blob[int(ids_off[i]):int(ids_off[i + 1])].decode(
        "utf-8", "replace")


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
                event_sequence=(dict(cfg.event_sequence)
                                if cfg.event_sequence is not None else None),
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
        and event-sequence stages are skipped: old lines belong to no window
        and no history of the live stream, so their state stays as it is and
        none of their alerts is counted."""
        if self.line_buffer is None:
            return {"rescored": 0, "reason": "line buffer disabled"}
        lines, lens = self.line_buffer.window(lines_back)
        if lines.shape[0] == 0:
            return {"rescored": 0, "anomalies": 0}
        # detect mode whatever the phase: a rescore during the training phase
        # must not INSERT window values into the live hash sets
        out = self.pipe.rescore(lines, lens, threshold)
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
            if not self.pipe.graph_enabled:
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
        # each stage's own keys move to the host once per alerting batch
        host = {"scores": scores}
        host.update((k, out[k].cpu()) for s in self.pipe.stages for k in s.keys
                    if out.get(k) is not None)
        now = int(time.time())
        alerts = []
        for i in idxs:
            reasons = [r for s in self.pipe.stages for r in s.reasons(host, i)]
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

    def process_packed_frames(self, lines, lens, ids_blob, ids_off) -> List:
        """Engine packed-loop entry: tensors in (already decoded by the
        C++ socket reader), [(idx, alert bytes)] out."""
        if lines.shape[0] == 0:
            return []
        return self._alerts(self._score_packed(lines, lens), _id_of(ids_blob, ids_off))

    # -- pipelined packed path (submit/collect) ------------------------
    # The engine overlaps batch N's GPU work with batch N+1's recv+decode:
    # submit launches the pipeline WITHOUT synchronizing; collect performs
    # the one device sync (anomaly readback) and builds the alerts.
    def submit_packed_frames(self, lines, lens, ids_blob, ids_off):
        if lines.shape[0] == 0:
            return None
        out = self._score_packed(lines, lens)  # async: kernels queued
        if self.pipe.graph_enabled:
            # graph replay writes into STATIC buffers: clone (async) so
            # the next submit's replay can't clobber this batch's outputs
            out = {k: (v.clone() if torch.is_tensor(v) else v)
                   for k, v in out.items() if k != "match"}
        # keep `lines` alive until the async H2D copy completes (the
        # pinned block would otherwise return to the cache mid-copy)
        return (out, ids_blob, ids_off, lines)

    def collect_packed_frames(self, token) -> List:
        if token is None:
            return []
        out, ids_blob, ids_off, _lines = token
        return self._alerts(out, _id_of(ids_blob, ids_off))

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
            id_of = _id_of(ids_blob, ids_off)
        else:
            logs = [LogSchema.deserialize(f) for f in frames]
            lines, lens = ops.pack_lines(
                [(l.log or "").encode() for l in logs], self.config.max_len
            )
            id_of = [l.logID for l in logs].__getitem__
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
        results: List[Optional[bytes]] = [None] * len(frames)
        for i, alert in self._alerts(out, id_of):
            results[i] = alert
        return results

    # -- checkpoint: the pipeline owns the state ---------------------------
    def dist_sync(self, group=None) -> None:
        """COLLECTIVE merge of the data-parallel stage state."""
        self.pipe.dist_sync(group)

    def state_dict(self) -> Dict[str, Any]:
        return self.pipe.state_dict()

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self.pipe.load_state_dict(state)
