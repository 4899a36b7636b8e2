"""EmbeddingDetector: transformer-embedding distance anomaly detection.

The reference library family carries embedding/LLM-assisted detection
(its dependency set includes tiktoken/openai — SURVEY.md §2.2 "capability
hints"). MI355X-native rebuild: log lines are embedded with the BERT-tiny
byte transformer (mean-pooled hidden state, bf16 MFMA kernels); training
fits a diagonal Gaussian over embeddings; detection flags lines whose
normalized distance

    d(x) = sqrt(mean_i ((x_i - mu_i)^2 / (var_i + eps)))

exceeds ``z_threshold``. Fully checkpointable (weights + moments).

``embed_path`` picks how a batch is embedded. ``"layered"`` (default) runs
the per-op transformer body and does the moments and the distance on the
host. ``"fused"`` keeps everything on the device: training batches go
through ``BertTinyDetectorModel.embed_spans`` into device-resident
``EmbeddingStats``, a detect batch is one ``embed_distance_spans`` call (on
a GPU with the flagship geometry, one launch of the fused kernel's distance
head), the threshold compare runs there too, and only the alerting rows and
their distances are read back. Where the fused kernel does not apply the
model falls back to its layered body; the path never raises for that.
"""
from __future__ import annotations

import time
from typing import Any, Dict, List, Optional

import torch

from ...components.base import CoreDetector, CoreDetectorConfig
from ...models.bert_tiny import (
    BertTinyConfig,
    BertTinyDetectorModel,
    EmbeddingStats,
    embedding_distance,
)
from ...schemas import DetectorSchema, ParserSchema
from ... import ops


class EmbeddingDetectorConfig(CoreDetectorConfig):
    method_type: str = "embedding_detector"
    z_threshold: float = 4.0
    max_seq: int = 64
    hidden: int = 128
    layers: int = 2
    heads: int = 2
    ffn: int = 512
    device: Optional[str] = None
    seed: int = 1234
    batch_max_len: int = 256
    #: "layered": per-op body, host moments and distance. "fused": device
    #: end to end through the fused kernel's embedding / distance head.
    embed_path: str = "layered"


class EmbeddingDetector(CoreDetector):
    CONFIG_CLASS = EmbeddingDetectorConfig

    def __init__(self, config=None) -> None:
        super().__init__(config)
        cfg = self.config
        self.device = torch.device(
            cfg.device or ("cuda" if torch.cuda.is_available() else "cpu")
        )
        self.model = BertTinyDetectorModel(
            BertTinyConfig(hidden=cfg.hidden, layers=cfg.layers,
                           heads=cfg.heads, ffn=cfg.ffn, max_seq=cfg.max_seq),
            device=self.device, seed=cfg.seed,
        )
        self.detector_id = f"embedding_detector-{id(self):x}"
        if cfg.embed_path not in ("layered", "fused"):
            raise ValueError(
                f"embed_path must be 'layered' or 'fused', got {cfg.embed_path!r}")
        self._fused = cfg.embed_path == "fused"
        # the layered path keeps its moments on the host, where it embeds to
        self.stats = EmbeddingStats(
            cfg.hidden, device=self.device if self._fused else "cpu")

    # the moments, under the names they had before EmbeddingStats held them
    @property
    def _sum(self) -> torch.Tensor:
        return self.stats.sum

    @property
    def _sumsq(self) -> torch.Tensor:
        return self.stats.sumsq

    @property
    def _n(self) -> int:
        return self.stats.n

    # ------------------------------------------------------------------
    def _pack(self, raw_lines: List[bytes]):
        """(lines, start, end) on the device: the whole line is the span."""
        lines, lens = ops.pack_lines(
            raw_lines, self.config.batch_max_len, device=self.device
        )
        start = torch.zeros(len(raw_lines), dtype=torch.int32, device=self.device)
        return lines, start, lens.int()

    def embed(self, raw_lines: List[bytes]) -> torch.Tensor:
        """Mean-pooled transformer embeddings [B, hidden] (f32), on the host.
        Always the layered body, whatever ``embed_path`` says."""
        lines, start, end = self._pack(raw_lines)
        tokens = self.model.tokenize_spans(lines, start, end)
        return self.model._encode(tokens).float().mean(dim=1).cpu()

    def train(self, parsed_batch: List[ParserSchema]) -> None:
        raw = [(p.log or "").encode() for p in parsed_batch]
        if self._fused:
            self.stats.update(self.model.embed_spans(*self._pack(raw)))
        else:
            self.stats.update(self.embed(raw))

    def _distance(self, emb: torch.Tensor) -> torch.Tensor:
        if self._fused:
            return embedding_distance(
                emb.to(self.stats.device), self.stats.mu, self.stats.inv_var)
        n = max(self._n, 1)
        mu = (self._sum / n).float()
        var = (self._sumsq / n).float() - mu ** 2
        z2 = (emb - mu) ** 2 / (var.clamp(min=1e-6))
        return z2.mean(dim=1).sqrt()

    def _alerting(self, raw_lines: List[bytes]) -> List[tuple]:
        """[(row, distance)] of the lines beyond the threshold."""
        thr = float(self.config.z_threshold)
        if not self._fused:
            dist = self._distance(self.embed(raw_lines))
            return [(j, d) for j, d in enumerate(dist.tolist()) if not d <= thr]
        dist = self.model.embed_distance_spans(
            *self._pack(raw_lines), self.stats.mu, self.stats.inv_var)
        rows = torch.nonzero(dist > thr).flatten()
        # one readback: row numbers and distances, both exact in f64
        both = torch.cat([rows.double(), dist[rows].double()]).cpu()
        k = rows.numel()
        return list(zip((int(r) for r in both[:k].tolist()), both[k:].tolist()))

    def process_batch(self, frames: List[bytes]) -> List[Optional[bytes]]:
        parsed = [ParserSchema.deserialize(f) for f in frames]
        results: List[Optional[bytes]] = [None] * len(frames)
        n_train = int(self.config.data_use_training)
        train_upto = 0
        if self._seen_lines < n_train:
            train_upto = min(len(parsed), n_train - self._seen_lines)
            self.train(parsed[:train_upto])
        self._seen_lines += len(parsed)
        rest = parsed[train_upto:]
        if not rest or self._n == 0:
            return results
        now = int(time.time())
        thr = float(self.config.z_threshold)
        for j, d in self._alerting([(p.log or "").encode() for p in rest]):
            p = rest[j]
            results[train_upto + j] = DetectorSchema(
                detectorID=self.detector_id,
                detectorType="embedding_detector",
                alertID=f"emb-{p.logID or p.parsedLogID}",
                detectionTimestamp=now,
                logIDs=[p.logID] if p.logID else [],
                score=float(d),
                description=f"Embedding distance {d:.3f} > {thr:.3f}",
            ).serialize()
        return results

    def detect(self, parsed, alert) -> bool:
        out = self.process_batch([parsed.serialize()])
        if out[0] is None:
            return False
        got = DetectorSchema.deserialize(out[0])
        for f in alert.FIELDS:
            setattr(alert, f, getattr(got, f))
        return True

    def state_dict(self) -> Dict[str, Any]:
        return {
            "seen_lines": self._seen_lines,
            **self.stats.state_dict(),  # sum, sumsq (CPU f64), n
            "model": self.model.state_dict(),
        }

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self._seen_lines = int(state.get("seen_lines", 0))
        self.stats.load_state_dict(state)
        self.model.load_state_dict(state["model"])
