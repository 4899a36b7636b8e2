"""EventSequenceDetector: n-gram anomaly detection over the order of events.

The oldest log-anomaly signal: a session that runs a command before it was
opened, a step of a job that is skipped. Every line is a symbol, its
``EventID``; the lines that share a key (a session id, a pid; no key = the
whole stream) form a sequence, and each line completes an n-gram of the last
``length`` symbols of its key, padded on the left while the key is young.
During the first ``data_use_training`` lines the grams are learnt; afterwards
a gram never seen alerts. docs/kernels.md, "Event sequences", is the
definition; this class applies it per frame on ``ParserSchema`` with exact
keys in a dict, the fused pipeline's ``event_sequence:`` key applies it on the
device with hashed keys in buckets (``ops/csrc/event_sequence.hip``).

Config::

    detectors:
      EventSequenceDetector:
        data_use_training: 10000
        length: 3
        key: {kind: header, pos: Session, name: ses}

``key`` takes ``kind`` (``variable`` | ``header``), ``pos`` (an index into
``variables`` or a name in ``logFormatVariables``), and the optional ``event``
(the field exists only on lines of that event) and ``name`` (alert wording).
A line whose EventID is below 1 or whose key field is absent belongs to no
sequence: it neither alerts nor moves a history.
"""
from __future__ import annotations

import time
from typing import Any, Dict, Optional, Set, Tuple

from pydantic import ConfigDict

from ... import ops
from ...components.base import CoreDetector, CoreDetectorConfig
from ...schemas import DetectorSchema, ParserSchema
from .new_value import _WatchSpec

_KEY_KEYS = ("kind", "pos", "event", "name")


class EventSequenceDetectorConfig(CoreDetectorConfig):
    model_config = ConfigDict(extra="allow", populate_by_name=True)

    method_type: str = "event_sequence_detector"
    #: n, 2 .. ops.SEQ_MAX_LEN: events per gram
    length: int = 3
    #: the field that names a sequence; None = the stream is one sequence
    key: Optional[Dict[str, Any]] = None


class EventSequenceDetector(CoreDetector):
    CONFIG_CLASS = EventSequenceDetectorConfig

    def __init__(self, config=None) -> None:
        super().__init__(config)
        self.length = int(self.config.length)
        if not 2 <= self.length <= ops.SEQ_MAX_LEN:
            raise ValueError(
                f"length must be within 2 .. {ops.SEQ_MAX_LEN}, got {self.length}")
        key = self.config.key
        self.key_spec: Optional[_WatchSpec] = None
        self.key_name: Optional[str] = None
        if key is not None:
            unknown = set(key) - set(_KEY_KEYS)
            if unknown:
                raise ValueError(
                    f"key: unknown key(s) {sorted(unknown)}; valid keys: "
                    f"{sorted(_KEY_KEYS)}")
            if "pos" not in key:
                raise ValueError(f"key has no 'pos': {dict(key)!r}")
            kind = key.get("kind", "variable")
            if kind not in ("variable", "header"):
                raise ValueError(
                    f"key: 'kind' must be 'variable' or 'header', got {kind!r}")
            event = int(key.get("event", -1))
            self.key_spec = _WatchSpec(
                "Global" if event < 0 else f"Event {event}",
                None if event < 0 else event, kind, key["pos"], key.get("name"))
            self.key_name = key.get("name")
        #: key value -> the key's last length - 1 event ids, oldest first
        self.history: Dict[str, Tuple[int, ...]] = {}
        self.known: Set[Tuple[int, ...]] = set()
        self.detector_id = f"event_sequence_detector-{id(self):x}"

    def _advance(self, parsed: ParserSchema) -> Optional[Tuple[int, ...]]:
        """Move the history of the line's key and return the gram the line
        completes, or None when the line belongs to no sequence."""
        event = parsed.EventID
        if event is None or not 1 <= int(event) <= ops.SEQ_MAX_EVENTS:
            return None
        spec = self.key_spec
        if spec is None:
            key = ""
        else:
            # a content variable scoped to an event exists on that event only
            if (spec.kind == "variable" and spec.event_id is not None
                    and spec.event_id != int(event)):
                return None
            key = spec.extract(parsed)
            if key is None:
                return None
        pad = (0,) * (self.length - 1)
        gram = self.history.get(key, pad) + (int(event),)
        self.history[key] = gram[1:]
        return gram

    def train(self, parsed_batch) -> None:
        for parsed in parsed_batch:
            gram = self._advance(parsed)
            if gram is not None:
                self.known.add(gram)

    def detect(self, parsed: ParserSchema, alert: DetectorSchema) -> bool:
        gram = self._advance(parsed)
        if gram is None or gram in self.known:
            return False
        alert.detectorID = self.detector_id
        alert.detectorType = "event_sequence_detector"
        alert.alertID = f"seq-{parsed.logID or parsed.parsedLogID}"
        alert.detectionTimestamp = int(time.time())
        alert.logIDs = [parsed.logID] if parsed.logID else []
        alert.score = 1.0
        alert.description = ops.sequence_text(gram, self.key_name)
        return True

    # -- data-parallel state merge (dist_mode "dp") --------------------
    def dist_sync(self, group=None) -> None:
        """COLLECTIVE union of every rank's learnt grams. The histories stay
        per rank: a key's lines must reach one rank for its sequence to mean
        anything."""
        import torch.distributed as tdist

        if not tdist.is_initialized() or tdist.get_world_size(group) <= 1:
            return
        gathered: list = [None] * tdist.get_world_size(group)
        tdist.all_gather_object(gathered, sorted(self.known), group=group)
        for other in gathered:
            self.known.update(tuple(g) for g in other or [])

    # -- checkpoint/resume ---------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        return {
            "seen_lines": self._seen_lines,
            "length": self.length,
            "known": sorted(list(g) for g in self.known),
            "history": {k: list(v) for k, v in self.history.items()},
        }

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        if int(state.get("length", self.length)) != self.length:
            raise ValueError(
                f"event-sequence checkpoint was taken with length = "
                f"{int(state['length'])} but this instance is configured for "
                f"{self.length}")
        self._seen_lines = int(state.get("seen_lines", 0))
        self.known = {tuple(int(s) for s in g) for g in state.get("known") or []}
        self.history = {k: tuple(int(s) for s in v)
                        for k, v in (state.get("history") or {}).items()}
