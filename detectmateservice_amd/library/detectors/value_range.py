"""ValueRangeDetector: numeric value-range anomaly detection.

The classic range detector for fields that are numbers (``bytes=18234511``,
``duration=0.731``, ``status=503``): during the first ``data_use_training``
lines the smallest and largest value of each configured field are learnt;
afterwards a value outside ``[lo - slack * (hi - lo), hi + slack * (hi - lo)]``
alerts. docs/kernels.md, "Value ranges", is the definition (grammar, value,
fit, judge); this class applies it per frame on ``ParserSchema``, the fused
pipeline's ``ranges:`` key applies it on the device
(``ops/csrc/value_range.hip``), and ``ops.value_range_step_cpu`` is the
mirror both are tested against.

Config, in the block shape of NewValueDetector::

    detectors:
      ValueRangeDetector:
        data_use_training: 10000
        global:
          inst:
            header_variables: [{pos: Status, min: 100, max: 599}]
        events:
          3:
            inst:
              variables: [{pos: 2, name: bytes, slack: 0.1,
                           non_numeric: alert}]

A field entry takes ``pos`` and the optional ``name``, ``slack`` (>= 0,
default 0), ``non_numeric`` (``ignore`` | ``alert``) and ``min`` / ``max``
(both or neither). As in NewValueDetector a block under ``events`` applies to
that event only, header variables included.
"""
from __future__ import annotations

import time
from typing import Any, Dict, List, Optional

from pydantic import ConfigDict, Field

from ... import ops
from ...components.base import CoreDetector, CoreDetectorConfig
from ...schemas import DetectorSchema, ParserSchema
from .new_value import _WatchSpec

_FIELD_KEYS = ("pos", "name", "slack", "non_numeric", "min", "max")


class ValueRangeDetectorConfig(CoreDetectorConfig):
    model_config = ConfigDict(extra="allow", populate_by_name=True)

    method_type: str = "value_range_detector"
    #: instance_name -> {"variables": [...], "header_variables": [...]}
    global_: Dict[str, Any] = Field(default_factory=dict, alias="global")
    #: event_id -> instance_name -> {...}
    events: Dict[Any, Any] = {}


class _RangeSpec(_WatchSpec):
    """One numeric field: where it lives (as a watched field) plus the
    range's parameters and learnt state."""

    __slots__ = ("slack", "alert_non_numeric", "lo", "hi", "n")

    def __init__(self, scope, event_id, kind, entry: Dict[str, Any]) -> None:
        super().__init__(scope, event_id, kind, entry.get("pos"), entry.get("name"))
        unknown = set(entry) - set(_FIELD_KEYS)
        if unknown:
            raise ValueError(
                f"{self.key}: unknown key(s) {sorted(unknown)}; valid keys: "
                f"{sorted(_FIELD_KEYS)}")
        if "pos" not in entry:
            raise ValueError(f"{scope}: a field entry has no 'pos': {dict(entry)!r}")
        # the numeric keys are validated by the same code as the pipeline's
        _, slack, lo, hi = ops.pack_ranges([{
            "pos": 0, **{k: entry[k] for k in ("slack", "non_numeric", "min", "max")
                         if k in entry}}])
        self.slack = float(slack[0])
        self.alert_non_numeric = entry.get("non_numeric", "ignore") == "alert"
        self.lo, self.hi, self.n = float(lo[0]), float(hi[0]), 0


def _parse_specs(config: ValueRangeDetectorConfig) -> List[_RangeSpec]:
    specs: List[_RangeSpec] = []

    def add_block(scope: str, event_id: Optional[int], block: Dict[str, Any]) -> None:
        for entry in block.get("variables") or []:
            specs.append(_RangeSpec(scope, event_id, "variable", entry))
        for entry in block.get("header_variables") or []:
            specs.append(_RangeSpec(scope, event_id, "header", entry))

    for _instance, block in (config.global_ or {}).items():
        if isinstance(block, dict):
            add_block("Global", None, block)
    for event_id, instances in (config.events or {}).items():
        try:
            eid = int(event_id)
        except (TypeError, ValueError):
            continue
        for _instance, block in (instances or {}).items():
            if isinstance(block, dict):
                add_block(f"Event {eid}", eid, block)
    return specs


class ValueRangeDetector(CoreDetector):
    CONFIG_CLASS = ValueRangeDetectorConfig

    def __init__(self, config=None) -> None:
        super().__init__(config)
        self.specs = _parse_specs(self.config)
        keys = [s.key for s in self.specs]
        if len(set(keys)) != len(keys):
            raise ValueError(f"ValueRangeDetector: duplicate field keys in {keys}")
        self.detector_id = f"value_range_detector-{id(self):x}"

    def _relevant_specs(self, parsed: ParserSchema) -> List[_RangeSpec]:
        return [s for s in self.specs
                if s.event_id is None or s.event_id == parsed.EventID]

    def train(self, parsed_batch: List[ParserSchema]) -> None:
        for parsed in parsed_batch:
            for spec in self._relevant_specs(parsed):
                text = spec.extract(parsed)
                if text is None:
                    continue
                v = ops.parse_number(text.encode("utf-8"))
                if v is not None:
                    spec.lo, spec.hi, spec.n = min(spec.lo, v), max(spec.hi, v), spec.n + 1

    @staticmethod
    def _judge(spec: _RangeSpec, text: str) -> Optional[str]:
        """The alert text of one present field, None when it has none."""
        v = ops.parse_number(text.encode("utf-8"))
        if v is None:
            return f"not a number: '{text}'" if spec.alert_non_numeric else None
        if not spec.lo <= spec.hi:  # nothing learnt, nothing configured
            return None
        m = spec.slack * (spec.hi - spec.lo)
        if v < spec.lo - m:
            side = "below"
        elif v > spec.hi + m:
            side = "above"
        else:
            return None
        return f"value out of range: {v:.15g} {side} [{spec.lo:.15g}, {spec.hi:.15g}]"

    def detect(self, parsed: ParserSchema, alert: DetectorSchema) -> bool:
        anomalies: Dict[str, str] = {}
        for spec in self._relevant_specs(parsed):
            text = spec.extract(parsed)
            if text is None:
                continue
            what = self._judge(spec, text)
            if what is not None:
                anomalies[spec.key] = what
        if not anomalies:
            return False
        alert.detectorID = self.detector_id
        alert.detectorType = "value_range_detector"
        alert.alertID = f"vr-{parsed.logID or parsed.parsedLogID}"
        alert.detectionTimestamp = int(time.time())
        alert.logIDs = [parsed.logID] if parsed.logID else []
        alert.score = 1.0
        alert.description = next(iter(anomalies.values()))
        alert.alertsObtain = dict(anomalies)
        return True

    # -- data-parallel state merge (dist_mode "dp") --------------------
    def dist_sync(self, group=None) -> None:
        """COLLECTIVE: every rank ends with the smallest lo, the largest hi
        and the summed n of all ranks."""
        import torch.distributed as tdist

        if not tdist.is_initialized() or tdist.get_world_size(group) <= 1:
            return
        gathered: list = [None] * tdist.get_world_size(group)
        tdist.all_gather_object(gathered, self._ranges(), group=group)
        for spec in self.specs:
            theirs = [g[spec.key] for g in gathered if g and spec.key in g]
            spec.lo = min(t["lo"] for t in theirs)
            spec.hi = max(t["hi"] for t in theirs)
            spec.n = sum(t["n"] for t in theirs)

    # -- checkpoint/resume ---------------------------------------------
    def _ranges(self) -> Dict[str, Dict[str, Any]]:
        return {s.key: {"lo": s.lo, "hi": s.hi, "n": s.n} for s in self.specs}

    def state_dict(self) -> Dict[str, Any]:
        return {"seen_lines": self._seen_lines, "ranges": self._ranges()}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        ranges = state.get("ranges") or {}
        mine = {s.key for s in self.specs}
        if set(ranges) != mine:
            raise ValueError(
                f"value-range checkpoint holds the fields {sorted(ranges)} but "
                f"this instance is configured for {sorted(mine)}")
        self._seen_lines = int(state.get("seen_lines", 0))
        for s in self.specs:
            r = ranges[s.key]
            s.lo, s.hi, s.n = float(r["lo"]), float(r["hi"]), int(r["n"])
