"""The detector stages of GpuPipeline, one object each: its launch, result
keys, flag, alert wording and state. GpuPipeline and FusedPipelineDetector
loop over ``pipe.stages``. No stage reads another's output or state, only
``lines`` and the parse result ``match`` (docs/architecture.md, "Adding a
stage")."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import torch

from . import ops
from .models.bert_tiny import BertTinyDetectorModel, EmbeddingStats


def marked(name: str, device: torch.device, fn: Callable, *args):
    """fn(*args) inside a roctx-visible range (torch.cuda.nvtx maps to
    rocTracer markers on ROCm — SURVEY.md §5.1 tracing requirement)."""
    if device.type != "cuda":
        return fn(*args)
    torch.cuda.nvtx.range_push(name)
    out = fn(*args)
    torch.cuda.nvtx.range_pop()
    return out


def straddle(B: int, train_upto: int, judge: Callable, zeros: Callable, *per_row):
    """The verdict on B rows, given as per-row tensors, of which the first
    train_upto are training rows: those score nothing, the tail is
    ``judge(*tail rows)``. In the steady state the kernel's output IS the
    result (a zeros + full copy here cost 2 kernel launches per batch);
    ``zeros()``, B rows of nothing, is built only while training."""
    if train_upto == 0:
        return judge(*per_row)
    out = zeros()
    if train_upto < B:
        out[train_upto:] = judge(*(t[train_upto:] for t in per_row))
    return out


def union_hashsets(hs: "ops.GpuHashSets", group) -> None:
    """COLLECTIVE union of the data-parallel hash sets ``hs`` of every rank."""
    import torch.distributed as tdist
    if hasattr(hs, "tables"):  # GPU open-addressing tables
        from .parallel.dist import all_reduce_hashsets
        all_reduce_hashsets(hs.tables, group=group)
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


class Stage:
    """What the pipeline and the detector ask of a stage, next to
    ``run(lines, match, train_upto, n_valid) -> dict`` of its keys; the
    defaults are a stage with nothing to do."""
    name = ""                  # also the stage's marker, "dmx::" + name
    keys: tuple = ()           # result keys the stage owns
    per_slot_keys: tuple = ()  # of those, the ones not indexed by line
    windowed = False           # verdict about the stream: a re-score skips it
    parts: Dict[str, object] = {}  # checkpoint key -> state object, or None

    def empty(self, device) -> dict:
        """The stage's keys for a batch of no rows, or when it is skipped."""
        return dict.fromkeys(self.keys)

    def flags(self, out: dict) -> Optional[torch.Tensor]:
        return None

    def reasons(self, host_out: dict, i: int) -> List[str]:
        return []

    def before_replay(self, n_rows: int) -> None:
        pass

    def dist_sync(self, group) -> None:
        pass

    def state_dict(self) -> dict:
        return {k: part.state_dict() for k, part in self.parts.items()
                if part is not None}

    def load_state_dict(self, state: dict) -> None:
        for k, part in self.parts.items():
            if k in state and part is not None:
                part.load_state_dict(state[k])


class NewValueStage(Stage):
    """Watched fields and combinations of fields (docs/kernels.md,
    "Combination hash"): one launch hashes both, one probe covers one table
    per watch, then one per combination; training rows insert instead."""
    name = "new_value"
    keys = ("nv_unseen", "combo_unseen")

    def __init__(self, config, device) -> None:
        specs = [ops.watch_spec_row(w) for w in config.watches]
        self.specs = torch.tensor(specs, dtype=torch.int32).reshape(-1, 4).to(device)
        # combinations: CSR member table, validated on the host before upload
        self.n_combos = len(config.combos)
        self.members = self.combo_off = None
        if self.n_combos:
            members, combo_off = ops.pack_combos(config.combos)
            self.members, self.combo_off = members.to(device), combo_off.to(device)
        self.lowercase = config.lowercase
        n_tables = len(specs) + self.n_combos
        self.state = (ops.GpuHashSets(n_tables, config.hashset_capacity, device=device)
                      if n_tables else None)
        self.parts = {"hashsets": self.state}
        self._unseen = None  # [B, W + C] of the last run; the two keys view it

    def run(self, lines, match, train_upto, n_valid):
        if self.n_combos:
            hashes = ops.watch_combo_hashes(
                lines, match, self.specs, self.members, self.combo_off, self.lowercase)
        else:
            hashes = ops.watch_hashes(lines, match, self.specs, self.lowercase)
        if train_upto > 0:
            self.state.insert(hashes[:train_upto])
        B, W = lines.shape[0], self.specs.shape[0]
        unseen = self._unseen = straddle(
            B, train_upto, self.state.probe,
            lambda: torch.zeros((B, W + self.n_combos), dtype=torch.int32,
                                device=lines.device), hashes)
        if not self.n_combos:
            return {"nv_unseen": unseen, "combo_unseen": None}
        return {"nv_unseen": unseen[:, :W] if W else None, "combo_unseen": unseen[:, W:]}

    def flags(self, out):
        # one reduction over watch and combination columns alike
        return self._unseen.sum(dim=1) > 0

    def reasons(self, host_out, i):
        return [text for k, text in (("nv_unseen", "unknown watched value"),
                                     ("combo_unseen", "unknown combination"))
                if host_out.get(k) is not None and int(host_out[k][i].sum()) > 0]

    def dist_sync(self, group):
        union_hashsets(self.state, group)


class EventRateStage(Stage):
    """Per-event line counts in windows of ``window_lines`` lines against an
    EWMA baseline (docs/kernels.md, "Event-rate windows"). The only stage
    whose verdict is about the stream and not about one line: its state lives
    on the device, the line that completes a window carries the alert, and
    each rank judges its own shard (no dist_sync)."""
    name = "event_rate"
    keys = ("rate_hits", "rate_slot", "rate_counts", "rate_z")
    per_slot_keys = ("rate_counts", "rate_z")  # [NW, E]
    windowed = True

    def __init__(self, config, device, n_templates: int) -> None:
        unknown = set(config.event_rate) - set(ops.EVENT_RATE_DEFAULTS)
        if unknown:
            raise ValueError(
                f"unknown event_rate key(s) {sorted(unknown)}; valid keys: "
                f"{sorted(ops.EVENT_RATE_DEFAULTS)}")
        self.state = ops.EventRateState(
            n_templates, device=device, **{**ops.EVENT_RATE_DEFAULTS, **config.event_rate})
        self.parts = {"event_rate": self.state}

    def run(self, lines, match, train_upto, n_valid):
        return self.state.step(match["event_id"], n_valid, train_upto)

    def flags(self, out):
        # non-zero only on a boundary line outside the training phase
        hits = out["rate_hits"]
        return None if hits is None else hits > 0

    def before_replay(self, n_rows):
        # pad rows parse as unparsed lines; they must not be counted
        self.state.set_n_valid(n_rows)

    def reasons(self, host_out, i):
        """"event rate: event 3: 950/window (z=+12.3); ..." for boundary row
        i: the flagged bins of the window that row completed."""
        hits = host_out.get("rate_hits")
        if hits is None or int(hits[i]) <= 0:
            return []
        slot = int(host_out["rate_slot"][i])
        counts, z = host_out["rate_counts"][slot], host_out["rate_z"][slot]
        parts = []
        for e in torch.nonzero(z, as_tuple=False).flatten().tolist():
            who = "unparsed" if e == 0 else f"event {e}"
            parts.append(f"{who}: {int(counts[e])}/window (z={float(z[e]):+.1f})")
        return ["event rate: " + "; ".join(parts)]


class EventSequenceStage(Stage):
    """The n-gram of event ids that each line completes within its key's
    history (docs/kernels.md, "Event sequences") against the set of grams
    seen in training. The per-key histories are stream state on the device
    and move on every member row, training or not; the verdict is a probe of
    the gram's hash, as NewValueStage probes a value's. Under data-parallel
    ranks the gram set is united, the histories stay per rank."""
    name = "event_sequence"
    keys = ("seq_unseen", "seq_gram")
    windowed = True  # a re-score of old lines must not move live histories

    def __init__(self, config, device, n_templates: int) -> None:
        unknown = set(config.event_sequence) - set(ops.EVENT_SEQUENCE_DEFAULTS)
        if unknown:
            raise ValueError(
                f"unknown event_sequence key(s) {sorted(unknown)}; valid keys: "
                f"{sorted(ops.EVENT_SEQUENCE_DEFAULTS)}")
        p = {**ops.EVENT_SEQUENCE_DEFAULTS, **config.event_sequence}
        self.state = ops.EventSequenceState(
            n_templates, length=p["length"], max_keys=p["max_keys"], key=p["key"],
            lowercase=config.lowercase, device=device)
        capacity = int(config.hashset_capacity if p["capacity"] is None
                       else p["capacity"])
        if capacity < 1 or capacity & (capacity - 1):
            raise ValueError(
                f"event_sequence capacity must be a power of two, got {capacity}")
        self.grams = ops.GpuHashSets(1, capacity, device=device)
        self.parts = {"event_sequence": self.state, "sequence_grams": self.grams}

    def run(self, lines, match, train_upto, n_valid):
        gram, hashes = self.state.step(lines, match, n_valid)
        if train_upto > 0:
            self.grams.insert(hashes[:train_upto])
        B = lines.shape[0]
        unseen = straddle(
            B, train_upto, self.grams.probe,
            lambda: torch.zeros((B, 1), dtype=torch.int32, device=lines.device),
            hashes)
        return {"seq_unseen": unseen.view(B), "seq_gram": gram}

    def flags(self, out):
        unseen = out.get("seq_unseen")
        return None if unseen is None else unseen > 0

    def before_replay(self, n_rows):
        # pad rows parse as lines of length 0; they must not enter a history
        self.state.set_n_valid(n_rows)

    def reasons(self, host_out, i):
        """"unknown event sequence: ^ > 3 > 7 (per ses)": the gram of row i,
        oldest event first, ^ where the key's history was still empty."""
        unseen = host_out.get("seq_unseen")
        if unseen is None or int(unseen[i]) <= 0:
            return []
        symbols = ops.decode_gram(int(host_out["seq_gram"][i]), self.state.length)
        return [ops.sequence_text(symbols, self.state.key_name)]

    def dist_sync(self, group):
        union_hashsets(self.grams, group)


class ValueRangeStage(Stage):
    """Each range's field is parsed as a decimal number from the line bytes
    and judged against the smallest and largest value seen in training
    (docs/kernels.md, "Value ranges"): rows below train_upto move lo / hi /
    n, every row is judged against the state after them, one launch."""
    name = "value_range"
    keys = ("range_code", "range_value")

    def __init__(self, config, device) -> None:
        self.state = ops.ValueRangeState(list(config.ranges), device=device)
        self.parts = {"value_ranges": self.state}

    def run(self, lines, match, train_upto, n_valid):
        code, value = self.state.step(lines, match, train_upto)
        return {"range_code": code, "range_value": value}

    def empty(self, device):
        R = self.state.R
        return {"range_code": torch.zeros((0, R), dtype=torch.int32, device=device),
                "range_value": torch.zeros((0, R), dtype=torch.float64, device=device)}

    def flags(self, out):
        return (out["range_code"] != 0).any(dim=1)

    def reasons(self, host_out, i):
        """"value out of range: bytes = 18234511 above [0, 1048576]" or "not
        a number: bytes" for every flagged range of row i. The bounds are
        read from the device state here, when an alert is worded, and
        nowhere on the hot path."""
        codes = host_out["range_code"][i]
        if not bool(codes.any()):
            return []
        lo, hi = self.state.lo.cpu(), self.state.hi.cpu()
        reasons = []
        for r in torch.nonzero(codes, as_tuple=False).flatten().tolist():
            code, name = int(codes[r]), self.state.names[r]
            if code == 3:
                reasons.append(f"not a number: {name}")
                continue
            side = "below" if code == 1 else "above"
            reasons.append(
                f"value out of range: {name} = {float(host_out['range_value'][i, r]):.15g} "
                f"{side} [{float(lo[r]):.15g}, {float(hi[r]):.15g}]")
        return reasons

    def dist_sync(self, group):
        """COLLECTIVE: every rank ends with the smallest lo, the largest hi
        and the summed n of all ranks, written into the tensors the kernels
        (and a captured graph) read."""
        import torch.distributed as tdist
        state = self.state
        lo, hi, n = state.lo.clone(), state.hi.clone(), state.n.clone()
        tdist.all_reduce(lo, op=tdist.ReduceOp.MIN, group=group)
        tdist.all_reduce(hi, op=tdist.ReduceOp.MAX, group=group)
        tdist.all_reduce(n, op=tdist.ReduceOp.SUM, group=group)
        state.merge_(lo, hi, n - state.n)  # n: the other ranks' share


class TransformerStage(Stage):
    """BERT-tiny (bf16 MFMA) over the byte tokens of the content span, which
    comes straight from the match kernel. ``score_mode`` "head" (default) is
    the model's linear score head. "embedding" is the distance of the line's
    mean-pooled embedding from a diagonal Gaussian fitted to the training rows
    (``stats``, None in "head"): those rows update the moments and score 0,
    later rows score ``sqrt(mean_i((x_i - mu_i)^2 / var_i))``: one launch of
    the fused kernel's distance head in the steady state, no [B, hidden]
    write, a second launch on the tail of a batch that straddles the
    boundary. An empty content span is far from any trained distribution, so
    it alerts (about 11.5 on the audit-log generator against a normal maximum
    of about 1.3)."""
    name = "transformer"  # its one key, "scores", is a base key of the result

    def __init__(self, config, device) -> None:
        self.config = config  # reasons() reads the live score_threshold
        self.state = BertTinyDetectorModel(config.bert, device=device, seed=config.seed)
        self.stats = (EmbeddingStats(config.bert.hidden, device=device)
                      if config.score_mode == "embedding" else None)
        self.parts = {"model": self.state, "embedding_stats": self.stats}

    def run(self, lines, match, train_upto, n_valid):
        model, stats = self.state, self.stats
        start, end = match["span_start"], match["span_end"]
        if stats is None:
            return {"scores": model.score_spans(lines, start, end)}
        B = lines.shape[0]
        if train_upto > 0:
            stats.update(model.embed_spans(
                lines[:train_upto], start[:train_upto], end[:train_upto]))
        return {"scores": straddle(
            B, B if stats.n == 0 else train_upto,  # nothing fitted: no distance
            lambda l, s, e: model.embed_distance_spans(l, s, e, stats.mu, stats.inv_var),
            lambda: torch.zeros(B, dtype=torch.float32, device=lines.device),
            lines, start, end)}

    def reasons(self, host_out, i):
        score = float(host_out["scores"][i])
        if score <= self.config.score_threshold:
            return []
        what = "embedding distance" if self.stats is not None else "score"
        return [f"{what} {score:.3f}"]
