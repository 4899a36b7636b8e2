"""GPU ops layer: HIP kernels with CPU reference fallbacks.

Policy (build mandate): on a GPU box the HIP extension MUST load — any op
asked to run on a CUDA/HIP tensor raises if ``_dmx_C`` is missing (no
silent eager fallback). On CPU (CI container has no GPU) the pure-torch
reference paths run; they define the semantics the kernels are tested
against (tests/test_gpu_ops.py compares kernel output to these fp32
references).
"""
from __future__ import annotations

import math
import re
from typing import List, Optional, Sequence, Tuple

import torch

_C = None
_C_ERR: Optional[str] = None
try:
    from . import _dmx_C as _C  # type: ignore[no-redef]
except ImportError as exc:  # pragma: no cover - exercised on GPU boxes
    _C_ERR = str(exc)


def have_extension() -> bool:
    return _C is not None


def _require_ext():
    if _C is None:
        raise RuntimeError(
            "detectmateservice_amd HIP extension (_dmx_C) is not built but a "
            "GPU tensor was passed. Build it in-tree with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Import error: {_C_ERR}"
        )
    return _C


# ---------------------------------------------------------------------------
# dense ops
# ---------------------------------------------------------------------------

EPILOGUE = {"none": 0, "gelu": 1, "relu": 2}


def fused_linear(
    x: torch.Tensor,
    wt: torch.Tensor,
    bias: Optional[torch.Tensor] = None,
    activation: str = "none",
) -> torch.Tensor:
    """C = act(x @ wt.T + bias).  x [M,K] bf16; wt [N,K] bf16 (pre-transposed).

    GPU: hand-written MFMA kernel (ops/csrc/gemm_bf16.hip).
    CPU: torch reference in fp32 then cast back.
    """
    if x.is_cuda:
        return _require_ext().fused_linear_bf16(x, wt, bias, EPILOGUE[activation])
    y = torch.nn.functional.linear(x.float(), wt.float(), bias)
    if activation == "gelu":
        y = torch.nn.functional.gelu(y, approximate="tanh")
    elif activation == "relu":
        y = torch.relu(y)
    return y.to(x.dtype)


def layernorm(
    x: torch.Tensor,
    gamma: torch.Tensor,
    beta: torch.Tensor,
    residual: Optional[torch.Tensor] = None,
    eps: float = 1e-5,
    return_xres: bool = False,
):
    """y = LN(x [+ residual]) * gamma + beta (fused residual add).

    Optionally also returns x+residual (the next block's residual input).
    """
    if x.is_cuda:
        out = _require_ext().layernorm_bf16(x, residual, gamma, beta, eps, return_xres)
        return (out[0], out[1]) if return_xres else out[0]
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
    y = torch.nn.functional.layer_norm(xf, (x.shape[-1],), gamma.float(), beta.float(), eps)
    y = y.to(x.dtype)
    if return_xres:
        return y, xf.to(x.dtype)
    return y


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """Fused MHA for [BH, S, Dh] with S<=128, Dh<=64 (bf16)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if q.is_cuda:
        return _require_ext().attention_bf16(q, k, v, scale)
    s = torch.softmax(q.float() @ k.float().transpose(-1, -2) * scale, dim=-1)
    return (s @ v.float()).to(q.dtype)


def attention_qkv(qkv: torch.Tensor, S: int, H: int, Dh: int, scale: Optional[float] = None) -> torch.Tensor:
    """MHA over the fused QKV projection output.

    qkv [B, S, 3*H*Dh] (q|k|v interleaved per row as the qkv linear emits
    them) -> O [B, S, H*Dh]. GPU: single MFMA kernel with no permutes
    (ops/csrc/attention_mfma.hip) when S%32==0, S<=128, Dh in {32,64};
    otherwise splits + falls back to :func:`attention`.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(Dh)
    B = qkv.shape[0]
    if qkv.is_cuda and S % 32 == 0 and S <= 128 and Dh in (32, 64):
        return _require_ext().attention_qkv_bf16(qkv, S, H, Dh, scale)
    # reference path: split + permute
    q, k, v = qkv.view(B, S, 3, H, Dh).unbind(dim=2)
    q = q.permute(0, 2, 1, 3).reshape(B * H, S, Dh).contiguous()
    k = k.permute(0, 2, 1, 3).reshape(B * H, S, Dh).contiguous()
    v = v.permute(0, 2, 1, 3).reshape(B * H, S, Dh).contiguous()
    o = attention(q, k, v, scale)
    return (
        o.view(B, H, S, Dh).permute(0, 2, 1, 3).reshape(B, S, H * Dh).contiguous()
    )


# ---------------------------------------------------------------------------
# parser: batched template matching
# ---------------------------------------------------------------------------


def pack_lines(lines: Sequence[bytes], max_len: int = 512, device="cpu") -> Tuple[torch.Tensor, torch.Tensor]:
    """Pad raw line bytes into a [B, max_len] u8 SoA tensor + lengths."""
    B = len(lines)
    buf = torch.zeros((B, max_len), dtype=torch.uint8)
    lens = torch.zeros((B,), dtype=torch.int32)
    for i, ln in enumerate(lines):
        b = ln[:max_len]
        if b:
            buf[i, : len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        lens[i] = len(b)
    return buf.to(device), lens.to(device)


def pack_templates(templates: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    """Template strings -> (seg_bytes u8, seg_off i32, tpl_seg_start i32,
    max_caps). Segments are ``template.split('<*>')`` — identical to the
    Python matcher."""
    seg_bytes = bytearray()
    seg_off = [0]
    tpl_seg_start = [0]
    max_caps = 0
    for t in templates:
        segs = t.split("<*>")
        max_caps = max(max_caps, len(segs) - 1 + (1 if segs and segs[-1] == "" else 0))
        for s in segs:
            seg_bytes.extend(s.encode("utf-8"))
            seg_off.append(len(seg_bytes))
        tpl_seg_start.append(tpl_seg_start[-1] + len(segs))
    return (
        torch.frombuffer(bytearray(seg_bytes) or bytearray(b"\0"), dtype=torch.uint8).clone(),
        torch.tensor(seg_off, dtype=torch.int32),
        torch.tensor(tpl_seg_start, dtype=torch.int32),
        max(max_caps, 1),
    )


class TemplateMatcher:
    """Batched GPU/CPU template matcher sharing semantics with
    library/parsers/template_matcher.py (format split + content templates)."""

    def __init__(
        self,
        templates: Sequence[str],
        log_format: Optional[str] = None,
        lowercase: bool = False,
        device: str | torch.device = "cpu",
        max_len: int = 512,
    ) -> None:
        self.templates = list(templates)
        self.log_format = log_format
        self.lowercase = lowercase
        self.device = torch.device(device)
        self.max_len = max_len

        sb, so, ts, self.max_caps = pack_templates(self.templates)
        self.seg_bytes = sb.to(self.device)
        self.seg_off = so.to(self.device)
        self.tpl_seg_start = ts.to(self.device)

        if log_format:
            import re

            fmt_tpl = re.sub(r"<[A-Za-z_][A-Za-z0-9_]*>", "<*>", log_format)
            self.fmt_field_names = re.findall(r"<([A-Za-z_][A-Za-z0-9_]*)>", log_format)
            fb, fo, _fts, self.max_fmt_caps = pack_templates([fmt_tpl])
            self.fmt_bytes = fb.to(self.device)
            self.fmt_seg_off = fo.to(self.device)
        else:
            self.fmt_field_names = []
            self.fmt_bytes = torch.zeros(0, dtype=torch.uint8, device=self.device)
            self.fmt_seg_off = torch.zeros(0, dtype=torch.int32, device=self.device)
            self.max_fmt_caps = 1

    def match_packed(self, lines: torch.Tensor, line_len: torch.Tensor):
        """lines [B, max_len] u8 on self.device. Returns dict of tensors:
        event_id [B], fmt_caps [B,Fc,2], n_fmt_caps [B], caps [B,C,2], n_caps [B]."""
        if lines.shape[0] == 0:  # zero-grid kernel launches are invalid
            z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=lines.device)  # noqa: E731
            return {"event_id": z(0), "fmt_caps": z(0, self.max_fmt_caps, 2),
                    "n_fmt_caps": z(0), "caps": z(0, self.max_caps, 2),
                    "n_caps": z(0), "span_start": z(0), "span_end": z(0)}
        if lines.is_cuda:
            (ev, fc, nfc, caps, ncaps, sps, spe) = _require_ext().template_match(
                lines, line_len, self.fmt_bytes, self.fmt_seg_off,
                self.seg_bytes, self.seg_off, self.tpl_seg_start,
                self.lowercase, self.max_fmt_caps, self.max_caps,
            )
            return {"event_id": ev, "fmt_caps": fc, "n_fmt_caps": nfc,
                    "caps": caps, "n_caps": ncaps, "span_start": sps,
                    "span_end": spe}
        if _C is not None:
            # C++ twin of the kernel (the pure-Python matcher measured
            # ~9.5k lines/s and bottlenecked CPU service mode)
            ev, fc, nfc, caps, ncaps = _C.template_match_cpu(
                lines, line_len, self.fmt_bytes, self.fmt_seg_off,
                self.seg_bytes, self.seg_off, self.tpl_seg_start,
                self.lowercase, self.max_fmt_caps, self.max_caps,
            )
            out = {"event_id": ev, "fmt_caps": fc, "n_fmt_caps": nfc,
                   "caps": caps, "n_caps": ncaps}
            self._add_spans(out, line_len, lines.shape[1])
            return out
        out = self._match_cpu(lines, line_len)
        self._add_spans(out, line_len, lines.shape[1])
        return out

    @staticmethod
    def _add_spans(match: dict, line_len: torch.Tensor, max_len: int) -> None:
        """CPU-path twin of the kernel's span outputs: content span = last
        written header capture when the format matched, else [0, len) with
        len = min(line_len, max_len) as the kernel cuts it."""
        nfc = match["n_fmt_caps"].long()
        has_hdr = nfc > 0
        fc = match["fmt_caps"]
        last = (nfc.clamp(max=fc.shape[1]) - 1).clamp(min=0)
        start = torch.where(
            has_hdr,
            fc.gather(1, last.view(-1, 1, 1).expand(-1, 1, 2))[:, 0, 0].long(),
            torch.zeros_like(nfc),
        )
        end = torch.where(
            has_hdr,
            fc.gather(1, last.view(-1, 1, 1).expand(-1, 1, 2))[:, 0, 1].long(),
            line_len.long().clamp(max=int(max_len)),
        )
        match["span_start"] = start.int()
        match["span_end"] = end.int()

    # -- pure-Python mirror of the kernel (runs when the extension is absent) --
    def _match_cpu(self, lines: torch.Tensor, line_len: torch.Tensor):
        """The kernel's match on the CPU, in bytes like the kernel and the
        C++ twin: a line is its first min(line_len, max_len) bytes, every
        offset is a byte offset, and ``lowercase`` folds A-Z only, and only
        for the content match (the format match never folds). No byte of the
        line is decoded, so lines that are not UTF-8 match the same way."""
        B, max_len = lines.shape[0], lines.shape[1]
        ev = torch.full((B,), -1, dtype=torch.int32)
        fc = torch.zeros((B, self.max_fmt_caps, 2), dtype=torch.int32)
        nfc = torch.zeros((B,), dtype=torch.int32)
        caps = torch.zeros((B, self.max_caps, 2), dtype=torch.int32)
        ncaps = torch.zeros((B,), dtype=torch.int32)

        fmt_segs = None
        if self.log_format:
            fmt_segs = [s.encode("utf-8") for s in re.sub(
                r"<[A-Za-z_][A-Za-z0-9_]*>", "<*>", self.log_format
            ).split("<*>")]
        tpl_segs = [[s.encode("utf-8") for s in t.split("<*>")]
                    for t in self.templates]

        rows = lines.numpy()
        lens = line_len.tolist()
        for i in range(B):
            raw = rows[i, : min(max(int(lens[i]), 0), max_len)].tobytes()
            start, end = 0, len(raw)
            if fmt_segs:
                spans = _span_match(raw, 0, len(raw), fmt_segs)
                if spans is not None:
                    nfc[i] = len(spans)
                    for j, (a, b) in enumerate(spans[: self.max_fmt_caps]):
                        fc[i, j, 0], fc[i, j, 1] = a, b
                    if spans:
                        start, end = spans[: self.max_fmt_caps][-1]
            cmp_raw = raw.translate(_ASCII_FOLD) if self.lowercase else raw
            for t, segs in enumerate(tpl_segs):
                spans = _span_match(cmp_raw, start, end, segs)
                if spans is not None:
                    ev[i] = t + 1
                    ncaps[i] = len(spans)
                    for j, (a, b) in enumerate(spans[: self.max_caps]):
                        caps[i, j, 0], caps[i, j, 1] = a, b
                    break
        return {"event_id": ev, "fmt_caps": fc, "n_fmt_caps": nfc,
                "caps": caps, "n_caps": ncaps}


#: bytes.translate table of the kernel's fold: A-Z -> a-z, every other byte
#: (0x80 - 0xff included) unchanged
_ASCII_FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def _span_match(text: bytes, start: int, end: int, segments: List[bytes]):
    """The algorithm of template_match.hip::match_segments on ``bytes``:
    greedy-anchored, byte offsets, (start, end) spans or None. The caller
    folds ``text``; the segments are compared as they are."""
    pos = start
    spans: List[Tuple[int, int]] = []
    n = len(segments)
    for i, seg in enumerate(segments):
        if len(seg) == 0:
            if i == n - 1:
                spans.append((pos, end))
                return spans
            continue
        idx = text.find(seg, pos, end)
        if idx < 0:
            return None
        if i == 0 and idx != start:
            return None
        if i > 0:
            spans.append((pos, idx))
        pos = idx + len(seg)
    if pos != end:
        return None
    return spans


# ---------------------------------------------------------------------------
# detector: GPU hash sets
# ---------------------------------------------------------------------------


class GpuHashSets:
    """W open-addressing u64 hash sets (one per watched field) resident on
    device; CPU fallback keeps Python sets with the same FNV-1a hashing."""

    def __init__(self, n_watch: int, capacity: int = 1 << 16, device="cpu") -> None:
        assert capacity & (capacity - 1) == 0
        self.W = n_watch
        self.capacity = capacity
        self.device = torch.device(device)
        if self.device.type == "cuda":
            self.tables = torch.zeros((n_watch, capacity), dtype=torch.int64, device=self.device)
        else:
            self.sets: List[set] = [set() for _ in range(n_watch)]

    def insert(self, hashes: torch.Tensor) -> None:
        if hashes.shape[0] == 0:
            return
        if self.device.type == "cuda":
            _require_ext().hashset_insert(hashes, self.tables)
        else:
            h = hashes.cpu().numpy()
            for w in range(self.W):
                self.sets[w].update(int(x) for x in h[:, w] if x != 0)

    def probe(self, hashes: torch.Tensor) -> torch.Tensor:
        if hashes.shape[0] == 0:
            return torch.zeros((0, self.W), dtype=torch.int32, device=hashes.device)
        if self.device.type == "cuda":
            return _require_ext().hashset_probe(hashes, self.tables)
        h = hashes.cpu().numpy()
        out = torch.zeros(hashes.shape, dtype=torch.int32)
        for w in range(self.W):
            s = self.sets[w]
            for i in range(h.shape[0]):
                v = int(h[i, w])
                out[i, w] = 1 if (v != 0 and v not in s) else 0
        return out

    def state_dict(self):
        if self.device.type == "cuda":
            return {"type": "gpu", "tables": self.tables.cpu()}
        return {"type": "cpu", "sets": [sorted(s) for s in self.sets]}

    def _check_state_shape(self, state) -> None:
        """A checkpoint holds one table per watch and per combination; one
        taken under another configuration must not load (its columns would
        mean other fields)."""
        if state["type"] == "gpu":
            theirs = tuple(state["tables"].shape)
        else:  # CPU sets carry no capacity
            theirs = (len(state["sets"]), self.capacity)
        mine = (self.W, self.capacity)
        if theirs != mine:
            raise ValueError(
                f"hash-set checkpoint holds [tables, capacity] = {list(theirs)} "
                f"but this instance is configured for {list(mine)} "
                "(watches + combos, hashset_capacity)")

    def load_state_dict(self, state):
        self._check_state_shape(state)
        if self.device.type == "cuda":
            if state["type"] == "gpu":
                self.tables.copy_(state["tables"].to(self.device))
            else:
                for w, vals in enumerate(state["sets"]):
                    if vals:
                        h = torch.zeros((len(vals), self.W), dtype=torch.int64)
                        h[:, w] = torch.tensor(vals, dtype=torch.int64)
                        self.insert(h.to(self.device))
        else:
            if state["type"] == "cpu":
                self.sets = [set(v) for v in state["sets"]]
            else:
                t = state["tables"]
                for w in range(self.W):
                    self.sets[w] = set(int(x) for x in t[w][t[w] != 0].tolist())


def fnv1a64(data: bytes, lower: bool = False) -> int:
    """CPU mirror of the kernel's hash (for parity tests + CPU fallback)."""
    h = 1469598103934665603
    for c in data:
        if lower and 65 <= c <= 90:
            c += 32
        h ^= c
        h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h | 1


def _parsed_args(lines, match: dict):
    """The parsed batch as the extension's field entry points take it: six
    positional tensors (docs/kernels.md, "Parsed batch and field span")."""
    return (lines, match["event_id"], match["caps"], match["n_caps"],
            match["fmt_caps"], match["n_fmt_caps"])


def _field_span(parsed, max_len: int, spec, i: int) -> Optional[Tuple[int, int]]:
    """CPU mirror of field_span (field_span.h): (start, end) of the field
    that the spec row (kind, event, pos, _) names on line i, or None when the
    spec is not relevant for the line or the field is absent. ``parsed`` is
    _parsed_args without the lines, each tensor as nested lists."""
    event_id, caps, n_caps, fmt_caps, n_fmt_caps = parsed
    kind, event, pos = spec[0], spec[1], spec[2]
    if not (kind != 0 or event < 0 or event_id[i] == event) or pos < 0:
        return None
    if kind != 0:
        table, there = fmt_caps[i], pos < min(n_fmt_caps[i], len(fmt_caps[i]))
    else:
        table, there = caps[i], pos < min(n_caps[i], len(caps[i]))
    if not there:
        return None
    start, end = table[pos]
    if start < 0 or end < start or end > max_len:
        return None
    return start, end


def watch_hashes_cpu(
    lines: torch.Tensor,
    match: dict,
    specs: torch.Tensor,
    lower: bool = False,
) -> torch.Tensor:
    """CPU mirror of dmx_watch_hashes."""
    B, max_len = int(lines.shape[0]), int(lines.shape[1])
    W = specs.shape[0]
    out = torch.zeros((B, W), dtype=torch.int64)
    parsed = [t.tolist() for t in _parsed_args(lines, match)[1:]]
    spec = specs.tolist()
    for i in range(B):
        row = bytes(lines[i].numpy().tobytes())
        for w in range(W):
            span = _field_span(parsed, max_len, spec[w], i)
            if span is not None:
                out[i, w] = _as_i64(fnv1a64(row[span[0]:span[1]], lower))
    return out


def watch_hashes(lines, match: dict, specs: torch.Tensor, lower: bool = False) -> torch.Tensor:
    if lines.is_cuda:
        return _require_ext().watch_hashes(*_parsed_args(lines, match), specs, lower)
    return watch_hashes_cpu(lines, match, specs, lower)


# ---------------------------------------------------------------------------
# detector: combinations of watched fields (docs/kernels.md, "Combination
# hash" is the definition; the kernel, the CPU mirror and combo_fold below
# are its three implementations)
# ---------------------------------------------------------------------------

FNV_OFFSET = 1469598103934665603
FNV_PRIME = 1099511628211
_U64 = 0xFFFFFFFFFFFFFFFF


def _as_i64(h: int) -> int:
    """Two's-complement view of an unsigned 64-bit hash (tensors are int64)."""
    return h - (1 << 64) if h >= (1 << 63) else h


def watch_spec_row(w: dict) -> List[int]:
    """One watch dict -> the kernel's FieldSpec row (kind, event, pos, pad)."""
    kind = 0 if w.get("kind", "variable") == "variable" else 1
    return [kind, int(w.get("event", -1)), int(w["pos"]), 0]


def pack_combos(combos: Sequence[Sequence[dict]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """List of combinations, each a list of watch dicts -> (members int32
    [M, 4], combo_off int32 [C + 1]), CSR style. This is the host-side
    validation of the offsets the kernel trusts: they start at 0, strictly
    increase (no empty combination) and end at M."""
    rows: List[List[int]] = []
    off = [0]
    for c, combo in enumerate(combos):
        if len(combo) == 0:
            raise ValueError(f"combo {c} is empty: a combination needs at least one member")
        for j, w in enumerate(combo):
            if "pos" not in w:
                raise ValueError(f"combo {c}, member {j} has no 'pos': {dict(w)!r}")
            row = watch_spec_row(w)
            if row[2] < 0:
                raise ValueError(f"combo {c}, member {j}: 'pos' must be >= 0, got {row[2]}")
            rows.append(row)
        off.append(len(rows))
    members = (torch.tensor(rows, dtype=torch.int32) if rows
               else torch.zeros((0, 4), dtype=torch.int32))
    return members, torch.tensor(off, dtype=torch.int32)


def combo_fold(relevant, member_hashes):
    """Host fold of the combination hash, vectorised over a batch.

    relevant [B, n] (0/1) and member_hashes [B, n] (int64 or uint64, 0 where
    the member is absent or not relevant) -> int64 numpy array [B]: 0 where
    no member is relevant, odd otherwise."""
    import numpy as np

    r = np.asarray(relevant)
    m = np.asarray(member_hashes)
    if r.ndim != 2 or r.shape != m.shape:
        raise ValueError(
            f"relevant {r.shape} and member_hashes {m.shape} must be the same [B, n]")
    r = (r != 0).astype(np.uint64)
    m = m.astype(np.int64, copy=False).view(np.uint64) if m.dtype != np.uint64 else m
    m = np.where(r != 0, m, np.uint64(0))
    prime = np.uint64(FNV_PRIME)
    h = np.full(r.shape[0], FNV_OFFSET, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(r.shape[1]):
            h = (h ^ r[:, j]) * prime
            for b in range(8):
                h = (h ^ ((m[:, j] >> np.uint64(8 * b)) & np.uint64(0xFF))) * prime
    h = np.where(r.any(axis=1), h | np.uint64(1), np.uint64(0))
    return h.view(np.int64)


def watch_combo_hashes_cpu(
    lines: torch.Tensor,
    match: dict,
    specs: torch.Tensor,
    members: torch.Tensor,
    combo_off: torch.Tensor,
    lower: bool = False,
) -> torch.Tensor:
    """CPU mirror of dmx_watch_combo_hashes: int64 [B, W + C], plain Python
    integers throughout."""
    B = lines.shape[0]
    W = specs.shape[0]
    off = [int(x) for x in combo_off.tolist()]
    C = len(off) - 1
    out = torch.zeros((B, W + C), dtype=torch.int64)
    out[:, :W] = watch_hashes_cpu(lines, match, specs, lower)
    if C == 0 or B == 0:
        return out
    # each member's span hash as an unsigned value (0 = absent / not relevant)
    mh = watch_hashes_cpu(lines, match, members, lower).tolist()
    mem = members.tolist()
    ev = match["event_id"].tolist()
    for i in range(B):
        for c in range(C):
            h, any_relevant = FNV_OFFSET, False
            for j in range(off[c], off[c + 1]):
                kind, event = mem[j][0], mem[j][1]
                r = 1 if (kind != 0 or event < 0 or ev[i] == event) else 0
                any_relevant = any_relevant or bool(r)
                m = mh[i][j] & _U64
                h = ((h ^ r) * FNV_PRIME) & _U64
                for b in range(8):
                    h = ((h ^ ((m >> (8 * b)) & 0xFF)) * FNV_PRIME) & _U64
            out[i, W + c] = _as_i64(h | 1) if any_relevant else 0
    return out


def watch_combo_hashes(
    lines, match: dict, specs: torch.Tensor, members: torch.Tensor,
    combo_off: torch.Tensor, lower: bool = False,
) -> torch.Tensor:
    """Watch hashes and combination hashes of a parsed batch, [B, W + C]."""
    if lines.is_cuda:
        return _require_ext().watch_combo_hashes(
            *_parsed_args(lines, match), specs, members, combo_off, lower)
    return watch_combo_hashes_cpu(lines, match, specs, members, combo_off, lower)


# ---------------------------------------------------------------------------
# detector: event-rate windows (docs/kernels.md, "Event-rate windows" is the
# definition; event_rate.hip and event_rate_step_cpu below implement it)
# ---------------------------------------------------------------------------

#: kernels.h limits, repeated here so that a CPU-only install can refuse a
#: configuration the GPU could not run (tests compare them to the extension's)
ER_MAX_EVENTS = 8192
ER_MAX_CELLS = 1 << 24

#: FrequencyDetectorConfig's keys and defaults
EVENT_RATE_DEFAULTS = {
    "window_lines": 1000,
    "ewma_alpha": 0.3,
    "z_threshold": 4.0,
    "min_windows": 3,
}


def event_rate_slots(B: int, window_lines: int) -> int:
    """Window slots of one call: B lines on top of an open window complete
    at most B // L + 1 windows and leave one open."""
    return B // int(window_lines) + 2


def _check_event_rate_params(window_lines, ewma_alpha, z_threshold, min_windows) -> None:
    if not 1 <= int(window_lines) <= 2**31 - 1:
        raise ValueError(f"window_lines must be within 1 .. 2^31 - 1, got {window_lines}")
    if not 0.0 < float(ewma_alpha) <= 1.0:
        raise ValueError(f"ewma_alpha must be in (0, 1], got {ewma_alpha}")
    if not float(z_threshold) >= 0.0:
        raise ValueError(f"z_threshold must be >= 0, got {z_threshold}")
    if not 0 <= int(min_windows) <= 2**31 - 1:
        raise ValueError(f"min_windows must be within 0 .. 2^31 - 1, got {min_windows}")


def event_rate_step_cpu(
    event_id: torch.Tensor,
    n_valid,
    mean: torch.Tensor,
    var: torch.Tensor,
    known: torch.Tensor,
    open_counts: torch.Tensor,
    ctl: torch.Tensor,
    train_upto: int,
    window_lines: int,
    ewma_alpha: float,
    z_threshold: float,
    min_windows: int,
):
    """CPU mirror of ``_dmx_C.event_rate_step``: same arguments, the state
    tensors (mean, var f64 [E]; known, open_counts int32 [E]; ctl int32 [2])
    updated in place, same outputs (rate_counts int32 [NW, E], rate_z f64
    [NW, E], rate_hits int32 [B], rate_slot int32 [B]). numpy f64, one
    rounding per operation, in the order docs/kernels.md gives."""
    import numpy as np

    _check_event_rate_params(window_lines, ewma_alpha, z_threshold, min_windows)
    B, E, L = int(event_id.shape[0]), int(mean.shape[0]), int(window_lines)
    if not 1 <= E <= ER_MAX_EVENTS:
        raise ValueError(f"mean: E = {E} bins must be within 1 .. {ER_MAX_EVENTS}")
    for name, t in (("var", var), ("known", known), ("open_counts", open_counts)):
        if tuple(t.shape) != (E,):
            raise ValueError(f"{name} must hold E = {E} elements, got {list(t.shape)}")
    if not 0 <= int(train_upto) <= B:
        raise ValueError(f"train_upto must be within 0 .. B = {B}, got {train_upto}")
    NW = event_rate_slots(B, L)
    if NW * E > ER_MAX_CELLS:
        raise ValueError(f"NW * E = {NW} * {E} must not exceed {ER_MAX_CELLS}")
    z_out = np.zeros((NW, E), dtype=np.float64)
    hits = np.zeros(B, dtype=np.int32)
    slot = np.full(B, -1, dtype=np.int32)
    if B == 0:
        return (torch.zeros((NW, E), dtype=torch.int32), torch.from_numpy(z_out),
                torch.from_numpy(hits), torch.from_numpy(slot))

    m, v = mean.numpy(), var.numpy()  # views: the state is updated in place
    kn, oc, ct = known.numpy(), open_counts.numpy(), ctl.numpy()
    n = min(max(int(n_valid), 0), B)
    p = min(max(int(ct[0]), 0), L - 1)
    windows_seen = int(ct[1])
    a = float(ewma_alpha)
    one_minus_a = 1.0 - a

    ev = event_id.numpy()[:n].astype(np.int64)
    bins = np.where(ev < 0, 0, ev)
    counted = (ev != 0) & (bins < E)
    slot_of = (p + np.arange(n, dtype=np.int64)) // L
    counts = np.bincount(slot_of[counted] * E + bins[counted], minlength=NW * E)
    counts = counts.reshape(NW, E).astype(np.int32)
    counts[0] += oc

    nc = min((p + n) // L, NW - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(nc):
            boundary = (s + 1) * L - p - 1
            slot[boundary] = s
            report = boundary >= train_upto and windows_seen + s >= min_windows
            c = counts[s].astype(np.float64)
            k = kn != 0
            z = (c - m) / np.sqrt(np.maximum(v, 1.0))
            flag = k & (np.abs(z) > z_threshold) & report
            d = c - m
            first = ~k & (c > 0)
            new_m = a * c + one_minus_a * m
            new_v = a * (d * d) + one_minus_a * v
            m[:] = np.where(k, new_m, np.where(first, c, m))
            v[:] = np.where(k, new_v, np.where(first, np.maximum(c, 1.0), v))
            kn[first] = 1
            z_out[s] = np.where(flag, z, 0.0)
            hits[boundary] = int(flag.sum())
    oc[:] = counts[nc]
    ct[0] = (p + n) % L
    ct[1] = windows_seen + nc
    return (torch.from_numpy(counts), torch.from_numpy(z_out),
            torch.from_numpy(hits), torch.from_numpy(slot))


def event_rate_step(event_id, n_valid, mean, var, known, open_counts, ctl,
                    train_upto, window_lines, ewma_alpha, z_threshold, min_windows):
    """One batch of the event-rate stage on event_id's device."""
    fn = _require_ext().event_rate_step if event_id.is_cuda else event_rate_step_cpu
    return fn(event_id, n_valid, mean, var, known, open_counts, ctl,
              int(train_upto), int(window_lines), float(ewma_alpha),
              float(z_threshold), int(min_windows))


class EventRateState:
    """Per-stream state of the event-rate stage, resident on ``device``: the
    EWMA baseline (``mean``, ``var`` f64 [E]), ``known`` and the open
    window's ``open_counts`` (int32 [E]) and ``ctl`` = (in_window,
    windows_seen), for E = n_templates + 1 bins (bin 0 = unparsed lines).
    ``step`` advances it by one batch without a host read, so it can be
    captured into a hipGraph; restoring a checkpoint writes into the same
    tensors, which a captured graph keeps reading."""

    def __init__(self, n_templates: int, window_lines: int = 1000,
                 ewma_alpha: float = 0.3, z_threshold: float = 4.0,
                 min_windows: int = 3, device="cpu") -> None:
        _check_event_rate_params(window_lines, ewma_alpha, z_threshold, min_windows)
        if not 0 <= int(n_templates) <= ER_MAX_EVENTS - 1:
            raise ValueError(
                f"event_rate supports at most ER_MAX_EVENTS - 1 = {ER_MAX_EVENTS - 1} "
                f"templates, got {n_templates}")
        self.E = int(n_templates) + 1
        self.window_lines = int(window_lines)
        self.ewma_alpha = float(ewma_alpha)
        self.z_threshold = float(z_threshold)
        self.min_windows = int(min_windows)
        self.device = torch.device(device)
        self.mean = torch.zeros(self.E, dtype=torch.float64, device=self.device)
        self.var = torch.zeros(self.E, dtype=torch.float64, device=self.device)
        self.known = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        self.open_counts = torch.zeros(self.E, dtype=torch.int32, device=self.device)
        self.ctl = torch.zeros(2, dtype=torch.int32, device=self.device)
        # the row count handed to the kernels: a device word, rewritten only
        # when the count changes (a captured graph reads it at replay)
        self.n_valid = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._n_valid_host = 0

    _STATE = ("mean", "var", "known", "open_counts", "ctl")

    def set_n_valid(self, n: int) -> None:
        if int(n) != self._n_valid_host:
            self.n_valid.fill_(int(n))
            self._n_valid_host = int(n)

    def step(self, event_id: torch.Tensor, n_valid: Optional[int] = None,
             train_upto: int = 0) -> dict:
        """Count the first ``n_valid`` rows (default: all) of event_id [B]
        and roll every window they complete. ``n_valid=None`` inside a graph
        capture would record the write; callers that capture set it first
        with set_n_valid()."""
        self.set_n_valid(event_id.shape[0] if n_valid is None else n_valid)
        counts, z, hits, slot = event_rate_step(
            event_id, self.n_valid, self.mean, self.var, self.known,
            self.open_counts, self.ctl, train_upto, self.window_lines,
            self.ewma_alpha, self.z_threshold, self.min_windows)
        return {"rate_counts": counts, "rate_z": z, "rate_hits": hits,
                "rate_slot": slot}

    def state_dict(self) -> dict:
        state = {k: getattr(self, k).detach().cpu().clone() for k in self._STATE}
        state["window_lines"] = self.window_lines
        return state

    def load_state_dict(self, state: dict) -> None:
        if int(state["window_lines"]) != self.window_lines:
            raise ValueError(
                f"event-rate checkpoint was taken with window_lines = "
                f"{int(state['window_lines'])} but this instance is configured "
                f"for {self.window_lines} (its open window would not line up)")
        for k in self._STATE:
            mine = getattr(self, k)
            if tuple(state[k].shape) != tuple(mine.shape):
                raise ValueError(
                    f"event-rate checkpoint holds {k} {list(state[k].shape)} but "
                    f"this instance is configured for {list(mine.shape)} "
                    "(templates + 1 bins)")
        for k in self._STATE:
            mine = getattr(self, k)
            mine.copy_(state[k].to(mine.dtype))


# ---------------------------------------------------------------------------
# detector: numeric value ranges (docs/kernels.md, "Value ranges" is the
# definition; value_range.hip and value_range_step_cpu below implement it)
# ---------------------------------------------------------------------------

#: kernels.h limits of the grammar (tests compare them to the extension's)
VR_MAX_SPAN = 17
VR_MAX_DIGITS = 15

_VR_NUMBER = re.compile(rb"[+-]?[0-9]+(\.[0-9]+)?")
_RANGE_KEYS = ("kind", "pos", "event", "name", "slack", "non_numeric", "min", "max")


def parse_number(span: bytes) -> Optional[float]:
    """The value of ``span`` under the "Value ranges" grammar, or None when
    it is not a number: the regular expression, the two length limits and
    Python's correctly rounded ``float()``, with 0.0 in place of -0.0."""
    if len(span) > VR_MAX_SPAN or _VR_NUMBER.fullmatch(span) is None:
        return None
    if sum(48 <= c <= 57 for c in span) > VR_MAX_DIGITS:
        return None
    v = float(span.decode("ascii"))
    return 0.0 if v == 0.0 else v


def range_spec_row(r: dict) -> List[int]:
    """One range dict -> the kernel's spec row (kind, event, pos, flags):
    a watch row whose pad word holds the flags, bit 0 = non_numeric alert."""
    kind, event, pos, _ = watch_spec_row(r)
    return [kind, event, pos, 1 if r.get("non_numeric", "ignore") == "alert" else 0]


def range_name(r: dict) -> str:
    """Alert name of a range: its ``name`` or ``variable <pos>`` /
    ``header <pos>``."""
    if r.get("name"):
        return str(r["name"])
    kind = "variable" if r.get("kind", "variable") == "variable" else "header"
    return f"{kind} {int(r['pos'])}"


def pack_ranges(specs: Sequence[dict]):
    """List of range dicts -> (specs int32 [R, 4], slack f64 [R], lo f64
    [R], hi f64 [R]) on the CPU: the host-side validation of everything the
    kernels trust, and the start state (lo = +inf, hi = -inf, or the
    configured min / max)."""
    rows, slack, lo, hi = [], [], [], []
    for i, r in enumerate(specs):
        unknown = set(r) - set(_RANGE_KEYS)
        if unknown:
            raise ValueError(
                f"range {i}: unknown key(s) {sorted(unknown)}; valid keys: "
                f"{sorted(_RANGE_KEYS)}")
        if "pos" not in r:
            raise ValueError(f"range {i} has no 'pos': {dict(r)!r}")
        if r.get("kind", "variable") not in ("variable", "header"):
            raise ValueError(
                f"range {i}: 'kind' must be 'variable' or 'header', got {r['kind']!r}")
        if r.get("non_numeric", "ignore") not in ("ignore", "alert"):
            raise ValueError(
                f"range {i}: 'non_numeric' must be 'ignore' or 'alert', "
                f"got {r['non_numeric']!r}")
        row = range_spec_row(r)
        if row[2] < 0:
            raise ValueError(f"range {i}: 'pos' must be >= 0, got {row[2]}")
        s = float(r.get("slack", 0.0))
        if not (math.isfinite(s) and s >= 0.0):
            raise ValueError(f"range {i}: 'slack' must be finite and >= 0, got {s}")
        if ("min" in r) != ("max" in r):
            raise ValueError(f"range {i}: 'min' and 'max' are given both or neither")
        if "min" in r:
            # + 0.0 turns -0.0 into 0.0, the only zero the parser yields
            a, b = float(r["min"]) + 0.0, float(r["max"]) + 0.0
            if not (math.isfinite(a) and math.isfinite(b)):
                raise ValueError(f"range {i}: 'min' and 'max' must be finite, got {a}, {b}")
            if a > b:
                raise ValueError(f"range {i}: 'min' = {a} exceeds 'max' = {b}")
        else:
            a, b = math.inf, -math.inf
        rows.append(row)
        slack.append(s)
        lo.append(a)
        hi.append(b)
    return (
        torch.tensor(rows, dtype=torch.int32).reshape(-1, 4),
        torch.tensor(slack, dtype=torch.float64),
        torch.tensor(lo, dtype=torch.float64),
        torch.tensor(hi, dtype=torch.float64),
    )


def value_range_step_cpu(lines, match: dict, specs, slack, lo, hi, n, train_upto: int):
    """CPU mirror of ``_dmx_C.value_range_step``: lo, hi (f64 [R]) and n
    (int64 [R]) are updated in place by the rows below train_upto, then
    every (line, range) cell is judged against the updated state. Returns
    (range_code int32 [B, R], range_value f64 [B, R]). Values come from
    parse_number, the compares are Python floats: IEEE f64, one rounding
    per operation."""
    B, max_len = int(lines.shape[0]), int(lines.shape[1])
    R = int(specs.shape[0])
    if R < 1 or tuple(specs.shape) != (R, 4):
        raise ValueError(f"specs must be int32 [R >= 1, 4], got {list(specs.shape)}")
    for name, t in (("slack", slack), ("lo", lo), ("hi", hi), ("n", n)):
        if tuple(t.shape) != (R,):
            raise ValueError(f"{name} must hold R = {R} elements, got {list(t.shape)}")
    if not 0 <= int(train_upto) <= B:
        raise ValueError(f"train_upto must be within 0 .. B = {B}, got {train_upto}")
    code = torch.zeros((B, R), dtype=torch.int32)
    value = torch.zeros((B, R), dtype=torch.float64)
    if B == 0:
        return code, value
    rows = [bytes(x) for x in lines.numpy()]
    parsed = [t.tolist() for t in _parsed_args(lines, match)[1:]]
    spec = specs.tolist()
    sl = slack.tolist()
    # the bytes range r reads on line i; None when the range is not relevant
    # for the line or the field is absent
    spans = [[None for _ in range(R)] for _ in range(B)]
    for i in range(B):
        for r in range(R):
            span = _field_span(parsed, max_len, spec[r], i)
            if span is not None:
                spans[i][r] = rows[i][span[0]:span[1]]
    vals = [[None if s is None else parse_number(s) for s in row] for row in spans]
    for r in range(R):
        a, b, cnt = float(lo[r]), float(hi[r]), int(n[r])
        for i in range(int(train_upto)):
            v = vals[i][r]
            if v is not None:
                a, b, cnt = min(a, v), max(b, v), cnt + 1
        lo[r], hi[r], n[r] = a, b, cnt
        alert_nan = bool(spec[r][3] & 1)
        for i in range(B):
            v = vals[i][r]
            if v is not None:
                value[i, r] = v
            if i < train_upto or spans[i][r] is None:
                continue
            if v is None:
                code[i, r] = 3 if alert_nan else 0
            elif a <= b:
                w = b - a
                m = sl[r] * w
                if v < a - m:
                    code[i, r] = 1
                elif v > b + m:
                    code[i, r] = 2
    return code, value


def value_range_step(lines, match: dict, specs, slack, lo, hi, n, train_upto: int):
    """One batch of the value-range stage on lines' device."""
    if lines.is_cuda:
        code, value = _require_ext().value_range_step(
            *_parsed_args(lines, match), specs, slack, lo, hi, n, int(train_upto))
        return code, value
    return value_range_step_cpu(lines, match, specs, slack, lo, hi, n, int(train_upto))


class ValueRangeState:
    """The value-range stage's tensors on ``device``: the packed specs and
    ``slack`` (constant) and the learned ``lo``, ``hi`` (f64 [R]) and ``n``
    (int64 [R]). ``step`` fits and judges one batch without a host read, so
    it can be captured into a hipGraph; ``load_state_dict`` and ``merge_``
    write into the same tensors, which a captured graph keeps reading."""

    _STATE = ("lo", "hi", "n")

    def __init__(self, specs: Sequence[dict], device="cpu") -> None:
        if len(specs) == 0:
            raise ValueError("ValueRangeState needs at least one range")
        rows, slack, lo, hi = pack_ranges(specs)
        self.R = int(rows.shape[0])
        self.names = [range_name(r) for r in specs]
        self.device = torch.device(device)
        self.specs = rows.to(self.device)
        self.slack = slack.to(self.device)
        self.lo = lo.to(self.device)
        self.hi = hi.to(self.device)
        self.n = torch.zeros(self.R, dtype=torch.int64, device=self.device)

    def step(self, lines: torch.Tensor, match: dict, train_upto: int = 0):
        """(range_code int32 [B, R], range_value f64 [B, R]) of one parsed
        batch; rows below train_upto move lo, hi and n first."""
        return value_range_step(lines, match, self.specs, self.slack, self.lo,
                                self.hi, self.n, train_upto)

    def state_dict(self) -> dict:
        return {k: getattr(self, k).detach().cpu().clone() for k in self._STATE}

    def load_state_dict(self, state: dict) -> None:
        for k in self._STATE:
            if tuple(state[k].shape) != (self.R,):
                raise ValueError(
                    f"value-range checkpoint holds {k} {list(state[k].shape)} but "
                    f"this instance is configured for R = {self.R} ranges")
        for k in self._STATE:
            mine = getattr(self, k)
            mine.copy_(state[k].to(mine.dtype))

    def merge_(self, lo: torch.Tensor, hi: torch.Tensor, n: torch.Tensor) -> None:
        """Fold another state of the same ranges into this one, in place:
        lo = min, hi = max, n = sum."""
        for name, t in (("lo", lo), ("hi", hi), ("n", n)):
            if tuple(t.shape) != (self.R,):
                raise ValueError(
                    f"merge_: {name} must hold R = {self.R} elements, got {list(t.shape)}")
        self.lo.copy_(torch.minimum(self.lo, lo.to(self.lo)))
        self.hi.copy_(torch.maximum(self.hi, hi.to(self.hi)))
        self.n.add_(n.to(self.n))


# ---------------------------------------------------------------------------
# detector: event sequences (docs/kernels.md, "Event sequences" is the
# definition; event_sequence.hip and event_sequence_step_cpu below implement it)
# ---------------------------------------------------------------------------

#: kernels.h limits, repeated here so that a CPU-only install can refuse a
#: configuration the GPU could not run (tests compare them to the extension's)
SEQ_MAX_LEN = 4
SEQ_MAX_KEYS = 1 << 24
SEQ_MAX_EVENTS = 65535

#: the keys of `event_sequence:` and their defaults (capacity None = the
#: pipeline's hashset_capacity)
EVENT_SEQUENCE_DEFAULTS = {
    "length": 3,
    "key": None,
    "max_keys": 1 << 16,
    "capacity": None,
}
_SEQ_KEY_KEYS = ("kind", "pos", "event", "name")


def _check_event_sequence_params(length, max_keys, n_templates) -> None:
    if not 2 <= int(length) <= SEQ_MAX_LEN:
        raise ValueError(
            f"length must be within 2 .. SEQ_MAX_LEN = {SEQ_MAX_LEN}, got {length}")
    K = int(max_keys)
    if not (1 <= K <= SEQ_MAX_KEYS and K & (K - 1) == 0):
        raise ValueError(
            f"max_keys must be a power of two within 1 .. SEQ_MAX_KEYS = "
            f"{SEQ_MAX_KEYS}, got {max_keys}")
    if not 0 <= int(n_templates) <= SEQ_MAX_EVENTS:
        raise ValueError(
            f"event_sequence supports at most SEQ_MAX_EVENTS = {SEQ_MAX_EVENTS} "
            f"templates (a symbol is 16 bits), got {n_templates}")


def sequence_key_row(key: Optional[dict]) -> Tuple[int, int, int]:
    """The `key:` entry of event_sequence -> (kind, event, pos) of its watch
    spec, or (-1, -1, 0) for no key."""
    if key is None:
        return (-1, -1, 0)
    unknown = set(key) - set(_SEQ_KEY_KEYS)
    if unknown:
        raise ValueError(
            f"event_sequence key: unknown key(s) {sorted(unknown)}; valid keys: "
            f"{sorted(_SEQ_KEY_KEYS)}")
    if "pos" not in key:
        raise ValueError(f"event_sequence key has no 'pos': {dict(key)!r}")
    if key.get("kind", "variable") not in ("variable", "header"):
        raise ValueError(
            f"event_sequence key: 'kind' must be 'variable' or 'header', "
            f"got {key['kind']!r}")
    kind, event, pos, _ = watch_spec_row(key)
    if pos < 0:
        raise ValueError(f"event_sequence key: 'pos' must be >= 0, got {pos}")
    return (kind, event, pos)


def sequence_bucket(kh: int, max_keys: int) -> int:
    """Bucket of key hash ``kh`` (unsigned or int64 view) among max_keys."""
    kh &= _U64
    return ((kh >> 32) ^ kh) & (int(max_keys) - 1)


def gram_hash(gram: int) -> int:
    """Hash of a gram word: its 8 bytes, low byte first, folded FNV-1a style
    and forced odd (unsigned)."""
    h = FNV_OFFSET
    for b in range(8):
        h = ((h ^ ((gram >> (8 * b)) & 0xFF)) * FNV_PRIME) & _U64
    return h | 1


def event_sequence_step_cpu(lines, match: dict, key_row, lower: bool, n_valid,
                            n_templates: int, seq_key, seq_hist, length: int):
    """CPU mirror of ``_dmx_C.event_sequence_step``: the sequential loop of
    the definition over the member rows, in row order. seq_key and seq_hist
    (int64 [K]) are updated in place; returns (seq_gram int64 [B], gram_hash
    int64 [B, 1]). Plain Python integers throughout."""
    B, max_len = int(lines.shape[0]), int(lines.shape[1])
    K, n = int(seq_key.shape[0]), int(length)
    _check_event_sequence_params(n, K, n_templates)
    if tuple(seq_hist.shape) != (K,):
        raise ValueError(f"seq_hist must hold K = {K} elements, got {list(seq_hist.shape)}")
    kind, event, pos = key_row
    grams = torch.zeros(B, dtype=torch.int64)
    hashes = torch.zeros((B, 1), dtype=torch.int64)
    if B == 0:
        return grams, hashes
    nv = min(max(int(n_valid), 0), B)
    ev = match["event_id"].tolist()
    parsed = [t.tolist() for t in _parsed_args(lines, match)[1:]] if kind >= 0 else None
    rows = lines.numpy()
    gram_mask = (1 << (16 * n)) - 1
    hist_mask = (1 << (16 * (n - 1))) - 1
    for i in range(nv):
        if not 1 <= ev[i] <= int(n_templates):
            continue
        if kind >= 0:
            span = _field_span(parsed, max_len, (kind, event, pos, 0), i)
            if span is None:
                continue
            kh = fnv1a64(rows[i, span[0]:span[1]].tobytes(), lower)
        else:
            kh = 1
        b = sequence_bucket(kh, K)
        if int(seq_key[b]) & _U64 != kh:  # take the bucket over
            seq_key[b] = _as_i64(kh)
            seq_hist[b] = 0
        gram = (((int(seq_hist[b]) & _U64) << 16) | ev[i]) & gram_mask
        seq_hist[b] = _as_i64(gram & hist_mask)
        grams[i] = _as_i64(gram)
        hashes[i, 0] = _as_i64(gram_hash(gram))
    return grams, hashes


def event_sequence_step(lines, match: dict, key_row, lower: bool, n_valid,
                        n_templates: int, seq_key, seq_hist, length: int):
    """One batch of the event-sequence stage on lines' device."""
    if lines.is_cuda:
        gram, hashes = _require_ext().event_sequence_step(
            *_parsed_args(lines, match), int(key_row[0]), int(key_row[1]),
            int(key_row[2]), bool(lower), n_valid, int(n_templates), seq_key,
            seq_hist, int(length))
        return gram, hashes
    return event_sequence_step_cpu(lines, match, key_row, lower, n_valid,
                                   n_templates, seq_key, seq_hist, length)


def decode_gram(gram: int, length: int) -> List[int]:
    """The ``length`` symbols of a gram word, oldest first, 0 = pad."""
    gram &= _U64
    return [(gram >> (16 * j)) & 0xFFFF for j in range(int(length) - 1, -1, -1)]


def sequence_text(symbols: Sequence[int], key_name: Optional[str] = None) -> str:
    """Alert wording of an unknown gram: "unknown event sequence: ^ > 3 > 7
    (per ses)", ^ for a pad."""
    text = "unknown event sequence: " + " > ".join(
        "^" if s == 0 else str(s) for s in symbols)
    return text + (f" (per {key_name})" if key_name else "")


class EventSequenceState:
    """Per-key histories of the event-sequence stage, resident on ``device``:
    ``seq_key`` (the key hash that owns each of the K = max_keys buckets, 0 =
    nobody) and ``seq_hist`` (its last length - 1 event ids, 16 bits each),
    both int64 [K]. ``step`` advances them by one batch without a host read,
    so it can be captured into a hipGraph; restoring a checkpoint writes into
    the same tensors, which a captured graph keeps reading."""

    _STATE = ("seq_key", "seq_hist")

    def __init__(self, n_templates: int, length: int = 3, max_keys: int = 1 << 16,
                 key: Optional[dict] = None, lowercase: bool = False,
                 device="cpu") -> None:
        _check_event_sequence_params(length, max_keys, n_templates)
        self.n_templates = int(n_templates)
        self.length = int(length)
        self.max_keys = int(max_keys)
        self.key_row = sequence_key_row(key)
        self.key_name = (key or {}).get("name")
        self.lowercase = bool(lowercase)
        self.device = torch.device(device)
        self.seq_key = torch.zeros(self.max_keys, dtype=torch.int64, device=self.device)
        self.seq_hist = torch.zeros(self.max_keys, dtype=torch.int64, device=self.device)
        # the row count handed to the kernels: a device word, rewritten only
        # when the count changes (a captured graph reads it at replay)
        self.n_valid = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._n_valid_host = 0

    def set_n_valid(self, n: int) -> None:
        if int(n) != self._n_valid_host:
            self.n_valid.fill_(int(n))
            self._n_valid_host = int(n)

    def step(self, lines: torch.Tensor, match: dict, n_valid: Optional[int] = None):
        """(seq_gram int64 [B], gram_hash int64 [B, 1]) of one parsed batch;
        the first ``n_valid`` rows (default: all) move the histories.
        ``n_valid=None`` inside a graph capture would record the write;
        callers that capture set it first with set_n_valid()."""
        self.set_n_valid(lines.shape[0] if n_valid is None else n_valid)
        return event_sequence_step(
            lines, match, self.key_row, self.lowercase, self.n_valid,
            self.n_templates, self.seq_key, self.seq_hist, self.length)

    def state_dict(self) -> dict:
        state = {k: getattr(self, k).detach().cpu().clone() for k in self._STATE}
        state["length"] = self.length
        state["max_keys"] = self.max_keys
        return state

    def load_state_dict(self, state: dict) -> None:
        for k in ("length", "max_keys"):
            if int(state[k]) != getattr(self, k):
                raise ValueError(
                    f"event-sequence checkpoint was taken with {k} = {int(state[k])} "
                    f"but this instance is configured for {getattr(self, k)} "
                    "(its histories would mean other grams)")
        for k in self._STATE:
            if tuple(state[k].shape) != (self.max_keys,):
                raise ValueError(
                    f"event-sequence checkpoint holds {k} {list(state[k].shape)} but "
                    f"this instance is configured for max_keys = {self.max_keys}")
        for k in self._STATE:
            mine = getattr(self, k)
            mine.copy_(state[k].to(mine.dtype))
