"""The launch contract between Python and the HIP kernels, checked without
a GPU: the fused-BERT blob layout the extension reports matches what
``_fused_blobs`` packs, the geometry gate holds no numbers of its own, and
every GPU binding rejects a malformed argument with a RuntimeError that
names it before anything could reach a device."""
import contextlib
import dataclasses
import re

import pytest
import torch

from detectmateservice_amd import ops
from detectmateservice_amd.models.bert_tiny import (
    BertTinyConfig,
    BertTinyDetectorModel,
)

pytestmark = pytest.mark.skipif(
    not ops.have_extension(), reason="HIP extension _dmx_C not built"
)

if ops.have_extension():
    from detectmateservice_amd.ops import _dmx_C


# ---------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------


def _randomised_model(n_layers: int) -> BertTinyDetectorModel:
    """CPU model whose every packed tensor holds distinct seeded values
    (the default init leaves biases 0 and LN gains 1, which would let a
    misplaced slice compare equal)."""
    m = BertTinyDetectorModel(BertTinyConfig(layers=n_layers), device="cpu")
    g = torch.Generator().manual_seed(100 + n_layers)

    def fill(t):
        return torch.randn(t.shape, generator=g).to(t.dtype)

    m.tok_emb, m.pos_emb = fill(m.tok_emb), fill(m.pos_emb)
    m.w_score, m.b_score = fill(m.w_score), fill(m.b_score)
    for layer in m.layers:
        for k in layer:
            layer[k] = fill(layer[k])
    return m


@pytest.mark.parametrize("n_layers", [1, 2, 4])
def test_fused_blobs_match_extension_layout(n_layers):
    m = _randomised_model(n_layers)
    lay = _dmx_C.bert_fused_layout(n_layers)
    wb, fb = m._fused_blobs()
    assert wb.dtype == torch.bfloat16 and fb.dtype == torch.float32
    assert wb.numel() == lay["wb_elems"]
    assert fb.numel() == lay["fb_elems"]

    def wb_at(off, t):
        assert torch.equal(wb[off:off + t.numel()], t.reshape(-1)), off

    def fb_at(off, t):
        assert torch.equal(fb[off:off + t.numel()], t.reshape(-1)), off

    wb_at(lay["wb_tok"], m.tok_emb)
    wb_at(lay["wb_pos"], m.pos_emb)
    wb_names = {"wqkv_t": "lw_qkv", "wo_t": "lw_wo", "w1_t": "lw_w1",
                "w2_t": "lw_w2", "ln1_g": "lw_ln1g", "ln1_b": "lw_ln1b",
                "ln2_g": "lw_ln2g", "ln2_b": "lw_ln2b"}
    fb_names = {"bqkv": "fb_bqkv", "bo": "fb_bo", "b1": "fb_b1", "b2": "fb_b2"}
    for i, layer in enumerate(m.layers):  # layer 0 ... the last layer
        for k, off in wb_names.items():
            wb_at(lay["wb_layer0"] + i * lay["lw_size"] + lay[off], layer[k])
        for k, off in fb_names.items():
            fb_at(i * lay["fb_size"] + lay[off], layer[k])
    wb_at(lay["wb_score"], m.w_score)
    fb_at(lay["fb_score"], m.b_score)
    # the blobs end exactly where the last named tensor ends
    assert lay["wb_score"] + m.w_score.numel() == lay["wb_elems"]
    assert lay["fb_score"] + m.b_score.numel() == lay["fb_elems"]


def test_fused_geometry_gate():
    assert BertTinyDetectorModel(BertTinyConfig())._fused_geometry_ok()
    base = BertTinyConfig()
    for field, value in [("hidden", 256), ("heads", 4), ("ffn", 1024),
                         ("max_seq", 32), ("vocab_size", 300)]:
        cfg = dataclasses.replace(base, **{field: value})
        m = BertTinyDetectorModel(cfg)
        assert not m._fused_geometry_ok(), field
        assert not m._fused_ok(), field


# ---------------------------------------------------------------------------
# rejection: one violated clause per call, otherwise well-formed CPU
# tensors. Never run where a GPU exists, so a missing check can fail a
# test but cannot reach a device.
# ---------------------------------------------------------------------------

no_gpu = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="malformed arguments are only ever passed where no GPU exists",
)

B = 4


@contextlib.contextmanager
def _rejected(named, device_clause=False):
    """The call inside must raise a RuntimeError that names `named`, and
    must be stopped by the device clause only when the arguments were
    otherwise correct (so a missing check cannot hide behind it)."""
    with pytest.raises(RuntimeError) as exc:
        yield
    msg = str(exc.value).split("\n")[0]
    assert re.search(rf"\b{named}\b", msg), msg
    assert ("must be on a GPU" in msg) == device_clause, msg


def _bf16(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


def _i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def _i64(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def _noncontig(t):
    """Same shape and dtype as t, but a strided view."""
    big = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)
    v = big[..., ::2]
    assert v.shape == t.shape and not v.is_contiguous()
    return v


def _fused_args(n_layers=2):
    lay = _dmx_C.bert_fused_layout(n_layers)
    return dict(
        lines=_u8(B, 64), start=_i32(B), end=_i32(B),
        wb=_bf16(lay["wb_elems"]),
        fb=torch.zeros(lay["fb_elems"], dtype=torch.float32),
        n_layers=n_layers, eps=1e-5,
    )


def _fused_cases(extra=None):
    """(violation id, argument the message must name, kwargs overrides)."""
    a = _fused_args()
    cases = [
        ("device", "lines", {}),
        ("lines-dtype", "lines", {"lines": a["lines"].int()}),
        ("lines-noncontig", "lines", {"lines": _noncontig(a["lines"])}),
        ("start-len", "start", {"start": _i32(B + 1)}),
        ("end-len", "end", {"end": _i32(B - 1)}),
        ("start-dtype", "start", {"start": _i64(B)}),
        ("wb-short", "wb", {"wb": a["wb"][:-1]}),
        ("wb-dtype", "wb", {"wb": a["wb"].float()}),
        ("fb-short", "fb", {"fb": a["fb"][:-1]}),
        ("layers-0", "n_layers", {"n_layers": 0}),
        # blobs sized for 2 layers cannot be indexed as 3
        ("layers-3", "wb", {"n_layers": 3}),
    ]
    return cases + (extra or [])


def _call_fused(fn, overrides, **more):
    a = {**_fused_args(), **more, **overrides}
    order = ["lines", "start", "end", "wb", "fb", "n_layers", "eps"]
    if "phase_mask" in a:
        order.append("phase_mask")
    return fn(*[a[k] for k in order])


@no_gpu
@pytest.mark.parametrize("case", _fused_cases() if ops.have_extension() else [],
                         ids=lambda c: c[0])
@pytest.mark.parametrize("entry", ["bert_fused_bf16", "bert_fused_timed"])
def test_bert_fused_rejects(entry, case):
    _, named, overrides = case
    with _rejected(named, device_clause=not overrides):
        _call_fused(getattr(_dmx_C, entry), overrides)


@no_gpu
@pytest.mark.parametrize(
    "case",
    _fused_cases([("mask-unknown", "phase_mask", {"phase_mask": 99}),
                  ("mask-negative", "phase_mask", {"phase_mask": -1})])
    if ops.have_extension() else [],
    ids=lambda c: c[0])
def test_bert_fused_probe_rejects(case):
    _, named, overrides = case
    with _rejected(named, device_clause=not overrides):
        _call_fused(_dmx_C.bert_fused_probe, overrides, phase_mask=31)


def _tm_args():
    return dict(
        lines=_u8(B, 128), line_len=_i32(B), fmt_bytes=_u8(8),
        fmt_seg_off=_i32(3), seg_bytes=_u8(100), seg_off=_i32(5),
        tpl_seg_start=_i32(3), lower=False, max_fmt_caps=2, max_caps=3,
    )


@no_gpu
@pytest.mark.parametrize("named,overrides", [
    ("lines", {}),  # device clause
    ("lines", {"lines": _u8(B, 1024)}),
    ("lines", {"lines": _noncontig(_u8(B, 128))}),
    ("line_len", {"line_len": _i32(B + 1)}),
    ("line_len", {"line_len": _i64(B)}),
    ("fmt_seg_off", {"fmt_seg_off": _i64(3)}),
    ("seg_off", {"seg_off": _noncontig(_i32(5))}),
    ("tpl_seg_start", {"tpl_seg_start": _i32(3).float()}),
    ("seg_bytes.*70000", {"seg_bytes": _u8(70000)}),
    # fits 64 KiB on its own but not next to the staged lines
    ("seg_bytes.*65000", {"seg_bytes": _u8(65000)}),
])
def test_template_match_rejects(named, overrides):
    with _rejected(named, device_clause=not overrides):
        _dmx_C.template_match(*{**_tm_args(), **overrides}.values())


def _wh_args():
    return dict(
        lines=_u8(B, 128), event_id=_i32(B), caps=_i32(B, 3, 2),
        n_caps=_i32(B), fmt_caps=_i32(B, 2, 2), n_fmt_caps=_i32(B),
        specs=_i32(2, 4), lower=False,
    )


@no_gpu
@pytest.mark.parametrize("named,overrides", [
    ("lines", {}),
    ("lines", {"lines": _u8(B, 128).int()}),
    ("event_id", {"event_id": _i32(B + 1)}),
    ("caps", {"caps": _i64(B, 3, 2)}),
    ("caps", {"caps": _i32(B, 3, 3)}),
    ("caps", {"caps": _i32(B, 6)}),
    ("n_caps", {"n_caps": _i32(B - 1)}),
    ("fmt_caps", {"fmt_caps": _i32(B + 1, 2, 2)}),
    ("fmt_caps", {"fmt_caps": _noncontig(_i32(B, 2, 2))}),
    ("n_fmt_caps", {"n_fmt_caps": _i64(B)}),
    ("specs", {"specs": _i32(2, 3)}),
    ("specs", {"specs": _i64(2, 4)}),
])
def test_watch_hashes_rejects(named, overrides):
    with _rejected(named, device_clause=not overrides):
        _dmx_C.watch_hashes(*{**_wh_args(), **overrides}.values())


@no_gpu
@pytest.mark.parametrize("entry", ["hashset_insert", "hashset_probe"])
@pytest.mark.parametrize("named,hashes,tables", [
    ("device", _i64(B, 2), _i64(2, 64)),
    ("hashes", _i32(B, 2), _i64(2, 64)),
    ("hashes", _i64(B * 2), _i64(2, 64)),
    ("hashes", _noncontig(_i64(B, 2)), _i64(2, 64)),
    ("tables", _i64(B, 2), _i64(3, 64)),  # wrong W
    ("tables", _i64(B, 2), _i32(2, 64)),
    ("tables", _i64(B, 2), _i64(2, 48)),  # capacity not a power of two
    ("tables", _i64(B, 2), _i64(2, 64).t().contiguous().t()),
])
def test_hashset_rejects(entry, named, hashes, tables):
    device = named == "device"
    with _rejected("hashes" if device else named, device_clause=device):
        getattr(_dmx_C, entry)(hashes, tables)


@no_gpu
@pytest.mark.parametrize("named,overrides", [
    ("A", {}),
    ("A", {"A": _u8(3, 64).int()}),
    ("A", {"A": _u8(3, 512), "B": _u8(5, 512)}),
    ("B", {"B": _u8(5, 32)}),
    ("B", {"B": _noncontig(_u8(5, 64))}),
    ("a_len", {"a_len": _i32(4)}),
    ("a_len", {"a_len": _i64(3)}),
    ("b_len", {"b_len": _i32(3)}),
])
def test_edit_distance_rejects(named, overrides):
    a = dict(A=_u8(3, 64), a_len=_i32(3), B=_u8(5, 64), b_len=_i32(5))
    with _rejected(named, device_clause=not overrides):
        _dmx_C.edit_distance(*{**a, **overrides}.values())


@no_gpu
@pytest.mark.parametrize("named,overrides", [
    ("x", {}),
    ("x", {"x": _bf16(8, 128).float()}),
    ("x", {"x": _bf16(8, 100)}),
    ("res", {"res": _bf16(4, 128)}),
    ("res", {"res": _noncontig(_bf16(8, 128))}),
    ("gamma", {"gamma": _bf16(64)}),
    ("gamma", {"gamma": _bf16(128).float()}),
    ("beta", {"beta": _bf16(256)}),
    ("beta", {"beta": _noncontig(_bf16(128))}),
])
def test_layernorm_rejects(named, overrides):
    a = dict(x=_bf16(8, 128), res=_bf16(8, 128), gamma=_bf16(128),
             beta=_bf16(128), eps=1e-5, want_xres=True)
    with _rejected(named, device_clause=not overrides):
        _dmx_C.layernorm_bf16(*{**a, **overrides}.values())


@no_gpu
@pytest.mark.parametrize("named,overrides", [
    ("q", {}),
    ("q", {"q": _bf16(2, 256, 64), "k": _bf16(2, 256, 64), "v": _bf16(2, 256, 64)}),
    ("k", {"k": _bf16(2, 32, 64)}),
    ("k", {"k": _bf16(2, 64, 64).float()}),
    ("v", {"v": _noncontig(_bf16(2, 64, 64))}),
    ("v", {"v": _bf16(3, 64, 64)}),
])
def test_attention_rejects(named, overrides):
    a = dict(q=_bf16(2, 64, 64), k=_bf16(2, 64, 64), v=_bf16(2, 64, 64),
             scale=0.125)
    with _rejected(named, device_clause=not overrides):
        _dmx_C.attention_bf16(*{**a, **overrides}.values())


@no_gpu
@pytest.mark.parametrize("named,overrides", [
    ("qkv", {}),
    ("qkv", {"qkv": _bf16(2, 64, 384).float()}),
    ("qkv", {"qkv": _noncontig(_bf16(2, 64, 384))}),
    ("qkv", {"qkv": _bf16(2, 32, 384)}),   # S disagrees with the tensor
    ("qkv", {"qkv": _bf16(2, 64, 192)}),
    ("S", {"qkv": _bf16(2, 48, 384), "S": 48}),
    ("S", {"qkv": _bf16(2, 160, 384), "S": 160}),
    ("Dh", {"qkv": _bf16(2, 64, 96), "Dh": 16}),
])
def test_attention_qkv_rejects(named, overrides):
    a = dict(qkv=_bf16(2, 64, 384), S=64, H=2, Dh=64, scale=0.125)
    with _rejected(named, device_clause=not overrides):
        _dmx_C.attention_qkv_bf16(*{**a, **overrides}.values())


@no_gpu
@pytest.mark.parametrize("named,overrides", [
    ("x", {}),
    ("x", {"x": _bf16(8, 128).half()}),
    ("x", {"x": _bf16(8, 96), "wt": _bf16(16, 96)}),  # K % 64
    ("wt", {"wt": _bf16(16, 64)}),
    ("wt", {"wt": _noncontig(_bf16(16, 128))}),
    ("bias", {"bias": torch.zeros(15)}),
    ("bias", {"bias": torch.zeros(16, dtype=torch.float64)}),
])
def test_fused_linear_rejects(named, overrides):
    a = dict(x=_bf16(8, 128), wt=_bf16(16, 128), bias=torch.zeros(16),
             epilogue=0)
    with _rejected(named, device_clause=not overrides):
        _dmx_C.fused_linear_bf16(*{**a, **overrides}.values())


@no_gpu
@pytest.mark.parametrize("entry,a_shape,b_shape,extra", [
    ("probe_mfma", (16, 32), (32, 16), (0, 0)),
    ("probe_mfma32", (32, 16), (16, 32), ()),
])
def test_mfma_probes_reject(entry, a_shape, b_shape, extra):
    fn = getattr(_dmx_C, entry)
    A, Bm = _bf16(*a_shape), _bf16(*b_shape)
    with _rejected("A", device_clause=True):
        fn(A, Bm, *extra)
    with _rejected("A"):
        fn(A.float(), Bm, *extra)
    with _rejected("B"):
        fn(A, _noncontig(Bm), *extra)
    with _rejected("B"):
        fn(A, _bf16(*a_shape), *extra)
