"""Fused BERT kernel with the explicit operand pipeline: weight fragments
of a quad in flight before its first MFMA, the next quad's issued ahead of
the epilogue, and the barrier in front of each GEMM executed inside
block_gemm (run on an MI355X with `-m gpu`).

The pipeline reorders loads and moves barriers but leaves every K chain as
it was, so the checks are: still the fp32 model's scores, no race across a
moved barrier (bit-identical reruns and rows), and the probe, timed and
embedding variants still the production kernel.

Models and inputs as in tests/test_bert_fused_epilogue.py: random weights,
every bias and LayerNorm affine randomised, spans on every edge of the
embed phase."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_LEN = 256
S = 64   # tokens per line of the fused geometry
H = 128  # hidden size of the fused geometry

# (start, end) content spans that hit every edge of the embed phase
EDGE_SPANS = [
    (0, 65),      # truncation: one byte more than fits
    (0, 0),       # empty span: every token is padding
    (192, 256),   # exactly S bytes, ending at max_len
    (0, 64),      # exact fit
    (0, 63),      # one token of padding
    (7, 8),       # span of 1, non-zero start
    (100, 141),   # non-zero start, padded
    (250, 256),   # short span ending at max_len
    (193, 256),   # 63 bytes ending at max_len
    (31, 131),    # non-zero start, truncated
    (12, 12),     # empty span at a non-zero start
]


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from detectmateservice_amd import ops

    assert ops.have_extension(), "HIP extension _dmx_C not built/loadable"
    yield


def _randomize_affine(model, seed):
    """Same random biases / LN affines for a given seed on any device."""
    g = torch.Generator().manual_seed(seed)

    def rnd(like, std, mean=0.0):
        v = torch.randn(like.shape, generator=g) * std + mean
        return v.to(like.dtype).to(like.device)

    for layer in model.layers:
        for k in ("bqkv", "bo", "b1", "b2"):
            layer[k] = rnd(layer[k], 0.05)
        for k in ("ln1_g", "ln2_g"):
            layer[k] = rnd(layer[k], 0.1, 1.0)
        for k in ("ln1_b", "ln2_b"):
            layer[k] = rnd(layer[k], 0.05)
    model.b_score = rnd(model.b_score, 0.05)
    model._wb = model._fb = None
    return model


def _models(layers, seed):
    from detectmateservice_amd.models.bert_tiny import (
        BertTinyConfig,
        BertTinyDetectorModel,
    )

    cfg = BertTinyConfig(layers=layers)
    gpu = _randomize_affine(BertTinyDetectorModel(cfg, device="cuda", seed=seed), seed + 1)
    cpu = _randomize_affine(BertTinyDetectorModel(cfg, device="cpu", seed=seed), seed + 1)
    assert gpu._fused_ok()
    return gpu, cpu


def _edge_batch(B, seed):
    """[B, MAX_LEN] random bytes and B spans cycling through EDGE_SPANS."""
    g = torch.Generator().manual_seed(seed)
    lines = torch.randint(0, 256, (B, MAX_LEN), generator=g, dtype=torch.uint8)
    spans = [EDGE_SPANS[i % len(EDGE_SPANS)] for i in range(B)]
    start = torch.tensor([s for s, _ in spans], dtype=torch.int32)
    end = torch.tensor([e for _, e in spans], dtype=torch.int32)
    return lines, start, end


def _mixed_batch(B, seed):
    """[B, MAX_LEN] random bytes with random spans: empty, short, exact,
    truncated, anywhere in the line."""
    g = torch.Generator().manual_seed(seed)
    lines = torch.randint(0, 256, (B, MAX_LEN), generator=g, dtype=torch.uint8)
    start = torch.randint(0, MAX_LEN, (B,), generator=g, dtype=torch.int32)
    length = torch.randint(0, 2 * S, (B,), generator=g, dtype=torch.int32)
    end = torch.minimum(start + length, torch.tensor(MAX_LEN, dtype=torch.int32))
    return lines, start, end.int()


@pytest.fixture(scope="module")
def model_pairs():
    return {layers: _models(layers, seed=60 + layers) for layers in (1, 2, 4)}


@pytest.mark.parametrize("B", [11, 1, 3])
@pytest.mark.parametrize("layers", [1, 2, 4])
def test_pipelined_gemms_vs_cpu_reference(model_pairs, layers, B):
    """Bounds are the project's own for this comparison: 0.08 up to 2
    layers, 0.1 at 4. B = 11 is one line per edge span."""
    gpu, cpu = model_pairs[layers]
    lines, start, end = _edge_batch(B, seed=13 * layers + B)
    tokens = cpu.tokenize_spans(lines, start, end)
    assert tokens.shape == (B, S)
    ref = cpu.forward(tokens)
    assert torch.isfinite(ref).all(), "CPU reference itself is not finite"
    fused = gpu.score_spans(lines.cuda(), start.cuda(), end.cuda()).cpu()
    assert torch.isfinite(fused).all()
    diff = (fused - ref).abs()
    bound = 0.08 if layers <= 2 else 0.1
    print(f"layers={layers} B={B}: max |fused - cpu| = {float(diff.max()):.5f}")
    assert diff.max() < bound, (int(diff.argmax()), float(diff.max()))


def test_moved_barriers_do_not_race(model_pairs):
    """2048 blocks: every CU holds two co-resident blocks over several
    rounds. A read of in_lds ahead of the barrier that now sits inside the
    GEMM, or a prefetched weight fragment consumed before it has landed,
    would show as a run-to-run or batch-position difference."""
    gpu, _ = model_pairs[2]
    B = 2048
    lines, start, end = _mixed_batch(B, seed=99)
    assert int((end - start).min()) == 0 and int((end - start).max()) > S
    lines, start, end = lines.cuda(), start.cuda(), end.cuda()
    first = gpu.score_spans(lines, start, end)
    assert torch.isfinite(first).all()
    for run in (1, 2):
        again = gpu.score_spans(lines, start, end)
        bad = (again != first).nonzero().flatten().tolist()
        assert not bad, f"launch {run}: rows {bad[:8]} differ from launch 0"
    for i in (0, 1, 1023, 2047):
        alone = gpu.score_spans(lines[i:i + 1], start[i:i + 1], end[i:i + 1])
        assert torch.equal(alone[0], first[i]), (
            f"row {i}: {float(alone[0])!r} alone, {float(first[i])!r} in the batch")


def test_variants_mirror_production(model_pairs):
    """Through the bindings the tools/probe_bert_*.py scripts use."""
    from detectmateservice_amd.ops import _dmx_C

    gpu, _ = model_pairs[2]
    wb, fb = gpu._fused_blobs()
    B = 64
    lines, start, end = _edge_batch(B, seed=21)
    lines, start, end = lines.cuda(), start.cuda(), end.cuda()
    prod = _dmx_C.bert_fused_bf16(lines, start, end, wb, fb, 2, 1e-5)
    assert torch.isfinite(prod).all()

    full = _dmx_C.bert_fused_probe(lines, start, end, wb, fb, 2, 1e-5, 31)
    assert torch.equal(full, prod), "PH_ALL / ABL 0 probe is not the production kernel"

    scores, stamps = _dmx_C.bert_fused_timed(lines, start, end, wb, fb, 2, 1e-5)
    assert torch.equal(scores, prod), "timed variant scores differ"
    st = stamps.cpu()
    # 2 layers use 3 + 2 * 8 + 1 = 20 slots per wave: work done / barrier
    # crossed pairs in schedule order, the crossed ones now taken inside the
    # GEMM that executes the barrier
    used = 3 + 2 * 8 + 1
    assert st.shape[0] == B and st.shape[-1] >= used
    assert (st[..., :used] > 0).all(), "a used stamp slot was never written"
    assert (st[..., 1:used] >= st[..., :used - 1]).all(), "stamp slots out of order"
    assert (st[..., used:] == 0).all(), "unused stamp slots are not zero"

    # the embedding head runs the same schedule: its pooled vector gives the
    # production score up to the order of one H-term f32 sum
    m = gpu.embed_spans(lines, start, end)
    assert m.shape == (B, H) and m.dtype == torch.float32
    terms = m.double().cpu() * gpu.w_score.double().cpu().reshape(1, H)
    ref = terms.sum(dim=1) + gpu.b_score.double().cpu()
    bound = H * 2.0 ** -23 * terms.abs().sum(dim=1)
    err = (prod.double().cpu() - ref).abs()
    print(f"embed head: max err {float(err.max()):.3e}, min bound {float(bound.min()):.3e}")
    assert (err <= bound).all(), (int((err - bound).argmax()), float(err.max()))
