"""Fused BERT kernel after the epilogue / softmax instruction diet: the
operand-swapped MFMA tiles, the 8-byte LDS epilogues, the 16-byte bias
loads and the reciprocal-based GELU (run on an MI355X with `-m gpu`).

Weights are random-init and every bias and LayerNorm affine is randomised
too (the model initialises them to 0 / 1, which would hide a bias fetched
from the wrong column), so a transposed or misplaced tile is a gross
error, not a tolerance miss."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_LEN = 256
S = 64  # tokens per line of the fused geometry

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


def _edge_batch(B, seed, first=0):
    """[B, MAX_LEN] random bytes and B spans cycling through EDGE_SPANS."""
    g = torch.Generator().manual_seed(seed)
    lines = torch.randint(0, 256, (B, MAX_LEN), generator=g, dtype=torch.uint8)
    spans = [EDGE_SPANS[(first + i) % len(EDGE_SPANS)] for i in range(B)]
    start = torch.tensor([s for s, _ in spans], dtype=torch.int32)
    end = torch.tensor([e for _, e in spans], dtype=torch.int32)
    return lines, start, end


@pytest.fixture(scope="module")
def model_pairs():
    return {layers: _models(layers, seed=40 + layers) for layers in (1, 2, 4)}


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("layers", [1, 2, 4])
def test_fused_vs_cpu_reference(model_pairs, layers, B):
    """Bounds are the project's own: 0.08 up to 2 layers, 0.1 at 4."""
    gpu, cpu = model_pairs[layers]
    # B=1 takes the truncating span, B=3 adds the empty and the
    # ends-at-max_len one, B=64 cycles through all of them
    lines, start, end = _edge_batch(B, seed=7 * layers + B)
    tokens = cpu.tokenize_spans(lines, start, end)
    assert tokens.shape == (B, S)
    ref = cpu.forward(tokens)
    assert torch.isfinite(ref).all(), "CPU reference itself is not finite"
    # sanity of the inputs: the empty span really is all padding
    for i in range(B):
        n = max(0, min(int(end[i]) - int(start[i]), S))
        assert int((tokens[i] != 0).sum()) == n

    fused = gpu.score_spans(lines.cuda(), start.cuda(), end.cuda()).cpu()
    assert torch.isfinite(fused).all()
    diff = (fused - ref).abs()
    bound = 0.08 if layers <= 2 else 0.1
    print(f"layers={layers} B={B}: max |fused - cpu| = {float(diff.max()):.5f}"
          f" (ref spread {float(ref.std()) if B > 1 else 0.0:.4f})")
    assert diff.max() < bound, (int(diff.argmax()), float(diff.max()))


def test_row_independence_and_determinism(model_pairs):
    gpu, _ = model_pairs[2]
    lines, start, end = _edge_batch(64, seed=5)
    lines, start, end = lines.cuda(), start.cuda(), end.cuda()
    batch = gpu.score_spans(lines, start, end)
    again = gpu.score_spans(lines, start, end)
    assert torch.equal(batch, again), "two runs of one batch differ"
    alone = torch.cat([
        gpu.score_spans(lines[i:i + 1], start[i:i + 1], end[i:i + 1])
        for i in range(64)
    ])
    bad = (alone != batch).nonzero().flatten().tolist()
    assert not bad, f"lines {bad} score differently alone than in the batch"


def test_fused_vs_layered_gpu_path():
    """Both paths use gelu_f32; bound 0.05 as in test_bert_fused_vs_layered."""
    from detectmateservice_amd import ops
    from detectmateservice_amd.utils.synthetic import AuditLogGenerator

    gpu, _ = _models(2, seed=77)
    gen = AuditLogGenerator(seed=123)
    raw = [gen.line()[0].encode() for _ in range(128)]
    lines, lens = ops.pack_lines(raw, MAX_LEN, device="cuda")
    start = torch.zeros(128, dtype=torch.int32, device="cuda")
    fused = gpu.score_spans(lines, start, lens.int())
    layered = gpu.forward(gpu.tokenize_spans(lines, start, lens.int()))
    diff = (fused - layered).abs().max().item()
    print(f"fused vs layered max diff {diff:.5f}")
    assert diff < 0.05, f"fused vs layered diff {diff}"


def test_fused_linear_gelu_range_and_extremes():
    """gelu_f32 through the layered GEMM epilogue, identity weights so each
    output is the GELU of exactly one input value."""
    from detectmateservice_amd import ops

    N = 128
    body = torch.linspace(-12.0, 12.0, 125 * N)
    special = torch.tensor(
        [0.0, -0.0, 1e-30, -1e-30, 1e-38, -1e-38, 1e-3, -1e-3,
         30.0, -30.0, 1e4, -1e4, 1e19, -1e19, 1e30, -1e30, 3e38, -3e38])
    pad = torch.zeros(3 * N - special.numel())
    x = torch.cat([body, special, pad]).view(128, N).bfloat16()
    wt = torch.eye(N).bfloat16()
    bias = torch.zeros(N)
    y = ops.fused_linear(x.cuda(), wt.cuda(), bias.cuda(),
                         activation="gelu").float().cpu()
    xf = x.float()
    ref = torch.nn.functional.gelu(xf, approximate="tanh")
    assert torch.isfinite(y).all(), "non-finite GELU output for finite input"

    # [-12, 12]: the existing 0.02 bound relative to the largest value ...
    yb, rb, xb = y[:125], ref[:125], xf[:125]
    err = (yb - rb).abs().max() / (rb.abs().max() + 1e-6)
    print(f"gelu [-12,12]: rel err {float(err):.2e}")
    assert err < 0.02, f"rel err {err}"
    # ... and element-wise: the output is a bf16 (relative spacing 2^-8)
    # of a value a few f32 ulp off; the f32 reference itself cancels
    # 0.5*x*(1 + tanh) to about 2^-24 * 0.5|x| < 4e-7 in the negative tail
    tol = rb.abs() * 2.0 ** -8 + 1e-5
    worst = ((yb - rb).abs() - tol).max()
    assert worst <= 0, f"element-wise GELU error exceeds bf16 rounding by {worst}"
    # sign and monotone tail behaviour
    assert (yb[xb > 0] > 0).all() and (yb[xb < -6] <= 0).all()

    # extremes: large positive gives x, large negative gives (-)0
    ys, xs = y[125:].flatten()[: special.numel()], xf[125:].flatten()[: special.numel()]
    big = xs >= 30
    assert torch.equal(ys[big], xs[big])
    assert (ys[xs <= -30] == 0).all()
    tiny = xs.abs() <= 1e-3
    assert ((ys[tiny] - 0.5 * xs[tiny]).abs() <= xs[tiny].abs() * 2.0 ** -7).all()


def _misaligned(t):
    """A contiguous view with the right numel that starts one element
    (4 bytes for f32) into a larger allocation."""
    big = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:] = t
    v = big[1:]
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def test_bindings_reject_misaligned_bias_blob(model_pairs):
    from detectmateservice_amd.ops import _dmx_C

    gpu, _ = model_pairs[2]
    wb, fb = gpu._fused_blobs()
    assert fb.data_ptr() % 16 == 0
    lines, start, end = _edge_batch(4, seed=3)
    lines, start, end = lines.cuda(), start.cuda(), end.cuda()
    bad = _misaligned(fb)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _dmx_C.bert_fused_bf16(lines, start, end, wb, bad, 2, 1e-5)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _dmx_C.bert_fused_probe(lines, start, end, wb, bad, 2, 1e-5, 31)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _dmx_C.bert_fused_timed(lines, start, end, wb, bad, 2, 1e-5)
    # the same values from an aligned blob are accepted
    ok = _dmx_C.bert_fused_bf16(lines, start, end, wb, fb.clone(), 2, 1e-5)
    assert torch.isfinite(ok).all()


def test_probe_and_timed_entry_points(model_pairs):
    from detectmateservice_amd.ops import _dmx_C

    gpu, _ = model_pairs[2]
    wb, fb = gpu._fused_blobs()
    lines, start, end = _edge_batch(4, seed=11)
    lines, start, end = lines.cuda(), start.cuda(), end.cuda()
    prod = _dmx_C.bert_fused_bf16(lines, start, end, wb, fb, 2, 1e-5)
    full = _dmx_C.bert_fused_probe(lines, start, end, wb, fb, 2, 1e-5, 31)
    assert torch.equal(full, prod), "probe mask 31 is not the production kernel"
    scores, stamps = _dmx_C.bert_fused_timed(lines, start, end, wb, fb, 2, 1e-5)
    assert torch.equal(scores, prod), "timed variant scores differ"
    st = stamps.cpu()
    assert st.shape[0] == 4 and (st[..., 19] >= st[..., 0]).all()
    assert (st[..., 0] > 0).all()
    # stamp slots: 2 layers record 3 + 2 * 8 + 1 = 20 stamps per wave, in
    # time order; the two unused slots are flushed as zero
    used = st[..., :20]
    assert (used[..., 1:] >= used[..., :-1]).all(), "stamp slots out of order"
    assert (st[..., 20:] == 0).all(), "unused stamp slots are not zero"
    # probe mask -> variant: every phase subset runs, and each mask reaches
    # its own kernel
    probe = {}
    for phases in (0, 1, 3, 7, 15, 16, 8, 31):
        out = _dmx_C.bert_fused_probe(lines, start, end, wb, fb, 2, 1e-5, phases)
        assert out.shape == (4,)
        probe[phases] = out
    # qkv and attention write only buf and vt, never x
    assert torch.equal(probe[1], probe[0]) and torch.equal(probe[3], probe[0])
    distinct = (0, 7, 15, 31, 16, 8)
    for i, a in enumerate(distinct):
        for b in distinct[i + 1:]:
            assert not torch.equal(probe[a], probe[b]), (a, b)
    # operand ablations (numerically wrong by design) still finish with
    # finite scores
    for phases in (31, 16):
        for abl in (1, 2, 3):
            out = _dmx_C.bert_fused_probe(lines, start, end, wb, fb, 2, 1e-5,
                                          phases | (abl << 8))
            assert torch.isfinite(out).all(), (phases, abl)
    torch.cuda.synchronize()
