"""The fused BERT kernel's embedding / distance head
(``dmx_bert_fused_embed_bf16``) and the detectors built on it (run on an
MI355X with `-m gpu`).

Weights are random-init and every bias and LayerNorm affine is randomised
too (the model initialises them to 0 / 1, which would hide a bias fetched
from the wrong column)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_LEN = 256
S = 64   # tokens per line of the fused geometry
H = 128  # hidden

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


def _model(layers, seed):
    from detectmateservice_amd.models.bert_tiny import (
        BertTinyConfig,
        BertTinyDetectorModel,
    )

    m = _randomize_affine(
        BertTinyDetectorModel(BertTinyConfig(layers=layers), device="cuda",
                              seed=seed), seed + 1)
    assert m._fused_ok()
    return m


def _edge_batch(B, seed):
    """[B, MAX_LEN] random bytes and B spans cycling through EDGE_SPANS."""
    g = torch.Generator().manual_seed(seed)
    lines = torch.randint(0, 256, (B, MAX_LEN), generator=g, dtype=torch.uint8)
    spans = [EDGE_SPANS[i % len(EDGE_SPANS)] for i in range(B)]
    start = torch.tensor([s for s, _ in spans], dtype=torch.int32)
    end = torch.tensor([e for _, e in spans], dtype=torch.int32)
    return lines.cuda(), start.cuda(), end.cuda()


@pytest.fixture(scope="module")
def models():
    return {layers: _model(layers, seed=60 + layers) for layers in (1, 2)}


def _stats(seed):
    """Random mu like an embedding, inv_var in [1e2, 1e3]."""
    g = torch.Generator().manual_seed(seed)
    mu = (torch.randn(H, generator=g) * 0.5).cuda()
    inv_var = (1e2 + 9e2 * torch.rand(H, generator=g)).cuda()
    return mu, inv_var


def _embed(model, lines, start, end, mu=None, inv_var=None, want_emb=True):
    from detectmateservice_amd.ops import _dmx_C

    wb, fb = model._fused_blobs()
    return _dmx_C.bert_fused_embed(lines, start, end, wb, fb,
                                   model.config.layers, 1e-5, mu, inv_var,
                                   want_emb)


# ---------------------------------------------------------------------------
# 1. the embedding is what the production kernel's score head pools
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("layers", [1, 2])
def test_head_consistency(models, layers, B):
    """emb @ w_score + b_score against score_spans of the production kernel.
    Both pool the same LDS contents; only the order of a 128-term f32 sum
    differs: |diff| <= 2*127*2^-24 * sum_i |emb_i w_i| + 2^-23 |score|."""
    m = models[layers]
    lines, start, end = _edge_batch(B, seed=11 * layers + B)
    score = m.score_spans(lines, start, end)
    emb = m.embed_spans(lines, start, end)
    assert emb.shape == (B, H) and emb.dtype == torch.float32
    assert torch.isfinite(emb).all()
    w = m.w_score.float()
    mine = (emb @ w + m.b_score).squeeze(-1)
    mag = (emb.abs() @ w.abs()).squeeze(-1)
    bound = 2 * 127 * 2.0 ** -24 * mag + 2.0 ** -23 * score.abs()
    diff = (mine - score).abs()
    print(f"layers={layers} B={B}: max diff {float(diff.max()):.3e}, "
          f"min bound {float(bound.min()):.3e}")
    assert (diff <= bound).all(), (diff - bound).max()


# ---------------------------------------------------------------------------
# 2. distance formula
# ---------------------------------------------------------------------------


def test_distance_formula(models):
    m = models[2]
    lines, start, end = _edge_batch(64, seed=21)
    mu, inv_var = _stats(22)
    emb, dist_a = _embed(m, lines, start, end, mu, inv_var, True)
    none, dist_b = _embed(m, lines, start, end, mu, inv_var, False)
    assert none is None and dist_a.shape == (64,)
    assert torch.equal(dist_b, dist_a)
    emb_only, no_dist = _embed(m, lines, start, end)
    assert no_dist is None and torch.equal(emb_only, emb)
    ref = ((emb - mu) ** 2 * inv_var).mean(dim=1).sqrt()
    rel = ((dist_a - ref).abs() / ref).max()
    print(f"distance: max rel err {float(rel):.3e}")
    torch.testing.assert_close(dist_a, ref, rtol=1e-4, atol=0.0)
    # the model-level call is the same launch
    d, e = m.embed_distance_spans(lines, start, end, mu, inv_var, return_emb=True)
    assert torch.equal(d, dist_a) and torch.equal(e, emb)
    assert torch.equal(m.embed_distance_spans(lines, start, end, mu, inv_var), dist_a)
    # B == 0 returns empty tensors without a launch
    e0, d0 = _embed(m, lines[:0], start[:0], end[:0], mu, inv_var)
    assert e0.shape == (0, H) and d0.shape == (0,)


# ---------------------------------------------------------------------------
# 3. row independence and determinism
# ---------------------------------------------------------------------------


def test_row_independence_and_determinism(models):
    m = models[2]
    lines, start, end = _edge_batch(64, seed=31)
    mu, inv_var = _stats(32)
    emb, dist = _embed(m, lines, start, end, mu, inv_var)
    emb2, dist2 = _embed(m, lines, start, end, mu, inv_var)
    assert torch.equal(emb, emb2) and torch.equal(dist, dist2)
    alone = [_embed(m, lines[i:i + 1], start[i:i + 1], end[i:i + 1], mu, inv_var)
             for i in range(64)]
    assert torch.equal(torch.cat([a[0] for a in alone]), emb)
    assert torch.equal(torch.cat([a[1] for a in alone]), dist)


# ---------------------------------------------------------------------------
# 4. accuracy against a true fp32 reference
# ---------------------------------------------------------------------------


def _reference_f32(model, tokens):
    """Plain-torch f32 forward: weights upcast, no intermediate bf16
    rounding, tanh-form GELU as gelu_f32, mean-pool. [B, H] f32."""
    F = torch.nn.functional
    c = model.config
    B = tokens.shape[0]
    x = model.tok_emb.float()[tokens.long()] + model.pos_emb.float()[:S]
    for layer in model.layers:
        qkv = x @ layer["wqkv_t"].float().T + layer["bqkv"]
        q, k, v = (t.view(B, S, c.heads, c.head_dim).transpose(1, 2)
                   for t in qkv.split(c.hidden, dim=-1))
        p = torch.softmax(q @ k.transpose(-1, -2) / c.head_dim ** 0.5, dim=-1)
        attn = (p @ v).transpose(1, 2).reshape(B, S, c.hidden)
        proj = attn @ layer["wo_t"].float().T + layer["bo"]
        x1 = F.layer_norm(x + proj, (c.hidden,), layer["ln1_g"].float(),
                          layer["ln1_b"].float(), 1e-5)
        ffn = F.gelu(x1 @ layer["w1_t"].float().T + layer["b1"],
                     approximate="tanh")
        ffn = ffn @ layer["w2_t"].float().T + layer["b2"]
        x = F.layer_norm(x1 + ffn, (c.hidden,), layer["ln2_g"].float(),
                         layer["ln2_b"].float(), 1e-5)
    return x.mean(dim=1)


def test_accuracy_against_f32_reference(models):
    """E_fused <= 2 * E_layered, the layered GPU path being the yardstick:
    the fused kernel has one rounding point per layer that the layered path
    lacks (the FFN accumulates into bf16 x in two halves).
    Measured on an MI355X: E_fused 1.092e-2, E_layered 1.042e-2 (embedding
    magnitude up to 2.84)."""
    from detectmateservice_amd import ops
    from detectmateservice_amd.utils.synthetic import AuditLogGenerator

    m = models[2]
    gen = AuditLogGenerator(seed=123)
    raw = [gen.line()[0].encode() for _ in range(128)] + [b""]
    lines, lens = ops.pack_lines(raw, MAX_LEN, device="cuda")
    start = torch.zeros(len(raw), dtype=torch.int32, device="cuda")
    end = lens.int()
    tokens = m.tokenize_spans(lines, start, end)
    # a CPU copy of the same model for the reference: f32 matmuls on the host
    cpu = type(m)(m.config, device="cpu")
    cpu.load_state_dict(m.state_dict())
    ref = _reference_f32(cpu, tokens.cpu())
    fused = m.embed_spans(lines, start, end).cpu()
    layered = m._encode(tokens).float().mean(dim=1).cpu()
    assert torch.isfinite(fused).all()
    e_fused = float((fused[:128] - ref[:128]).abs().max())
    e_layered = float((layered[:128] - ref[:128]).abs().max())
    print(f"E_fused {e_fused:.3e}  E_layered {e_layered:.3e}  "
          f"(embedding max |x| {float(ref.abs().max()):.3f})")
    assert e_fused <= 2 * e_layered
    # a stuck column would pass a max-norm test: the all-padding row (the
    # last one) must differ from a full row, in most columns
    full = int(lens[:128].argmax())
    assert int(lens[full]) >= S
    assert int((fused[128] != fused[full]).sum()) > H // 2


# ---------------------------------------------------------------------------
# 5. EmbeddingDetector(embed_path="fused")
# ---------------------------------------------------------------------------

ODD = [b"\x01\x02!!!" + b"Z" * 180, b""]


def _scenario():
    from detectmateservice_amd.utils.synthetic import AuditLogGenerator

    gen = AuditLogGenerator(seed=61)
    train = [gen.line()[0].encode() for _ in range(256)]
    return train, [gen.line()[0].encode() for _ in range(32)] + ODD


def test_embedding_detector_fused_path():
    from detectmateservice_amd.library.detectors import EmbeddingDetector
    from detectmateservice_amd.schemas import DetectorSchema, ParserSchema

    train, test = _scenario()

    def frames(raw, tag):
        return [ParserSchema(logID=f"{tag}{i}", log=l.decode("latin-1"),
                             EventID=1).serialize() for i, l in enumerate(raw)]

    cfg = {"data_use_training": 256, "z_threshold": 4.0, "device": "cuda",
           "embed_path": "fused"}
    det = EmbeddingDetector(cfg)
    assert det.model._fused_ok()
    assert all(o is None for o in det.process_batch(frames(train, "t")))
    assert det._n == 256 and det.stats.sum.is_cuda
    out = det.process_batch(frames(test, "x"))
    dist = det.model.embed_distance_spans(
        *det._pack(test), det.stats.mu, det.stats.inv_var)
    print("normal max", float(dist[:32].max()), "odd", dist[32:].tolist())
    assert [o is not None for o in out] == [False] * 32 + [True, True]
    for o, d, lid in zip(out[32:], dist[32:].tolist(), ("x32", "x33")):
        a = DetectorSchema.deserialize(o)
        assert a.logIDs == [lid] and a.alertID == f"emb-{lid}"
        assert a.score == pytest.approx(d, rel=1e-6)
        assert a.description == f"Embedding distance {d:.3f} > 4.000"
    det2 = EmbeddingDetector(cfg)
    det2.load_state_dict(det.state_dict())
    dist2 = det2.model.embed_distance_spans(
        *det2._pack(test), det2.stats.mu, det2.stats.inv_var)
    assert torch.equal(dist2, dist)
    out2 = det2.process_batch(frames(test, "x"))
    assert [o is not None for o in out2] == [o is not None for o in out]


# ---------------------------------------------------------------------------
# 6. pipeline graph replay
# ---------------------------------------------------------------------------


def test_pipeline_embedding_graph_replay():
    from detectmateservice_amd import ops
    from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig
    from detectmateservice_amd.utils.synthetic import AUDIT_TEMPLATES

    train, test = _scenario()
    # no log_format: the content span is the whole line
    cfg = PipelineConfig(templates=AUDIT_TEMPLATES, train_lines=256,
                         score_mode="embedding", score_threshold=4.0)
    pipe = GpuPipeline(cfg, device="cuda")
    out = pipe.process_lines(train)
    assert not out["scores"].any() and pipe.embedding_stats.n == 256
    batch = (test + train)[:64]
    lines, lens = ops.pack_lines(batch, cfg.max_len, device="cuda")
    eager = pipe.process_packed(lines.clone(), lens.clone())
    eager_scores = eager["scores"].clone().cpu()
    eager_anom = eager["anomaly"].clone().cpu()
    assert eager_anom.tolist() == [False] * 32 + [True, True] + [False] * 30

    assert pipe.enable_graph(64)
    out = pipe.process_packed_graph(lines, lens)
    torch.cuda.synchronize()
    assert torch.allclose(out["scores"].cpu(), eager_scores, atol=1e-4)
    assert torch.equal(out["anomaly"].cpu(), eager_anom)
    part = pipe.process_packed_graph_partial(lines[:40], lens[:40])
    torch.cuda.synchronize()
    assert part["scores"].shape == (40,) and part["anomaly"].shape == (40,)
    assert torch.allclose(part["scores"].cpu(), eager_scores[:40], atol=1e-4)
    assert pipe.embedding_stats.n == 256
