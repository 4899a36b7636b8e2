"""The embedding / distance head without a GPU: the launch contract of
``_dmx_C.bert_fused_embed``, the model's layered fallback, ``EmbeddingStats``
against an f64 numpy computation, and ``score_mode="embedding"`` through
``GpuPipeline`` and ``FusedPipelineDetector`` on the CPU path."""
import contextlib
import re

import numpy as np
import pytest
import torch

from detectmateservice_amd import ops
from detectmateservice_amd.library.detectors import (
    EmbeddingDetector,
    FusedPipelineDetector,
)
from detectmateservice_amd.models.bert_tiny import (
    BertTinyConfig,
    BertTinyDetectorModel,
    EmbeddingStats,
)
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig
from detectmateservice_amd.schemas import DetectorSchema, LogSchema, ParserSchema
from detectmateservice_amd.utils.synthetic import AuditLogGenerator

if ops.have_extension():
    from detectmateservice_amd.ops import _dmx_C

H = 128  # hidden size of the fused geometry

# ---------------------------------------------------------------------------
# 1. contract rejections: one violated clause per call, otherwise well-formed
# CPU tensors. Never run where a GPU exists, so a missing check can fail a
# test but cannot reach a device.
# ---------------------------------------------------------------------------

contract = [
    pytest.mark.skipif(not ops.have_extension(),
                       reason="HIP extension _dmx_C not built"),
    pytest.mark.skipif(
        torch.cuda.is_available(),
        reason="malformed arguments are only ever passed where no GPU exists"),
]

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


def _i32(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def _noncontig(t):
    """Same shape and dtype as t, but a strided view."""
    big = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype)
    v = big[..., ::2]
    assert v.shape == t.shape and not v.is_contiguous()
    return v


def _embed_args(n_layers=2):
    lay = _dmx_C.bert_fused_layout(n_layers)
    return dict(
        lines=torch.zeros((B, 64), dtype=torch.uint8), start=_i32(B),
        end=_i32(B), wb=torch.zeros(lay["wb_elems"], dtype=torch.bfloat16),
        fb=torch.zeros(lay["fb_elems"], dtype=torch.float32),
        n_layers=n_layers, eps=1e-5, mu=None, inv_var=None, want_emb=True,
    )


def _embed_cases():
    """(violation id, argument the message must name, kwargs overrides)."""
    a = _embed_args()
    stat = torch.ones(H)
    with_stats = {"mu": stat, "inv_var": stat.clone()}
    return [
        # every shared fused-argument case
        ("device", "lines", {}),
        ("lines-dtype", "lines", {"lines": a["lines"].int()}),
        ("lines-noncontig", "lines", {"lines": _noncontig(a["lines"])}),
        ("start-len", "start", {"start": _i32(B + 1)}),
        ("end-len", "end", {"end": _i32(B - 1)}),
        ("start-dtype", "start", {"start": torch.zeros(B, dtype=torch.int64)}),
        ("wb-short", "wb", {"wb": a["wb"][:-1]}),
        ("wb-dtype", "wb", {"wb": a["wb"].float()}),
        ("fb-short", "fb", {"fb": a["fb"][:-1]}),
        ("layers-0", "n_layers", {"n_layers": 0}),
        ("layers-3", "wb", {"n_layers": 3}),
        # the statistics vectors
        ("device-stats", "lines", with_stats),
        ("device-dist-only", "lines", {**with_stats, "want_emb": False}),
        ("mu-dtype", "mu", {**with_stats, "mu": stat.double()}),
        ("mu-len", "mu", {**with_stats, "mu": torch.ones(H - 1)}),
        ("mu-2d", "mu", {**with_stats, "mu": torch.ones(1, H)}),
        ("mu-noncontig", "mu", {**with_stats, "mu": _noncontig(stat)}),
        ("inv_var-dtype", "inv_var", {**with_stats, "inv_var": stat.bfloat16()}),
        ("inv_var-len", "inv_var", {**with_stats, "inv_var": torch.ones(2 * H)}),
        ("mu-alone", "mu", {"mu": stat}),
        ("inv_var-alone", "inv_var", {"inv_var": stat}),
        ("no-output", "want_emb", {"want_emb": False}),
    ]


DEVICE_CASES = ("device", "device-stats", "device-dist-only")


@pytest.mark.parametrize(
    "case", [pytest.param(c, marks=contract) for c in _embed_cases()]
    if ops.have_extension() else [], ids=lambda c: c[0])
def test_bert_fused_embed_rejects(case):
    cid, named, overrides = case
    with _rejected(named, device_clause=cid in DEVICE_CASES):
        _dmx_C.bert_fused_embed(**{**_embed_args(), **overrides})


@pytest.mark.skipif(not ops.have_extension(), reason="extension not built")
def test_bert_fused_embed_signature():
    """Positional form of the issue's signature, defaults included."""
    doc = _dmx_C.bert_fused_embed.__doc__
    for piece in ("mu: ", "inv_var: ", "want_emb: bool = True"):
        assert piece in doc, doc


# ---------------------------------------------------------------------------
# shared scenario: 256 training lines, then 32 normal lines and two odd ones
# ---------------------------------------------------------------------------

ODD = [b"\x01\x02!!!" + b"Z" * 180, b""]
THRESHOLD = 4.0


def _scenario():
    gen = AuditLogGenerator(seed=61)
    train = [gen.line()[0].encode() for _ in range(256)]
    normal = [gen.line()[0].encode() for _ in range(32)]
    return train, normal + ODD


@pytest.fixture(scope="module")
def scenario():
    return _scenario()


@pytest.fixture(scope="module")
def cpu_embeddings(scenario):
    """[256, H] f32 embeddings of the training lines, computed once."""
    det = EmbeddingDetector({"device": "cpu"})
    return det.embed(scenario[0])


# ---------------------------------------------------------------------------
# 2. fallback exactness
# ---------------------------------------------------------------------------


def test_embed_spans_fallback_is_detector_embed(scenario, cpu_embeddings):
    det = EmbeddingDetector({"device": "cpu"})
    raw = scenario[0][:48] + ODD
    lines, lens = ops.pack_lines(raw, det.config.batch_max_len, device="cpu")
    start = torch.zeros(len(raw), dtype=torch.int32)
    emb = det.model.embed_spans(lines, start, lens.int())
    assert emb.dtype == torch.float32 and emb.shape == (len(raw), H)
    assert torch.equal(emb, det.embed(raw))
    assert torch.equal(emb[:48], cpu_embeddings[:48])  # batch-independent
    # distance fallback: the formula, in torch, and the same embedding
    mu, inv_var = torch.randn(H), torch.rand(H) + 0.5
    dist, emb2 = det.model.embed_distance_spans(
        lines, start, lens.int(), mu, inv_var, return_emb=True)
    assert torch.equal(emb2, emb)
    assert torch.equal(dist, ((emb - mu) ** 2 * inv_var).mean(dim=1).sqrt())
    assert torch.equal(
        det.model.embed_distance_spans(lines, start, lens.int(), mu, inv_var),
        dist)
    # empty batch
    e0 = det.model.embed_spans(lines[:0], start[:0], lens[:0].int())
    assert e0.shape == (0, H)


def test_forward_shares_the_encoder():
    m = BertTinyDetectorModel(BertTinyConfig(), device="cpu", seed=5)
    g = torch.Generator().manual_seed(9)
    m.b_score = torch.randn(1, generator=g)
    tokens = torch.randint(0, 259, (5, 64), generator=g)
    tokens[3, 20:] = 0
    tokens[4] = 0
    x = m._encode(tokens)
    assert x.shape == (5, 64, H) and x.dtype == m.dtype
    pooled = x.float().mean(dim=1)
    expect = (pooled @ m.w_score.float() + m.b_score).squeeze(-1)
    assert torch.equal(m.forward(tokens), expect)


# ---------------------------------------------------------------------------
# 3. EmbeddingStats against f64 numpy
# ---------------------------------------------------------------------------


def _numpy_stats(emb):
    e = emb.numpy().astype(np.float64)
    mu = e.sum(axis=0) / e.shape[0]
    var = np.maximum((e * e).sum(axis=0) / e.shape[0] - mu * mu, 1e-6)
    return mu, 1.0 / var


def test_embedding_stats_match_numpy(cpu_embeddings):
    st = EmbeddingStats(H)
    assert st.sum.dtype == torch.float64 and st.sumsq.dtype == torch.float64
    for chunk in (cpu_embeddings[:7], cpu_embeddings[7:200], cpu_embeddings[200:]):
        st.update(chunk)
    assert st.n == 256
    mu, inv_var = _numpy_stats(cpu_embeddings)
    assert st.mu.dtype == torch.float32 and st.inv_var.dtype == torch.float32
    np.testing.assert_allclose(st.mu.numpy(), mu, rtol=1e-6)
    np.testing.assert_allclose(st.inv_var.numpy(), inv_var, rtol=1e-6)
    # cached until the next update, which invalidates both
    assert st.mu is st.mu and st.inv_var is st.inv_var
    before = st.mu.clone()
    st.update(cpu_embeddings[:1] + 1.0)
    assert st.n == 257 and not torch.equal(st.mu, before)
    # the variance floor: a constant column has inv_var 1 / 1e-6
    flat = EmbeddingStats(4)
    flat.update(torch.full((5, 4), 0.25))
    np.testing.assert_allclose(flat.inv_var.numpy(), 1e6, rtol=1e-6)


def test_embedding_stats_checkpoints(cpu_embeddings):
    st = EmbeddingStats(H)
    st.update(cpu_embeddings)
    state = st.state_dict()
    assert set(state) == {"sum", "sumsq", "n"}
    assert state["sum"].dtype == torch.float64 and state["sum"].device.type == "cpu"
    assert state["sumsq"].dtype == torch.float64 and isinstance(state["n"], int)
    st2 = EmbeddingStats(H)
    _ = st2.mu  # a cached value from before the restore must not survive
    st2.load_state_dict(state)
    assert st2.n == 256
    assert torch.equal(st2.mu, st.mu) and torch.equal(st2.inv_var, st.inv_var)

    # EmbeddingDetector checkpoint -> EmbeddingStats
    det = EmbeddingDetector({"device": "cpu"})
    det.stats.update(cpu_embeddings)
    ckpt = det.state_dict()
    assert {"seen_lines", "sum", "sumsq", "n", "model"} <= set(ckpt)
    assert ckpt["sum"].dtype == torch.float64 and ckpt["sum"].device.type == "cpu"
    st3 = EmbeddingStats(H)
    st3.load_state_dict(ckpt)
    assert torch.equal(st3.sum, st.sum) and torch.equal(st3.sumsq, st.sumsq)
    assert torch.equal(st3.mu, st.mu)
    # EmbeddingStats -> EmbeddingDetector checkpoint, in both embed paths
    for path in ("layered", "fused"):
        det2 = EmbeddingDetector({"device": "cpu", "embed_path": path})
        det2.load_state_dict({**ckpt, **st.state_dict()})
        assert det2._n == 256 and torch.equal(det2._sum, st.sum)
        assert torch.equal(det2._sumsq, st.sumsq)
    # a checkpoint as the code before EmbeddingStats wrote it
    old = {"seen_lines": 256, "sum": cpu_embeddings.double().sum(dim=0),
           "sumsq": (cpu_embeddings.double() ** 2).sum(dim=0), "n": 256,
           "model": det.model.state_dict()}
    det3 = EmbeddingDetector({"device": "cpu", "embed_path": "fused"})
    det3.load_state_dict(old)
    assert torch.equal(det3.stats.mu, st.mu)


# ---------------------------------------------------------------------------
# 4. score_mode="embedding" on the CPU path
# ---------------------------------------------------------------------------


def _pipe(train_lines=256):
    return GpuPipeline(
        PipelineConfig(train_lines=train_lines, score_mode="embedding",
                       score_threshold=THRESHOLD), device="cpu")


def _check_scores(scores, anomaly):
    """32 normal rows, then the two odd ones."""
    print("normal max", float(scores[:32].max()), "odd", scores[32:].tolist())
    assert anomaly.tolist() == [False] * 32 + [True, True]
    assert scores[:32].max() < THRESHOLD < scores[32:].min()
    assert (scores[:32] > 0).all()


def test_pipeline_embedding_mode_cpu(scenario):
    train, test = scenario
    pipe = _pipe()
    out = pipe.process_lines(train)
    assert torch.equal(out["scores"], torch.zeros(256))
    assert not out["anomaly"].any()
    assert pipe.embedding_stats.n == 256
    out = pipe.process_lines(test)
    _check_scores(out["scores"], out["anomaly"])
    assert pipe.embedding_stats.n == 256  # detect rows do not train
    # the default mode is untouched by the new field
    head = GpuPipeline(PipelineConfig(train_lines=256), device="cpu")
    assert head.embedding_stats is None and head.config.score_mode == "head"
    with pytest.raises(ValueError, match="score_mode"):
        GpuPipeline(PipelineConfig(score_mode="distance"), device="cpu")


def test_pipeline_embedding_mode_straddling_batch(scenario):
    train, test = scenario
    ref = _pipe()
    ref.process_lines(train)
    expect = ref.process_lines(test)["scores"]
    # 300 lines over the 256-line boundary: head rows train, the tail scores
    pipe = _pipe()
    batch = train + test + train[:10]
    assert len(batch) == 300
    out = pipe.process_lines(batch)
    assert torch.equal(out["scores"][:256], torch.zeros(256))
    assert not out["anomaly"][:256].any()
    assert pipe.embedding_stats.n == 256
    assert torch.equal(pipe.embedding_stats.sum, ref.embedding_stats.sum)
    assert torch.equal(out["scores"][256:290], expect)
    assert (out["scores"][290:] > 0).all()
    assert out["anomaly"][256:].tolist() == [False] * 32 + [True, True] + [False] * 10


def _log_frames(raw, tag):
    return [LogSchema(logID=f"{tag}{i}", log=l.decode("latin-1")).serialize()
            for i, l in enumerate(raw)]


def test_fused_pipeline_detector_embedding_mode(scenario):
    train, test = scenario
    # the odd line's control bytes survive the schema as latin-1 text of
    # code points < 128, so the detector sees the same bytes as the pipeline
    assert all(l.decode("latin-1").encode() == l for l in test)
    cfg = {"score_mode": "embedding", "score_threshold": THRESHOLD,
           "data_use_training": 256, "device": "cpu"}
    det = FusedPipelineDetector(cfg)
    assert all(o is None for o in det.process_batch(_log_frames(train, "t")))
    state = det.state_dict()
    assert set(state["embedding_stats"]) == {"sum", "sumsq", "n"}
    assert state["embedding_stats"]["n"] == 256
    out = det.process_batch(_log_frames(test, "x"))
    assert [o is not None for o in out] == [False] * 32 + [True, True]
    alerts = [DetectorSchema.deserialize(o) for o in out[32:]]
    for a, lid in zip(alerts, ("x32", "x33")):
        assert a.logIDs == [lid] and a.score > THRESHOLD
        assert re.fullmatch(r"Anomaly: embedding distance \d+\.\d{3}",
                            a.description), a.description
    # restore into a fresh detector: the same alerts with the same scores
    det2 = FusedPipelineDetector(cfg)
    det2.load_state_dict(state)
    out2 = det2.process_batch(_log_frames(test, "x"))
    assert [o is not None for o in out2] == [o is not None for o in out]
    for a, o in zip(alerts, out2[32:]):
        b = DetectorSchema.deserialize(o)
        assert (b.score, b.description, b.logIDs) == (a.score, a.description, a.logIDs)
    # the head mode keeps its wording and carries no embedding_stats
    head = FusedPipelineDetector({"device": "cpu"})
    assert "embedding_stats" not in head.state_dict()


def test_embedding_detector_fused_path_falls_back_on_cpu(scenario):
    """embed_path="fused" where the fused kernel does not apply: the model's
    layered fallback, same alerts as the layered path."""
    train, test = scenario

    def frames(raw, tag):
        return [ParserSchema(logID=f"{tag}{i}", log=l.decode("latin-1"),
                             EventID=1).serialize() for i, l in enumerate(raw)]

    outs = {}
    for path in ("layered", "fused"):
        det = EmbeddingDetector({"data_use_training": 256, "device": "cpu",
                                 "z_threshold": THRESHOLD, "embed_path": path})
        assert all(o is None for o in det.process_batch(frames(train, "t")))
        assert det._n == 256
        outs[path] = det.process_batch(frames(test, "x"))
        assert [o is not None for o in outs[path]] == [False] * 32 + [True, True]
    for a, b in zip(outs["layered"][32:], outs["fused"][32:]):
        a, b = DetectorSchema.deserialize(a), DetectorSchema.deserialize(b)
        assert a.alertID == b.alertID and a.logIDs == b.logIDs
        assert b.description.startswith("Embedding distance ")
        # f32 moments (layered) against f64 moments cast once (fused)
        assert a.score == pytest.approx(b.score, rel=1e-3)
    with pytest.raises(ValueError, match="embed_path"):
        EmbeddingDetector({"device": "cpu", "embed_path": "kernel"})


# ---------------------------------------------------------------------------
# 5. nothing fitted: no distance
# ---------------------------------------------------------------------------


def test_no_training_scores_zero(scenario):
    _, test = scenario
    pipe = _pipe(train_lines=0)
    out = pipe.process_lines(test)
    assert torch.equal(out["scores"], torch.zeros(len(test)))
    assert not out["anomaly"].any()
    det = FusedPipelineDetector({"score_mode": "embedding", "device": "cpu",
                                 "score_threshold": THRESHOLD})
    assert all(o is None for o in det.process_batch(_log_frames(test, "x")))

    def frame(l, i):
        return ParserSchema(logID=str(i), log=l.decode("latin-1"),
                            EventID=1).serialize()

    emb = EmbeddingDetector({"data_use_training": 0, "device": "cpu",
                             "embed_path": "fused"})
    assert all(o is None for o in emb.process_batch(
        [frame(l, i) for i, l in enumerate(test)]))
