"""GPU kernel numerics tests: every HIP kernel vs a plain PyTorch fp32
reference of the same op (run on an MI355X with `-m gpu`)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from detectmateservice_amd import ops

    # On a GPU box the HIP extension MUST be present (no silent fallback).
    assert ops.have_extension(), "HIP extension _dmx_C not built/loadable"
    yield


def test_mfma_layout_probe():
    """Verify the assumed mfma_f32_16x16x32_bf16 fragment layout (guide §3:
    layout tables unavailable offline — empirically pinned here).
    Asymmetric operands so transposes cannot pass (guide §5.4 rule 16)."""
    from detectmateservice_amd.ops import _dmx_C

    torch.manual_seed(0)
    A = (torch.randn(16, 32) * 0.5).bfloat16().cuda()
    B = (torch.arange(32 * 16).reshape(32, 16).float() * 0.01 +
         torch.randn(32, 16)).bfloat16().cuda()
    ref = (A.float() @ B.float()).cpu()

    results = {}
    for a_l in (0, 1):
        for b_l in (0, 1):
            D = _dmx_C.probe_mfma(A, B, a_l, b_l).cpu()
            results[(a_l, b_l)] = float((D - ref).abs().max())
    best = min(results, key=results.get)
    assert results[best] < 0.15, f"no layout matches: {results}"
    assert best == (0, 0), (
        f"kernel assumes contiguous-octet layout (0,0) but hardware wants "
        f"{best}; errors: {results} — fix read_frag in gemm_bf16.hip"
    )


@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (256, 384, 128),
                                   (512, 128, 512), (200, 112, 128)])
def test_fused_linear_vs_torch(M, N, K):
    from detectmateservice_amd import ops

    torch.manual_seed(1)
    x = (torch.randn(M, K) * 0.5).bfloat16().cuda()
    wt = (torch.randn(N, K) * 0.5).bfloat16().cuda()
    bias = torch.randn(N).cuda()
    y = ops.fused_linear(x, wt, bias, activation="none").float().cpu()
    ref = torch.nn.functional.linear(x.float().cpu(), wt.float().cpu(), bias.cpu())
    err = (y - ref).abs().max() / (ref.abs().max() + 1e-6)
    assert err < 0.02, f"rel err {err}"


def test_fused_linear_gelu():
    from detectmateservice_amd import ops

    torch.manual_seed(2)
    x = (torch.randn(256, 128) * 0.5).bfloat16().cuda()
    wt = (torch.randn(512, 128) * 0.5).bfloat16().cuda()
    bias = torch.randn(512).cuda()
    y = ops.fused_linear(x, wt, bias, activation="gelu").float().cpu()
    ref = torch.nn.functional.gelu(
        torch.nn.functional.linear(x.float().cpu(), wt.float().cpu(), bias.cpu()),
        approximate="tanh",
    )
    err = (y - ref).abs().max() / (ref.abs().max() + 1e-6)
    assert err < 0.02, f"rel err {err}"


def test_layernorm_vs_torch():
    from detectmateservice_amd import ops

    torch.manual_seed(3)
    for D in (128, 512):
        x = torch.randn(333, D).bfloat16().cuda()
        r = torch.randn(333, D).bfloat16().cuda()
        g = torch.randn(D).bfloat16().cuda()
        b = torch.randn(D).bfloat16().cuda()
        y, xres = ops.layernorm(x, g, b, residual=r, return_xres=True)
        ref = torch.nn.functional.layer_norm(
            x.float().cpu() + r.float().cpu(), (D,), g.float().cpu(), b.float().cpu()
        )
        assert (y.float().cpu() - ref).abs().max() < 0.05
        assert (xres.float().cpu() - (x.float().cpu() + r.float().cpu())).abs().max() < 0.02


@pytest.mark.parametrize("S", [64, 48, 128])
def test_attention_vs_torch(S):
    from detectmateservice_amd import ops

    torch.manual_seed(4)
    BH, Dh = 12, 64
    q = (torch.randn(BH, S, Dh) * 0.5).bfloat16().cuda()
    k = (torch.randn(BH, S, Dh) * 0.5).bfloat16().cuda()
    v = (torch.randn(BH, S, Dh) * 0.5).bfloat16().cuda()
    o = ops.attention(q, k, v).float().cpu()
    scale = 1.0 / Dh ** 0.5
    s = torch.softmax(q.float().cpu() @ k.float().cpu().transpose(-1, -2) * scale, -1)
    ref = s @ v.float().cpu()
    assert (o - ref).abs().max() < 0.03


def test_template_match_gpu_vs_cpu():
    from detectmateservice_amd import ops
    from detectmateservice_amd.utils.synthetic import (
        AUDIT_LOG_FORMAT,
        AUDIT_TEMPLATES,
        AuditLogGenerator,
    )

    gen = AuditLogGenerator(seed=17, anomaly_rate=0.1)
    raw = [gen.line()[0].encode() for _ in range(512)]
    cpu_m = ops.TemplateMatcher(AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT, device="cpu")
    gpu_m = ops.TemplateMatcher(AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT, device="cuda")
    lines_c, lens_c = ops.pack_lines(raw, 512, device="cpu")
    lines_g, lens_g = lines_c.cuda(), lens_c.cuda()
    mc = cpu_m.match_packed(lines_c, lens_c)
    mg = {k: v.cpu() for k, v in gpu_m.match_packed(lines_g, lens_g).items()}
    assert torch.equal(mc["event_id"], mg["event_id"])
    assert torch.equal(mc["n_caps"], mg["n_caps"])
    assert torch.equal(mc["n_fmt_caps"], mg["n_fmt_caps"])
    # compare capture spans for matched lines
    for i in range(len(raw)):
        nc = int(mc["n_caps"][i])
        assert torch.equal(mc["caps"][i, :nc], mg["caps"][i, :nc]), raw[i]
        nf = int(mc["n_fmt_caps"][i])
        assert torch.equal(mc["fmt_caps"][i, :nf], mg["fmt_caps"][i, :nf]), raw[i]


def test_watch_hashes_and_hashsets_gpu_vs_cpu():
    from detectmateservice_amd import ops
    from detectmateservice_amd.utils.synthetic import (
        AUDIT_LOG_FORMAT,
        AUDIT_TEMPLATES,
        AuditLogGenerator,
    )

    gen = AuditLogGenerator(seed=23, anomaly_rate=0.2)
    raw = [gen.line()[0].encode() for _ in range(256)]
    lines_c, lens_c = ops.pack_lines(raw, 512)
    cpu_m = ops.TemplateMatcher(AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT, device="cpu")
    gpu_m = ops.TemplateMatcher(AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT, device="cuda")
    mc = cpu_m.match_packed(lines_c, lens_c)
    lines_g = lines_c.cuda()
    mg = gpu_m.match_packed(lines_g, lens_c.cuda())

    specs_c = torch.tensor([[0, 1, 5, 0], [0, -1, 0, 0]], dtype=torch.int32)
    hc = ops.watch_hashes(lines_c, mc, specs_c)
    hg = ops.watch_hashes(lines_g, mg, specs_c.cuda()).cpu()
    assert torch.equal(hc, hg)

    # insert first half, probe second half; CPU and GPU sets must agree
    cpu_s = ops.GpuHashSets(2, 1 << 12, device="cpu")
    gpu_s = ops.GpuHashSets(2, 1 << 12, device="cuda")
    cpu_s.insert(hc[:128])
    gpu_s.insert(hg[:128].cuda())
    pc = cpu_s.probe(hc[128:])
    pg = gpu_s.probe(hg[128:].cuda()).cpu()
    assert torch.equal(pc, pg)


def test_bert_tiny_gpu_vs_cpu():
    """Full model forward: GPU kernels vs CPU fp32 reference path."""
    from detectmateservice_amd.models.bert_tiny import (
        BertTinyConfig,
        BertTinyDetectorModel,
    )

    cfg = BertTinyConfig()
    cpu_model = BertTinyDetectorModel(cfg, device="cpu", seed=7)
    gpu_model = BertTinyDetectorModel(cfg, device="cuda", seed=7)
    tokens = torch.randint(0, 259, (64, 64))
    sc = cpu_model(tokens)
    sg = gpu_model(tokens.cuda()).cpu()
    assert (sc - sg).abs().max() < 0.05, (sc - sg).abs().max()


def test_pipeline_gpu_end_to_end():
    from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig
    from detectmateservice_amd.utils.synthetic import (
        AUDIT_LOG_FORMAT,
        AUDIT_TEMPLATES,
        AuditLogGenerator,
    )

    cfg = PipelineConfig(
        templates=AUDIT_TEMPLATES,
        log_format=AUDIT_LOG_FORMAT,
        watches=[{"kind": "variable", "pos": 5, "event": 1}],
        train_lines=256,
        use_transformer=True,
        score_threshold=1e9,
    )
    pipe = GpuPipeline(cfg, device="cuda")
    gen = AuditLogGenerator(seed=5)
    train = [gen.line()[0].encode() for _ in range(256)]
    pipe.process_lines(train)
    normal = [gen.line()[0].encode() for _ in range(64)]
    out = pipe.process_lines(normal)
    assert int(out["anomaly"].sum()) == 0
    bad = (
        "type=USER_ACCT msg=audit(1642723741.072:999): pid=1 uid=0 auid=1 ses=1 "
        "msg='op=PAM:accounting acct=\"intruder\" exe=/usr/sbin/cron hostname=? "
        "addr=? terminal=cron res=success'"
    ).encode()
    out = pipe.process_lines(normal[:3] + [bad])
    assert out["anomaly"].cpu().tolist() == [False, False, False, True]


def test_attention_qkv_mfma_vs_reference():
    """MFMA fused-QKV attention vs the permute+torch reference path."""
    from detectmateservice_amd import ops

    torch.manual_seed(5)
    B, S, H, Dh = 32, 64, 2, 64
    qkv = (torch.randn(B, S, 3 * H * Dh) * 0.5).bfloat16().cuda()
    o = ops.attention_qkv(qkv, S, H, Dh).float().cpu()
    # reference on CPU fp32
    q, k, v = qkv.float().cpu().view(B, S, 3, H, Dh).unbind(dim=2)
    q = q.permute(0, 2, 1, 3)
    k = k.permute(0, 2, 1, 3)
    v = v.permute(0, 2, 1, 3)
    s = torch.softmax(q @ k.transpose(-1, -2) / Dh ** 0.5, -1)
    ref = (s @ v).permute(0, 2, 1, 3).reshape(B, S, H * Dh)
    assert (o - ref).abs().max() < 0.03, (o - ref).abs().max()


def test_attention_qkv_mfma_s32():
    from detectmateservice_amd import ops

    torch.manual_seed(6)
    B, S, H, Dh = 16, 32, 4, 32
    qkv = (torch.randn(B, S, 3 * H * Dh) * 0.5).bfloat16().cuda()
    o = ops.attention_qkv(qkv, S, H, Dh).float().cpu()
    q, k, v = qkv.float().cpu().view(B, S, 3, H, Dh).unbind(dim=2)
    s = torch.softmax(
        q.permute(0, 2, 1, 3) @ k.permute(0, 2, 1, 3).transpose(-1, -2) / Dh ** 0.5, -1
    )
    ref = (s @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(B, S, H * Dh)
    assert (o - ref).abs().max() < 0.03


@pytest.mark.parametrize("B,S,H,Dh", [(2, 96, 2, 32), (2, 128, 1, 64)])
def test_attention_qkv_mfma_more_than_one_tile_per_wave(B, S, H, Dh):
    """S > 64: the 4 waves each own more than one 16-row query tile. Every
    one of the S output rows must be computed (the output is allocated
    uninitialised), against the same CPU fp32 softmax reference and
    tolerance as test_attention_qkv_mfma_vs_reference."""
    from detectmateservice_amd import ops

    torch.manual_seed(7)
    qkv = (torch.randn(B, S, 3 * H * Dh) * 0.5).bfloat16().cuda()
    o = ops.attention_qkv(qkv, S, H, Dh).float().cpu()
    q, k, v = qkv.float().cpu().view(B, S, 3, H, Dh).unbind(dim=2)
    q = q.permute(0, 2, 1, 3)
    k = k.permute(0, 2, 1, 3)
    v = v.permute(0, 2, 1, 3)
    s = torch.softmax(q @ k.transpose(-1, -2) / Dh ** 0.5, -1)
    ref = (s @ v).permute(0, 2, 1, 3).reshape(B, S, H * Dh)
    assert o.shape == ref.shape
    err = (o - ref).abs().amax(dim=(0, 2))  # per query row
    assert torch.isfinite(o).all()
    assert err.max() < 0.03, (int(err.argmax()), float(err.max()))


def test_bert_fused_vs_layered():
    """Fused whole-model kernel vs the layered GPU path (same weights)."""
    from detectmateservice_amd import ops
    from detectmateservice_amd.models.bert_tiny import (
        BertTinyConfig,
        BertTinyDetectorModel,
    )
    from detectmateservice_amd.utils.synthetic import AuditLogGenerator

    model = BertTinyDetectorModel(BertTinyConfig(), device="cuda", seed=13)
    assert model._fused_ok()
    gen = AuditLogGenerator(seed=99)
    raw = [gen.line()[0].encode() for _ in range(128)]
    lines, lens = ops.pack_lines(raw, 256, device="cuda")
    start = torch.zeros(128, dtype=torch.int32, device="cuda")

    fused = model.score_spans(lines, start, lens.int())
    # layered path with identical weights
    tokens = model.tokenize_spans(lines, start, lens.int())
    layered = model.forward(tokens)
    diff = (fused - layered).abs().max().item()
    assert diff < 0.05, f"fused vs layered diff {diff}"
    # and against the CPU fp32 reference
    cpu = BertTinyDetectorModel(BertTinyConfig(), device="cpu", seed=13)
    ref = cpu.forward(tokens.cpu())
    assert (fused.cpu() - ref).abs().max() < 0.08


def test_multi_gpu_dp_pipeline():
    """Single-node multi-GPU DP (SURVEY §4.2's missing 4th tier); skips on
    1-GPU boxes — the 8-GPU scaling bench is driver-run."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >=2 GPUs")
    from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig
    from detectmateservice_amd.utils.synthetic import (
        AUDIT_LOG_FORMAT,
        AUDIT_TEMPLATES,
        AuditLogGenerator,
    )
    from detectmateservice_amd import ops

    outs = []
    for dev in ("cuda:0", "cuda:1"):
        cfg = PipelineConfig(
            templates=AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT,
            use_transformer=True, train_lines=0, seed=1,
        )
        pipe = GpuPipeline(cfg, device=dev)
        gen = AuditLogGenerator(seed=3)
        raw = [gen.line()[0].encode() for _ in range(64)]
        out = pipe.process_lines(raw)
        outs.append(out["scores"].cpu())
    assert torch.allclose(outs[0], outs[1], atol=1e-3)


def test_edit_distance_kernel_vs_python():
    """Wavefront-DP Levenshtein kernel vs the CPU reference on random and
    structured strings."""
    import random

    from detectmateservice_amd import ops
    from detectmateservice_amd.library.parsers.template_miner import (
        levenshtein_py,
    )
    from detectmateservice_amd.ops import _dmx_C

    rng = random.Random(7)
    alpha = b"abcdefgh "
    qs, rs = [], []
    for _ in range(12):
        n = rng.randrange(0, 200)
        qs.append(bytes(rng.choice(alpha) for _ in range(n)))
    for _ in range(9):
        n = rng.randrange(0, 250)
        rs.append(bytes(rng.choice(alpha) for _ in range(n)))
    qs.append(b"kitten"); rs.append(b"sitting")
    qa, ql = ops.pack_lines(qs, 256, device="cuda")
    ra, rl = ops.pack_lines(rs, 256, device="cuda")
    d = _dmx_C.edit_distance(qa, ql, ra, rl).cpu()
    for i, q in enumerate(qs):
        for j, r in enumerate(rs):
            assert int(d[i, j]) == levenshtein_py(q, r), (i, j, len(q), len(r))


def test_template_miner_gpu_matches_cpu():
    from detectmateservice_amd.library.parsers.template_miner import TemplateMiner
    from detectmateservice_amd.utils.synthetic import AuditLogGenerator

    gen = AuditLogGenerator(seed=5)
    contents = [gen.line()[0].split("): ", 1)[1] for _ in range(200)]
    cpu_t = TemplateMiner(device="cpu").fit(contents)
    gpu_t = TemplateMiner(device="cuda").fit(contents)
    assert cpu_t == gpu_t


def test_pipeline_graph_replay_matches_eager():
    """hipGraph-captured steady-state pipeline must produce identical
    results to the eager path on fresh data."""
    from detectmateservice_amd import ops
    from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig
    from detectmateservice_amd.utils.synthetic import (
        AUDIT_LOG_FORMAT,
        AUDIT_TEMPLATES,
        AuditLogGenerator,
    )

    B = 512
    cfg = PipelineConfig(
        templates=AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT,
        watches=[{"kind": "variable", "pos": 5, "event": 1}],
        train_lines=B, use_transformer=True, score_threshold=3.0,
    )
    pipe = GpuPipeline(cfg, device="cuda")
    gen = AuditLogGenerator(seed=3, anomaly_rate=0.05)
    train = [gen.line()[0].encode() for _ in range(B)]
    pipe.process_lines(train)  # training batch

    batch = [gen.line()[0].encode() for _ in range(B)]
    lines, lens = ops.pack_lines(batch, cfg.max_len, device="cuda")
    eager = pipe.process_packed(lines.clone(), lens.clone())
    eager_scores = eager["scores"].clone().cpu()
    eager_anom = eager["anomaly"].clone().cpu()
    seen_before = pipe.seen_lines

    assert pipe.enable_graph(B)
    out = pipe.process_packed_graph(lines, lens)
    torch.cuda.synchronize()
    assert torch.allclose(out["scores"].cpu(), eager_scores, atol=1e-4)
    assert torch.equal(out["anomaly"].cpu(), eager_anom)
    # replay again on different data
    batch2 = [gen.line()[0].encode() for _ in range(B)]
    l2, n2 = ops.pack_lines(batch2, cfg.max_len, device="cuda")
    out2 = pipe.process_packed_graph(l2, n2)
    torch.cuda.synchronize()
    ref2 = pipe.process_packed(l2, n2)
    assert torch.allclose(out2["scores"].cpu(), ref2["scores"].cpu(), atol=1e-4)


def test_mfma_32x32x16_layout_probe():
    """Pin the 32x32x16 bf16 fragment layout (used by block_gemm's wide
    fragments). Asymmetric operands (rule 16)."""
    from detectmateservice_amd.ops import _dmx_C

    torch.manual_seed(9)
    A = (torch.randn(32, 16) * 0.5 + torch.arange(32).view(32, 1) * 0.01).bfloat16().cuda()
    B = (torch.randn(16, 32) * 0.5 + torch.arange(32).view(1, 32) * 0.02).bfloat16().cuda()
    D = _dmx_C.probe_mfma32(A, B).cpu()
    ref = A.float().cpu() @ B.float().cpu()
    err = (D - ref).abs().max()
    assert err < 0.1, f"32x32x16 layout mismatch: max err {err}"


def test_bert_fused_four_layers():
    """The fused kernel loops arbitrary layer counts (runtime param)."""
    from detectmateservice_amd import ops
    from detectmateservice_amd.models.bert_tiny import (
        BertTinyConfig,
        BertTinyDetectorModel,
    )
    from detectmateservice_amd.utils.synthetic import AuditLogGenerator

    cfg = BertTinyConfig(layers=4)
    gpu = BertTinyDetectorModel(cfg, device="cuda", seed=21)
    cpu = BertTinyDetectorModel(cfg, device="cpu", seed=21)
    assert gpu._fused_ok()
    gen = AuditLogGenerator(seed=2)
    raw = [gen.line()[0].encode() for _ in range(64)]
    lines, lens = ops.pack_lines(raw, 256, device="cuda")
    start = torch.zeros(64, dtype=torch.int32, device="cuda")
    fused = gpu.score_spans(lines, start, lens.int()).cpu()
    tokens = cpu.tokenize_spans(lines.cpu(), start.cpu(), lens.int().cpu())
    ref = cpu.forward(tokens)
    assert (fused - ref).abs().max() < 0.1


def test_ops_fail_loudly_without_extension(monkeypatch):
    """On a GPU box, a CUDA tensor hitting the ops layer with the
    extension missing must raise (no silent eager fallback)."""
    from detectmateservice_amd import ops

    x = torch.randn(64, 128).bfloat16().cuda()
    wt = torch.randn(128, 128).bfloat16().cuda()
    monkeypatch.setattr(ops, "_C", None)
    with pytest.raises(RuntimeError, match="not built"):
        ops.fused_linear(x, wt)


@pytest.mark.gpu
def test_fused_pipeline_detector_gpu():
    """FusedPipelineDetector component end-to-end on the GPU: train on
    clean audit traffic, then a line with an unseen watched header value
    must alert (and only that line)."""
    from detectmateservice_amd.library.detectors import FusedPipelineDetector
    from detectmateservice_amd.schemas import DetectorSchema, LogSchema
    from detectmateservice_amd.utils.synthetic import (
        AUDIT_LOG_FORMAT,
        AUDIT_TEMPLATES,
        AuditLogGenerator,
    )

    det = FusedPipelineDetector({
        "templates": list(AUDIT_TEMPLATES),
        "log_format": AUDIT_LOG_FORMAT,
        "watches": [{"kind": "header", "pos": 0}],
        "data_use_training": 64,
        "use_transformer": True,
        "score_threshold": 1.0e9,  # NV-only alerts (random-init model)
        "device": "cuda",
    })
    gen = AuditLogGenerator(seed=17)
    train = [LogSchema(logID=f"t{i}", log=gen.line()[0]).serialize()
             for i in range(64)]
    assert all(o is None for o in det.process_batch(train))

    normal = [LogSchema(logID=f"n{i}", log=gen.line()[0]).serialize()
              for i in range(8)]
    bad = LogSchema(logID="bad", log=(
        "type=ZZZ_NEVER_SEEN msg=audit(1.0:1): pid=1 uid=0 auid=1 ses=1 "
        "msg='op=PAM:x acct=\"x\" exe=/bin/x hostname=? addr=? "
        "terminal=x res=success'"
    )).serialize()
    out = det.process_batch(normal + [bad])
    assert [o is not None for o in out] == [False] * 8 + [True]
    alert = DetectorSchema.deserialize(out[8])
    assert alert.logIDs == ["bad"]
    assert "unknown watched value" in alert.description


@pytest.mark.gpu
def test_fused_pipeline_detector_graph_matches_eager():
    """graph_batch replay (incl. padded partial batches) produces the same
    alerts as the eager path."""
    from detectmateservice_amd.library.detectors import FusedPipelineDetector
    from detectmateservice_amd.schemas import LogSchema
    from detectmateservice_amd.utils.synthetic import (
        AUDIT_LOG_FORMAT,
        AUDIT_TEMPLATES,
        AuditLogGenerator,
    )

    def build(graph_batch):
        return FusedPipelineDetector({
            "templates": list(AUDIT_TEMPLATES),
            "log_format": AUDIT_LOG_FORMAT,
            "watches": [{"kind": "header", "pos": 0}],
            "data_use_training": 64,
            "use_transformer": True,
            "score_threshold": 1.0e9,
            "graph_batch": graph_batch,
            "device": "cuda",
            "seed": 99,
        })

    gen = AuditLogGenerator(seed=23)
    train = [LogSchema(logID=f"t{i}", log=gen.line()[0]).serialize()
             for i in range(64)]
    lines = [gen.line()[0] for _ in range(40)]
    bad = ("type=ZZZ_NEW msg=audit(1.0:1): pid=1 uid=0 auid=1 ses=1 "
           "msg='op=PAM:x acct=\"x\" exe=/bin/x hostname=? addr=? "
           "terminal=x res=success'")
    batch = [LogSchema(logID=f"n{i}", log=l).serialize()
             for i, l in enumerate(lines)] + [
        LogSchema(logID="bad", log=bad).serialize()]

    eager, graph = build(0), build(64)
    eager.process_batch(train)
    graph.process_batch(train)
    out_e = eager.process_batch(batch)       # 41 frames, eager
    out_g = graph.process_batch(batch)       # 41 <= graph_batch 64: padded
    assert [o is not None for o in out_e] == [o is not None for o in out_g]
    assert out_g[-1] is not None
    # full-size batch through the graph
    out_g2 = graph.process_batch(batch[:40] + batch[:23] + [batch[-1]])
    assert out_g2[-1] is not None
    assert sum(o is not None for o in out_g2) == 1
