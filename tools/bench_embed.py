"""Embedding / distance head of the fused BERT kernel against the production
score head and the layered embedding body, in ms per batch.

    python tools/bench_embed.py [--batch 65536] [--rounds 7] [--iters 30]

Four variants on the same seeded batch of generator lines:
  score       dmx_bert_fused_bf16 (the production kernel)
  dist        dmx_bert_fused_embed_bf16, want_emb=False (steady-state detect)
  emb+dist    dmx_bert_fused_embed_bf16, want_emb=True
  layered     tokenize + the per-op transformer body + mean-pool
              (what EmbeddingDetector.embed runs)

Every variant is warmed up, then the variants are timed in alternation for
`rounds` rounds, each timing `iters` back-to-back calls between two device
events. The table gives the median, the minimum and the maximum over the
rounds; the production kernel's min..max is the run-to-run spread a
difference has to exceed. The outputs of the variants are compared once
before timing. Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from detectmateservice_amd import ops  # noqa: E402
from detectmateservice_amd.models.bert_tiny import (  # noqa: E402
    BertTinyConfig,
    BertTinyDetectorModel,
)
from detectmateservice_amd.utils.synthetic import AuditLogGenerator  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-len", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.have_extension():
        sys.exit("bench_embed needs a GPU and the built HIP extension")
    from detectmateservice_amd.ops import _dmx_C

    B = args.batch
    gen = AuditLogGenerator(seed=1)
    raw = [gen.line()[0].encode() for _ in range(min(B, 8192))]
    raw = (raw * (B // len(raw) + 1))[:B]
    lines, lens = ops.pack_lines(raw, args.max_len, device="cuda")
    start = torch.zeros(B, dtype=torch.int32, device="cuda")
    end = lens.int().contiguous()
    m = BertTinyDetectorModel(BertTinyConfig(), device="cuda")
    assert m._fused_ok()
    wb, fb = m._fused_blobs()
    n_layers = m.config.layers
    g = torch.Generator().manual_seed(2)
    mu = (torch.randn(128, generator=g) * 0.5).cuda()
    inv_var = (1e2 + 9e2 * torch.rand(128, generator=g)).cuda()

    def layered():
        tokens = m.tokenize_spans(lines, start, end)
        return m._encode(tokens).float().mean(dim=1)

    variants = {
        "score": lambda: _dmx_C.bert_fused_bf16(
            lines, start, end, wb, fb, n_layers, 1e-5),
        "dist": lambda: _dmx_C.bert_fused_embed(
            lines, start, end, wb, fb, n_layers, 1e-5, mu, inv_var, False),
        "emb+dist": lambda: _dmx_C.bert_fused_embed(
            lines, start, end, wb, fb, n_layers, 1e-5, mu, inv_var, True),
        "layered": layered,
    }
    # the layered body is several times slower: fewer calls per window
    iters = {k: args.iters for k in variants}
    iters["layered"] = max(1, args.iters // 5)

    # outputs agree before anything is timed
    score = variants["score"]()
    _, dist = variants["dist"]()
    emb, dist2 = variants["emb+dist"]()
    assert torch.equal(dist, dist2)
    head = (emb @ m.w_score.float() + m.b_score).squeeze(-1)
    lay = layered()
    check = {
        "max|emb@w+b - score|": float((head - score).abs().max()),
        "max|emb - layered|": float((emb - lay).abs().max()),
    }
    del score, dist, dist2, emb, head, lay

    for name, fn in variants.items():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

    ms = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters[name]):
                fn()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / iters[name])

    result = {"batch": B, "rounds": args.rounds, "iters": iters, "check": check}
    print(f"batch {B}, {args.rounds} rounds, ms per batch")
    print(f"{'variant':10s} {'median':>9s} {'min':>9s} {'max':>9s} {'lines/s':>12s}")
    for name, v in ms.items():
        med = statistics.median(v)
        result[name] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v)}
        print(f"{name:10s} {med:9.3f} {min(v):9.3f} {max(v):9.3f} "
              f"{B / med * 1e3:12.0f}")
    for k, v in check.items():
        print(f"{k}: {v:.3e}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
