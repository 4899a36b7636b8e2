"""What numeric value-range detection costs in the fused pipeline.

    python tools/bench_ranges.py [--batch 65536] [--rounds 5] [--iters 10]

Two configurations on the audit-log generator bench.py uses, transformer off
so that the parse + detect stages are what is timed:
  a  watches          two watches (acct, exe of event 1), no ranges
  b  watches+ranges   the same plus two ranges: a content variable (pid of
                      event 1) and a header field (the audit timestamp,
                      `1642723741.123`: 13 digits, a number of the grammar)

(a) and (b) each train on one batch, are warmed up, and are then timed in
alternation for `rounds` rounds; a round times `iters` back-to-back steps
over a pool of distinct device-resident batches between two device events.
rounds * iters is the number of timed steps (50 by default). Before timing,
(b)'s per-line outputs are compared with (a)'s on every pool batch, and its
range_code / range_value on the first `--check-rows` rows of one batch with
the CPU mirror started from the same learnt state, to the bit. The audit
timestamp grows along the stream, so every pool batch holds values above the
trained range: the alert count is checked to be non-zero.

`--no-ranges` times (a) alone and never names the `ranges` key, so that the
same file runs against a checkout that predates the feature. Needs a GPU:
there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from detectmateservice_amd import ops  # noqa: E402
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig  # noqa: E402
from detectmateservice_amd.utils.synthetic import (  # noqa: E402
    AUDIT_LOG_FORMAT,
    AUDIT_TEMPLATES,
    AuditLogGenerator,
)

WATCHES = [
    {"kind": "variable", "pos": 5, "event": 1},   # acct
    {"kind": "variable", "pos": 6, "event": 1},   # exe
]
RANGES = [
    {"kind": "variable", "pos": 0, "event": 1, "name": "pid"},
    {"kind": "header", "pos": 1, "name": "time", "non_numeric": "alert"},
]


def make_pipe(batch: int, max_len: int, ranges, device="cuda") -> GpuPipeline:
    extra = {} if ranges is None else {"ranges": ranges}
    cfg = PipelineConfig(
        templates=AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT,
        watches=WATCHES, train_lines=batch, use_transformer=False,
        max_len=max_len, **extra)
    return GpuPipeline(cfg, device=device)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--check-rows", type=int, default=2048)
    ap.add_argument("--no-ranges", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.have_extension():
        sys.exit("bench_ranges needs a GPU and the built HIP extension")

    B = args.batch
    gen = AuditLogGenerator(seed=1000, anomaly_rate=0.01)
    raw_pool = [[gen.line()[0].encode() for _ in range(B)] for _ in range(args.pool + 1)]
    pool = [ops.pack_lines(raw, args.max_len, device="cuda") for raw in raw_pool]
    train, pool = pool[0], pool[1:]

    pipes = {"watches": make_pipe(B, args.max_len, None)}
    if not args.no_ranges:
        pipes["watches+ranges"] = make_pipe(B, args.max_len, RANGES)
    for pipe in pipes.values():
        pipe.process_packed(*train)

    range_alerts = 0
    if not args.no_ranges:
        state = pipes["watches+ranges"].value_ranges
        assert bool((state.n > 0).all()), "a range learnt nothing in training"
        for lines, lens in pool:
            a = pipes["watches"].process_packed(lines, lens)
            b = pipes["watches+ranges"].process_packed(lines, lens)
            assert "range_code" not in a and b["range_code"].shape == (B, len(RANGES))
            assert torch.equal(a["nv_unseen"], b["nv_unseen"])
            assert torch.equal(a["event_id"], b["event_id"])
            hit = (b["range_code"] != 0).any(dim=1)
            assert torch.equal(a["anomaly"] | hit, b["anomaly"])
            range_alerts += int(hit.sum())
        assert range_alerts > 0, "no value left its trained range"
        # the device against the mirror, from the same learnt state
        n = min(args.check_rows, B)
        mirror = make_pipe(B, args.max_len, RANGES, device="cpu")
        mirror.seen_lines = B
        mirror.value_ranges.load_state_dict(state.state_dict())
        want = mirror.process_packed(pool[0][0][:n].cpu(), pool[0][1][:n].cpu())
        got = pipes["watches+ranges"].process_packed(pool[0][0][:n], pool[0][1][:n])
        for k in ("range_code", "range_value"):
            assert torch.equal(_bits(got[k].cpu()), _bits(want[k])), k

    for pipe in pipes.values():
        for i in range(args.warmup):
            pipe.process_packed(*pool[i % len(pool)])
    torch.cuda.synchronize()

    ms = {k: [] for k in pipes}
    for _ in range(args.rounds):
        for name, pipe in pipes.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(args.iters):
                pipe.process_packed(*pool[i % len(pool)])
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / args.iters)

    steps = args.rounds * args.iters
    result = {"batch": B, "rounds": args.rounds, "iters": args.iters,
              "timed_steps": steps, "ranges": None if args.no_ranges else RANGES,
              "range_alerts_in_pool": range_alerts,
              "device": torch.cuda.get_device_name(0)}
    print(f"batch {B}, {steps} timed steps per configuration "
          f"({args.rounds} rounds of {args.iters}), ms per step")
    print(f"{'configuration':16s} {'median':>9s} {'min':>9s} {'max':>9s} {'lines/s':>12s}")
    for name, v in ms.items():
        med = statistics.median(v)
        result[name] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v),
                        "lines_per_s": B / med * 1e3}
        print(f"{name:16s} {med:9.3f} {min(v):9.3f} {max(v):9.3f} {B / med * 1e3:12.0f}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
