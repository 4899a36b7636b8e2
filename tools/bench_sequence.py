"""What event-sequence detection costs in the fused pipeline.

    python tools/bench_sequence.py [--batch 65536] [--rounds 5] [--iters 10]

Two configurations on the audit-log generator bench.py uses, transformer off
so that the parse + detect stages are what is timed:
  a  watches            two watches (acct, exe of event 1)
  b  watches+sequence   the same plus event_sequence with length 3, keyed on
                        capture 3 (`ses=` of the templates that carry it there)

(a) and (b) each train on one batch, are warmed up, and are then timed in
alternation for `rounds` rounds, first eager and then as a captured graph; a
round times `iters` back-to-back steps over a pool of distinct device-resident
batches between two device events. rounds * iters is the number of timed steps
(50 by default). Before timing, (b)'s outputs outside its own keys are
compared with (a)'s on every pool batch, and its seq_gram / seq_unseen on the
first `--check-rows` rows of one batch with the CPU mirror started from the
same state, to the bit. The stage moves its histories on every step, so the
timed steps do the work of a live stream.

`--no-sequence` times (a) alone and never names the `event_sequence` key, so
that the same file runs against a checkout that predates the feature. Needs a
GPU: there is no CPU fallback."""
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
SEQUENCE = {"length": 3,
            "key": {"kind": "variable", "pos": 3, "event": -1, "name": "ses"}}


def make_pipe(batch: int, max_len: int, sequence, device="cuda") -> GpuPipeline:
    extra = {} if sequence is None else {"event_sequence": sequence}
    cfg = PipelineConfig(
        templates=AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT,
        watches=WATCHES, train_lines=batch, use_transformer=False,
        max_len=max_len, **extra)
    return GpuPipeline(cfg, device=device)


def timed(pipes, pool, rounds, iters, how):
    ms = {k: [] for k in pipes}
    for _ in range(rounds):
        for name, pipe in pipes.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(iters):
                getattr(pipe, how)(*pool[i % len(pool)])
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / iters)
    return ms


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--check-rows", type=int, default=2048)
    ap.add_argument("--no-sequence", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.have_extension():
        sys.exit("bench_sequence needs a GPU and the built HIP extension")

    B = args.batch
    gen = AuditLogGenerator(seed=1000, anomaly_rate=0.01)
    raw_pool = [[gen.line()[0].encode() for _ in range(B)] for _ in range(args.pool + 1)]
    pool = [ops.pack_lines(raw, args.max_len, device="cuda") for raw in raw_pool]
    train, pool = pool[0], pool[1:]

    pipes = {"watches": make_pipe(B, args.max_len, None)}
    if not args.no_sequence:
        pipes["watches+sequence"] = make_pipe(B, args.max_len, SEQUENCE)
    for pipe in pipes.values():
        pipe.process_packed(*train)

    members = unseen = 0
    if not args.no_sequence:
        seq = pipes["watches+sequence"]
        assert bool((seq.event_sequence.seq_key != 0).any()), "no key entered a bucket"
        own = set(seq.stages[1].keys)
        for lines, lens in pool:
            a = pipes["watches"].process_packed(lines, lens)
            b = seq.process_packed(lines, lens)
            assert set(b) - set(a) == own and b["seq_gram"].shape == (B,)
            assert torch.equal(a["nv_unseen"], b["nv_unseen"])
            assert torch.equal(a["event_id"], b["event_id"])
            assert torch.equal(a["scores"], b["scores"])
            assert torch.equal(a["anomaly"] | (b["seq_unseen"] > 0), b["anomaly"])
            members += int((b["seq_gram"] != 0).sum())
            unseen += int(b["seq_unseen"].sum())
        assert members > 0, "no line was a member of a sequence"
        # the device against the mirror, from the same state
        n = min(args.check_rows, B)
        mirror = make_pipe(B, args.max_len, SEQUENCE, device="cpu")
        mirror.seen_lines = B
        mirror.stages[1].load_state_dict(seq.stages[1].state_dict())
        want = mirror.process_packed(pool[0][0][:n].cpu(), pool[0][1][:n].cpu())
        got = seq.process_packed(pool[0][0][:n], pool[0][1][:n])
        for k in ("seq_gram", "seq_unseen"):
            assert torch.equal(got[k].cpu(), want[k]), k
        for k in ops.EventSequenceState._STATE:
            assert torch.equal(getattr(seq.event_sequence, k).cpu(),
                               getattr(mirror.event_sequence, k)), k

    for pipe in pipes.values():
        for i in range(args.warmup):
            pipe.process_packed(*pool[i % len(pool)])
    torch.cuda.synchronize()
    ms = {"eager": timed(pipes, pool, args.rounds, args.iters, "process_packed")}
    for pipe in pipes.values():
        pipe.enable_graph(B)
        for i in range(args.warmup):
            pipe.process_packed_graph(*pool[i % len(pool)])
    torch.cuda.synchronize()
    ms["graph"] = timed(pipes, pool, args.rounds, args.iters, "process_packed_graph")

    steps = args.rounds * args.iters
    result = {"batch": B, "rounds": args.rounds, "iters": args.iters,
              "timed_steps": steps,
              "event_sequence": None if args.no_sequence else SEQUENCE,
              "member_rows_in_pool": members, "unseen_grams_in_pool": unseen,
              "device": torch.cuda.get_device_name(0)}
    print(f"batch {B}, {steps} timed steps per configuration and mode "
          f"({args.rounds} rounds of {args.iters}), ms per step")
    print(f"{'mode':6s} {'configuration':17s} {'median':>9s} {'min':>9s} {'max':>9s} "
          f"{'lines/s':>12s}")
    for mode, by_name in ms.items():
        result[mode] = {}
        for name, v in by_name.items():
            med = statistics.median(v)
            result[mode][name] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v),
                                  "lines_per_s": B / med * 1e3}
            print(f"{mode:6s} {name:17s} {med:9.3f} {min(v):9.3f} {max(v):9.3f} "
                  f"{B / med * 1e3:12.0f}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
