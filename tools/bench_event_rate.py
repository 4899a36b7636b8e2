"""What event-rate detection costs in the fused pipeline, and what it
replaces.

    python tools/bench_event_rate.py [--batch 65536] [--rounds 5] [--iters 10]

Three configurations on the audit-log generator bench.py uses, transformer
off so that the parse + detect stages are what is timed:
  a  watches         two watches (acct, exe of event 1), no event_rate
  b  watches+rate    the same plus event_rate at window_lines 1000
  c  host rate       the only way to get (b)'s answer without the feature:
                     the same parse on the GPU, then FrequencyDetector on
                     the host, frame by frame, over the parsed lines

The generator draws its events independently, so a stream of it holds no
rate anomaly. In one batch of each stream a run of lines is therefore
replaced by copies of one line: that event floods its windows and every
other event drops in them.

(a) and (b) each train on one batch, are warmed up, and are then timed in
alternation for `rounds` rounds; a round times `iters` back-to-back steps
over a pool of distinct device-resident batches between two device events.
rounds * iters is the number of timed steps (50 by default). (c) runs at
`--host-batch` lines, small enough to finish in seconds; its ParserSchema
frames are serialised before the clock starts, and the clock stops after
the device synchronise and the last frame. Before timing, (b)'s per-line
outputs are compared with (a)'s on every pool batch, and (c)'s alert lines
and scores with (b)'s rate_hits over a stream of host batches. Needs a GPU:
there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from detectmateservice_amd import ops  # noqa: E402
from detectmateservice_amd.library.detectors import FrequencyDetector  # noqa: E402
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig  # noqa: E402
from detectmateservice_amd.schemas import DetectorSchema, ParserSchema  # noqa: E402
from detectmateservice_amd.utils.synthetic import (  # noqa: E402
    AUDIT_LOG_FORMAT,
    AUDIT_TEMPLATES,
    AuditLogGenerator,
)

WATCHES = [
    {"kind": "variable", "pos": 5, "event": 1},   # acct
    {"kind": "variable", "pos": 6, "event": 1},   # exe
]
RATE = {"window_lines": 1000, "ewma_alpha": 0.3, "z_threshold": 4.0,
        "min_windows": 3}


def make_pipe(batch: int, max_len: int, event_rate) -> GpuPipeline:
    cfg = PipelineConfig(
        templates=AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT,
        watches=WATCHES, train_lines=batch, use_transformer=False,
        max_len=max_len, event_rate=event_rate)
    return GpuPipeline(cfg, device="cuda")


def flood(raw, start: int, n: int) -> None:
    """Replace raw[start : start + n] by copies of raw[start]."""
    raw[start:start + n] = [raw[start]] * len(raw[start:start + n])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pool", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--host-batch", type=int, default=4096)
    ap.add_argument("--host-steps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available() or not ops.have_extension():
        sys.exit("bench_event_rate needs a GPU and the built HIP extension")

    B, L = args.batch, RATE["window_lines"]
    gen = AuditLogGenerator(seed=1000, anomaly_rate=0.01)
    raw_pool = [[gen.line()[0].encode() for _ in range(B)] for _ in range(args.pool + 1)]
    flood(raw_pool[2], B // 2, 3 * L)
    pool = [ops.pack_lines(raw, args.max_len, device="cuda") for raw in raw_pool]
    train, pool = pool[0], pool[1:]

    pipes = {"watches": make_pipe(B, args.max_len, None),
             "watches+rate": make_pipe(B, args.max_len, dict(RATE))}
    for pipe in pipes.values():
        pipe.process_packed(*train)

    # same per-line answers before anything is timed; rate alerts only on
    # boundary lines
    rate_alerts = 0
    for lines, lens in pool:
        a = pipes["watches"].process_packed(lines, lens)
        b = pipes["watches+rate"].process_packed(lines, lens)
        assert a.get("rate_hits") is None and b["rate_hits"].shape == (B,)
        assert b["rate_counts"].shape == (B // L + 2, len(AUDIT_TEMPLATES) + 1)
        assert torch.equal(a["nv_unseen"], b["nv_unseen"])
        assert torch.equal(a["event_id"], b["event_id"])
        hit = b["rate_hits"] > 0
        assert torch.equal(a["anomaly"] | hit, b["anomaly"])
        assert bool((b["rate_slot"][hit] >= 0).all())
        rate_alerts += int(hit.sum())
    assert rate_alerts > 0, "the flood raised no rate alert"

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

    # (c) the parse on the GPU, the rate per frame on the host. The stream:
    # one training batch, then host_steps timed batches, the last of them
    # with a flood; checked against (b)'s configuration at the same batch.
    hb = args.host_batch
    host_pipe = make_pipe(hb, args.max_len, None)
    check_pipe = make_pipe(hb, args.max_len, dict(RATE))
    detector = FrequencyDetector({"data_use_training": hb, **RATE})
    host_batches = []
    for k in range(args.host_steps + 1):
        raw = list(raw_pool[k % len(raw_pool)][k * 7:k * 7 + hb])
        if k == args.host_steps:
            flood(raw, hb // 4, min(2 * L, hb // 2))
        lines, lens = ops.pack_lines(raw, args.max_len, device="cuda")
        want = check_pipe.process_packed(lines, lens)
        ev = want["event_id"].cpu().tolist()
        frames = [ParserSchema(EventID=e, logID=f"l{i}").serialize()
                  for i, e in enumerate(ev)]
        hits = want["rate_hits"].cpu()
        host_batches.append((lines, lens, frames, {
            i: float(hits[i]) for i in torch.nonzero(hits).flatten().tolist()}))
    lines, lens, frames, want = host_batches[0]  # training step, untimed
    assert not want
    host_pipe.process_packed(lines, lens)
    for f in frames:
        detector.process(f)
    torch.cuda.synchronize()
    host_s = []
    host_alerts = 0
    for lines, lens, frames, want in host_batches[1:]:
        t0 = time.perf_counter()
        host_pipe.process_packed(lines, lens)
        alerts = [detector.process(f) for f in frames]
        torch.cuda.synchronize()
        host_s.append(time.perf_counter() - t0)
        got = {i: DetectorSchema.deserialize(a).score
               for i, a in enumerate(alerts) if a is not None}
        assert got == want, "host detector and rate_hits disagree"
        host_alerts += len(got)
    assert host_alerts > 0, "the host stream raised no rate alert"

    steps = args.rounds * args.iters
    result = {"batch": B, "rounds": args.rounds, "iters": args.iters,
              "timed_steps": steps, "event_rate": RATE,
              "rate_alerts_in_pool": rate_alerts,
              "rate_alerts_host": host_alerts,
              "device": torch.cuda.get_device_name(0)}
    print(f"batch {B}, {steps} timed steps per configuration "
          f"({args.rounds} rounds of {args.iters}), ms per step")
    print(f"{'configuration':16s} {'median':>9s} {'min':>9s} {'max':>9s} {'lines/s':>12s}")
    for name, v in ms.items():
        med = statistics.median(v)
        result[name] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v),
                        "lines_per_s": B / med * 1e3}
        print(f"{name:16s} {med:9.3f} {min(v):9.3f} {max(v):9.3f} {B / med * 1e3:12.0f}")
    med = statistics.median(host_s)
    result["host rate"] = {"batch": hb, "steps": args.host_steps,
                           "median_ms": med * 1e3, "min_ms": min(host_s) * 1e3,
                           "max_ms": max(host_s) * 1e3, "lines_per_s": hb / med}
    print(f"{'host rate':16s} {med * 1e3:9.3f} {min(host_s) * 1e3:9.3f} "
          f"{max(host_s) * 1e3:9.3f} {hb / med:12.0f}   (batch {hb})")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
