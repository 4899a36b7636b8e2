"""What NewValue combination detection costs in the fused pipeline, and what
it replaces.

    python tools/bench_combo.py [--batch 65536] [--rounds 5] [--iters 10]

Three configurations on the audit-log generator bench.py uses, transformer
off so that the parse + hash stage is what is timed:
  a  watches       two watches (acct, exe of event 1)
  b  watches+combo the same watches plus one combination of the two
  c  host combo    the only way to get (b)'s answer without the feature:
                   the watches on the GPU, then NewValueComboDetector on
                   the host, frame by frame, over the parsed lines

The generator draws acct and exe independently from short lists, so a
stream of it holds no new combination. One (acct, exe) pair is therefore
held out of the training batch (its lines are replaced by another line); in
the timed batches it is the `alice from host B` case: both values known,
the pair new.

(a) and (b) each train on one batch, are warmed up, and are then timed in
alternation for `rounds` rounds; a round times `iters` back-to-back steps
over a pool of distinct device-resident batches between two device events.
rounds * iters is the number of timed steps (50 by default). (c) runs at
`--host-batch` lines, small enough to finish in seconds; its ParserSchema
frames are serialised before the clock starts, and the clock stops after
the device synchronise and the last frame. Before timing, (b)'s watch
columns are compared with (a)'s on every pool batch, and (c)'s alert rows
with (b)'s combination column. Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from detectmateservice_amd import ops  # noqa: E402
from detectmateservice_amd.library.detectors.new_value import (  # noqa: E402
    NewValueComboDetector,
)
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig  # noqa: E402
from detectmateservice_amd.schemas import ParserSchema  # noqa: E402
from detectmateservice_amd.utils.synthetic import (  # noqa: E402
    AUDIT_LOG_FORMAT,
    AUDIT_TEMPLATES,
    AuditLogGenerator,
)

WATCHES = [
    {"kind": "variable", "pos": 5, "event": 1},   # acct
    {"kind": "variable", "pos": 6, "event": 1},   # exe
]


PAIR = re.compile(rb'acct=(\S+) exe=(\S+)')


def hold_out_pair(train_raw):
    """Replace every training line that carries the first (acct, exe) pair
    of the batch by a line that does not; returns the pair."""
    pairs = [m.groups() if m else None for m in map(PAIR.search, train_raw)]
    held = next(p for p in pairs if p is not None)
    filler = next(line for line, p in zip(train_raw, pairs) if p != held)
    for i, p in enumerate(pairs):
        if p == held:
            train_raw[i] = filler
    return held


def make_pipe(batch: int, max_len: int, combos) -> GpuPipeline:
    cfg = PipelineConfig(
        templates=AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT,
        watches=WATCHES, combos=combos, train_lines=batch,
        use_transformer=False, max_len=max_len)
    return GpuPipeline(cfg, device="cuda")


def parser_frames(raw, match) -> list:
    """What a parser stage would hand the host detector for these lines."""
    ev = match["event_id"].cpu().tolist()
    caps = match["caps"].cpu().tolist()
    n_caps = match["n_caps"].cpu().tolist()
    frames = []
    for i, line in enumerate(raw):
        variables = [line[a:b].decode("utf-8", "replace")
                     for a, b in caps[i][:min(n_caps[i], len(caps[i]))]]
        frames.append(ParserSchema(
            EventID=max(ev[i], 0), logID=f"l{i}", variables=variables).serialize())
    return frames


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
        sys.exit("bench_combo needs a GPU and the built HIP extension")

    B = args.batch
    gen = AuditLogGenerator(seed=1000, anomaly_rate=0.01)
    raw_pool = [[gen.line()[0].encode() for _ in range(B)] for _ in range(args.pool + 1)]
    held = hold_out_pair(raw_pool[0])
    pool = [ops.pack_lines(raw, args.max_len, device="cuda") for raw in raw_pool]
    train, pool = pool[0], pool[1:]

    pipes = {"watches": make_pipe(B, args.max_len, ()),
             "watches+combo": make_pipe(B, args.max_len, [WATCHES])}
    for pipe in pipes.values():
        pipe.process_packed(*train)

    # same answers before anything is timed
    combo_alerts = 0
    for lines, lens in pool:
        a = pipes["watches"].process_packed(lines, lens)
        b = pipes["watches+combo"].process_packed(lines, lens)
        assert a["combo_unseen"] is None and b["combo_unseen"].shape == (B, 1)
        assert torch.equal(a["nv_unseen"], b["nv_unseen"])
        assert torch.equal(a["event_id"], b["event_id"])
        combo_alerts += int(b["combo_unseen"].sum())
    assert combo_alerts > 0, "the held-out pair never occurs in the pool"

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

    # (c) the watches on the GPU, the combination per frame on the host
    hb = args.host_batch
    host_pipe = make_pipe(hb, args.max_len, ())
    check_pipe = make_pipe(hb, args.max_len, [WATCHES])
    detector = NewValueComboDetector({
        "events": {1: {"combo": {"variables": [{"pos": 5}, {"pos": 6}]}}},
        "data_use_training": hb,
    })
    host_batches = []
    host_alerts = 0
    for k in range(args.host_steps + 1):
        raw = raw_pool[k % len(raw_pool)][k * 7:k * 7 + hb]
        lines, lens = ops.pack_lines(raw, args.max_len, device="cuda")
        want = check_pipe.process_packed(lines, lens)
        host_batches.append((lines, lens, parser_frames(raw, want["match"]),
                             want["combo_unseen"][:, 0].cpu().bool().tolist()))
    lines, lens, frames, _ = host_batches[0]  # training step, untimed
    host_pipe.process_packed(lines, lens)
    for f in frames:
        detector.process(f)
    torch.cuda.synchronize()
    host_s = []
    for lines, lens, frames, want in host_batches[1:]:
        t0 = time.perf_counter()
        out = host_pipe.process_packed(lines, lens)
        alerts = [detector.process(f) is not None for f in frames]
        torch.cuda.synchronize()
        host_s.append(time.perf_counter() - t0)
        assert out["nv_unseen"] is not None
        assert alerts == want, "host detector and combo column disagree"
        host_alerts += sum(alerts)

    steps = args.rounds * args.iters
    result = {"batch": B, "rounds": args.rounds, "iters": args.iters,
              "timed_steps": steps, "held_out_pair": [x.decode() for x in held],
              "combo_alerts_in_pool": combo_alerts,
              "combo_alerts_host": host_alerts,
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
    result["host combo"] = {"batch": hb, "steps": args.host_steps,
                            "median_ms": med * 1e3, "min_ms": min(host_s) * 1e3,
                            "max_ms": max(host_s) * 1e3, "lines_per_s": hb / med}
    print(f"{'host combo':16s} {med * 1e3:9.3f} {min(host_s) * 1e3:9.3f} "
          f"{max(host_s) * 1e3:9.3f} {hb / med:12.0f}   (batch {hb})")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
