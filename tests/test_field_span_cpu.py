"""The field-span lookup (field_span.h, ops._field_span) on the CPU: the
mirror against a reference that never sees the matcher's capture tables,
and a hand-built batch whose rows break every promise the lookup checks.

docs/kernels.md, "Parsed batch and field span", states the clauses."""
import random
import re

import torch

from detectmateservice_amd import ops
from detectmateservice_amd.utils.synthetic import (
    AUDIT_LOG_FORMAT,
    AUDIT_TEMPLATES,
    AuditLogGenerator,
)

B, MAX_LEN = 16, 64
#: content variables at pos 0, 1 and 5, header variables at pos 0 and 3
SPECS = [
    {"kind": "variable", "pos": 0},
    {"kind": "variable", "pos": 1},
    {"kind": "variable", "pos": 5},
    {"kind": "header", "pos": 0},
    {"kind": "header", "pos": 3},
]


def hostile_batch():
    """(lines, match, present): 16 lines of random letters with two captures
    and one header field each, all inside the line, except for rows 1..5,
    and present [B, 5], whether SPECS[w] names a field on line i.

    Every address that even an unguarded lookup would compute from these
    rows lies inside caps, fmt_caps and lines (the hostile rows are away from
    row 0 and from the last rows), so a lookup that lacks a clause shows as a
    wrong hash, never as a fault."""
    rng = random.Random(17)
    lines = torch.tensor(
        [[rng.randrange(97, 123) for _ in range(MAX_LEN)] for _ in range(B)],
        dtype=torch.uint8)
    caps = torch.tensor([[4, 12], [20, 31]], dtype=torch.int32).repeat(B, 1, 1)
    fmt_caps = torch.tensor([[40, 52]], dtype=torch.int32).repeat(B, 1, 1)
    n_caps = torch.full((B,), 2, dtype=torch.int32)
    n_fmt_caps = torch.full((B,), 1, dtype=torch.int32)
    present = torch.tensor([[1, 1, 0, 1, 0]] * B, dtype=torch.bool)

    n_caps[1] = 9                                       # the table holds 2
    caps[2, 0] = torch.tensor([60, 68], dtype=torch.int32)   # ends past max_len
    present[2, 0] = False
    caps[3, 0] = torch.tensor([-3, 5], dtype=torch.int32)    # starts before the line
    present[3, 0] = False
    caps[4, 1] = torch.tensor([9, 4], dtype=torch.int32)     # ends before it starts
    present[4, 1] = False
    n_fmt_caps[5] = 7                                   # the table holds 1
    match = {"event_id": torch.ones(B, dtype=torch.int32), "caps": caps,
             "n_caps": n_caps, "fmt_caps": fmt_caps, "n_fmt_caps": n_fmt_caps}
    return lines, match, present


def spec_rows(flags: int = 0) -> torch.Tensor:
    rows = [ops.watch_spec_row(s)[:3] + [flags] for s in SPECS]
    return torch.tensor(rows, dtype=torch.int32)


def test_mirror_against_values_cut_by_regex():
    gen = AuditLogGenerator(seed=29)
    raw = [gen.line()[0] for _ in range(256)]
    matcher = ops.TemplateMatcher(AUDIT_TEMPLATES, log_format=AUDIT_LOG_FORMAT,
                                  device="cpu")
    lines, lens = ops.pack_lines([r.encode() for r in raw], max_len=512)
    match = matcher.match_packed(lines, lens)
    specs = torch.tensor([[0, 1, 5, 0], [1, -1, 0, 0]], dtype=torch.int32)
    got = ops.watch_hashes_cpu(lines, match, specs).tolist()

    # event 1 is the only template with "msg='op=<*> acct=<*> exe=": its
    # sixth capture is the acct value; header field 0 is <Type>
    acct = re.compile(r" msg='op=.*? acct=(.*?) exe=")
    head = re.compile(r"^type=(.*?) msg=audit\(")
    n_acct = 0
    for i, line in enumerate(raw):
        m = acct.search(line)
        want = ops._as_i64(ops.fnv1a64(m.group(1).encode())) if m else 0
        assert got[i][0] == want, line
        n_acct += m is not None
        assert got[i][1] == ops._as_i64(
            ops.fnv1a64(head.match(line).group(1).encode())), line
    assert 0 < n_acct < len(raw)


def test_hostile_batch_is_absent_in_every_mirror():
    lines, match, present = hostile_batch()
    # a spec with pos = -1 names nothing on any line
    specs = torch.cat([spec_rows(), torch.tensor([[0, -1, -1, 0]], dtype=torch.int32)])
    present = torch.cat([present, torch.zeros((B, 1), dtype=torch.bool)], dim=1)
    W = specs.shape[0]

    h = ops.watch_hashes_cpu(lines, match, specs)
    assert torch.equal(h != 0, present)

    combo_off = torch.tensor([0, W], dtype=torch.int32)
    hc = ops.watch_combo_hashes_cpu(lines, match, specs, specs, combo_off)
    assert torch.equal(hc[:, :W], h)
    # every member is relevant on every line; an absent one contributes 0
    want = ops.combo_fold(torch.ones((B, W), dtype=torch.int64).numpy(), h.numpy())
    assert hc[:, W].tolist() == want.tolist()
    assert bool((hc[:, W] != 0).all())

    ranges = specs.clone()
    ranges[:, 3] = 1  # non_numeric: alert, so a present field of letters gets 3
    code, value = ops.value_range_step_cpu(
        lines, match, ranges, torch.zeros(W, dtype=torch.float64),
        torch.full((W,), float("inf"), dtype=torch.float64),
        torch.full((W,), float("-inf"), dtype=torch.float64),
        torch.zeros(W, dtype=torch.int64), 0)
    assert torch.equal(code, torch.where(present, 3, 0).to(torch.int32))
    assert not value.any()
