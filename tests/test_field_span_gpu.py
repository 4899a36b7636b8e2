"""The field-span lookup on the GPU: the three kernels that use it against
their CPU mirrors, to the bit, on the hostile batch of
test_field_span_cpu.py, and the literal "absent" of every hostile cell."""
import pytest
import torch

from detectmateservice_amd import ops
from test_field_span_cpu import B, SPECS, hostile_batch, spec_rows

pytestmark = pytest.mark.gpu


def test_hostile_batch_matches_mirrors_and_is_absent():
    lines, match, present = hostile_batch()
    specs = spec_rows()
    W = len(SPECS)
    members, combo_off = ops.pack_combos([SPECS])
    d_lines = lines.cuda()
    d_match = {k: v.cuda() for k, v in match.items()}

    h = ops.watch_hashes(d_lines, d_match, specs.cuda()).cpu()
    assert torch.equal(h, ops.watch_hashes_cpu(lines, match, specs))
    assert torch.equal(h != 0, present)
    # the table of the issue, literally
    assert h[1, 0] != 0 and h[1, 1] != 0 and h[1, 2] == 0
    assert h[2, 0] == 0 and h[3, 0] == 0 and h[4, 1] == 0 and h[5, 4] == 0

    hc = ops.watch_combo_hashes(d_lines, d_match, specs.cuda(), members.cuda(),
                                combo_off.cuda()).cpu()
    assert torch.equal(
        hc, ops.watch_combo_hashes_cpu(lines, match, specs, members, combo_off))
    assert torch.equal(hc[:, :W], h)
    # every member is relevant on every line; an absent one contributes 0
    want = ops.combo_fold(torch.ones((B, W), dtype=torch.int64).numpy(), h.numpy())
    assert hc[:, W].tolist() == want.tolist()
    assert bool((hc[:, W] != 0).all())

    ranges = [dict(s, non_numeric="alert") for s in SPECS]
    cpu = ops.ValueRangeState(ranges, device="cpu")
    gpu = ops.ValueRangeState(ranges, device="cuda")
    want_code, want_value = cpu.step(lines, match, 0)
    code, value = gpu.step(d_lines, d_match, 0)
    assert torch.equal(code.cpu(), want_code)
    assert torch.equal(value.cpu().view(torch.int64), want_value.view(torch.int64))
    # letters are no number: 3 where the field is present, 0 where it is not
    assert torch.equal(code.cpu(), torch.where(present, 3, 0).to(torch.int32))
