"""Event-rate windows on the GPU: the two HIP kernels against the CPU mirror
(ops.event_rate_step_cpu), and the stage inside GpuPipeline on cuda, eager and
as a captured graph with a partial replay, against the same pipeline on CPU.

Integer outputs and the baseline (mean, var, known) must be equal to the bit:
the roll is compiled with contraction off and does one rounding per operation
like the mirror. rate_z goes through a device sqrt and division, whose last
bit is not asserted: 1e-12 relative."""
import random

import pytest
import torch

from detectmateservice_amd import ops
from detectmateservice_amd.pipeline import GpuPipeline, PipelineConfig

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1
PARAMS = dict(window_lines=None, ewma_alpha=0.3, z_threshold=2.0, min_windows=1)


def _bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _assert_same_state(gpu, cpu):
    sg, sc = gpu.state_dict(), cpu.state_dict()
    for k in ops.EventRateState._STATE:
        assert torch.equal(_bits(sg[k]), _bits(sc[k])), k


def _assert_same_out(og, oc, where):
    for k in ("rate_counts", "rate_hits", "rate_slot"):
        assert torch.equal(og[k].cpu(), oc[k]), (k, where)
    zg, zc = og["rate_z"].cpu(), oc["rate_z"]
    assert torch.equal(zg == 0, zc == 0), where
    torch.testing.assert_close(zg, zc, rtol=1e-12, atol=0)


def _ids(rng, B, T):
    """Rows drawn from {-1, 1 .. T} and, so that the single bin of E = 1
    swings too, 0 (which counts nowhere), with weights redrawn every 40
    rows: counts swing between windows and bins get flagged. Plus a few
    T + 1 and INT32_MAX rows, which count nowhere either."""
    values = [-1, 0] + list(range(1, min(T, 6) + 1)) + ([T] if T > 6 else [])
    ids = []
    while len(ids) < B:
        weights = [rng.random() ** 3 + 0.01 for _ in values]
        ids.extend(rng.choices(values, weights, k=min(40, B - len(ids))))
    for bad in (T + 1, INT32_MAX):
        if rng.random() < 0.7:
            ids[rng.randrange(B)] = bad
    return torch.tensor(ids, dtype=torch.int32)


# (B, L, calls, phase the stream starts in)
SHAPES = [
    (1, 1, 2, 0),        # every line a window
    (1, 3, 7, 0),        # a window spans calls
    (300, 1000, 5, 0),   # L > B: most calls complete nothing
    (1024, 7, 2, 5),     # many windows per call, open window carried in
    (256, 64, 2, 0),     # a window ends exactly on the batch end
    (257, 64, 2, 0),     # ... and one line later
]


@pytest.mark.parametrize("E", [1, 2, 257, ops.ER_MAX_EVENTS])
@pytest.mark.parametrize("B,L,calls,phase", SHAPES)
def test_kernels_match_mirror(B, L, calls, phase, E):
    T = E - 1
    rng = random.Random(B * 1000003 + L * 101 + E)
    kw = dict(PARAMS, window_lines=L)
    gpu = ops.EventRateState(T, device="cuda", **kw)
    cpu = ops.EventRateState(T, device="cpu", **kw)
    if phase:
        start = cpu.state_dict()
        start["ctl"][0] = phase
        start["open_counts"][0] = phase
        cpu.load_state_dict(start)
        gpu.load_state_dict(start)
    n_valid_set = sorted({0, 1, B - 1, B})
    flagged = 0
    step = 0
    for call in range(calls):
        for n_valid in reversed(n_valid_set):
            ids = _ids(rng, B, T)
            p = int(cpu.ctl[0])
            first_boundary = L - p - 1
            train_upto = (0, first_boundary if first_boundary < n_valid else 0,
                          B)[step % 3]
            step += 1
            oc = cpu.step(ids, n_valid=n_valid, train_upto=train_upto)
            og = gpu.step(ids.cuda(), n_valid=n_valid, train_upto=train_upto)
            _assert_same_out(og, oc, (call, n_valid, train_upto))
            _assert_same_state(gpu, cpu)
            flagged += int(oc["rate_hits"].sum())
    if (B, L) == (1024, 7):
        assert flagged > 0, "the case must exercise flagged bins"


def test_n_valid_zero_rewrites_state_bit_for_bit():
    gpu = ops.EventRateState(5, device="cuda", **dict(PARAMS, window_lines=10))
    rng = random.Random(3)
    gpu.step(_ids(rng, 37, 5).cuda())
    before = gpu.state_dict()
    out = gpu.step(_ids(rng, 37, 5).cuda(), n_valid=0)
    after = gpu.state_dict()
    assert before["ctl"].tolist() == [7, 3]
    for k in ops.EventRateState._STATE:
        assert torch.equal(_bits(before[k]), _bits(after[k])), k
    assert not out["rate_hits"].any() and bool((out["rate_slot"] == -1).all())


# ---------------------------------------------------------------------------
# pipeline: cuda (eager, then captured graph with a partial replay) against CPU
# ---------------------------------------------------------------------------

TEMPLATES = ["alpha <*>", "beta <*>", "gamma <*>", "delta <*>"]
STEADY = {"alpha": 8, "beta": 6, "gamma": 4, "zzz": 2}


def _log_lines(n_windows):
    lines = []
    for w in range(n_windows):
        c = dict(STEADY)
        if w % 12 == 6:
            c.update(alpha=2, beta=16, gamma=0)
        if w % 12 >= 9:
            c.update(gamma=0, alpha=12)
        if w % 12 == 8:
            c.update(alpha=6, delta=2)
        words = [k for k, n in c.items() for _ in range(n)]
        random.Random(w).shuffle(words)
        lines.extend(f"{word} v{w}".encode() for word in words)
    return lines


def test_pipeline_cuda_matches_cpu_eager_graph_partial():
    G = 256
    sizes = [G, G] + [G, G, 100, G, G, G]  # two eager, six replays
    lines = _log_lines(sum(sizes) // 20 + 1)
    cfg = dict(templates=TEMPLATES, use_transformer=False, max_len=32,
               train_lines=300, event_rate={"window_lines": 20, "min_windows": 2})
    dev = GpuPipeline(PipelineConfig(**cfg), device="cuda")
    ref = GpuPipeline(PipelineConfig(**cfg), device="cpu")

    def compare(got, want, n, where):
        for k in ("rate_hits", "rate_slot", "anomaly", "event_id"):
            assert got[k].shape[0] == n, (k, where)
            assert torch.equal(got[k].cpu(), want[k]), (k, where)
        rows = want["rate_counts"].shape[0]  # a partial replay has more slots
        assert torch.equal(got["rate_counts"].cpu()[:rows], want["rate_counts"])
        zg, zc = got["rate_z"].cpu()[:rows], want["rate_z"]
        assert torch.equal(zg == 0, zc == 0), where
        torch.testing.assert_close(zg, zc, rtol=1e-12, atol=0)

    at = 0
    total_hits = 0
    for j, n in enumerate(sizes):
        packed = ops.pack_lines(lines[at:at + n], 32)
        at += n
        want = ref.process_packed(*packed)
        dl, dn = packed[0].cuda(), packed[1].cuda()
        if j < 2:
            got = dev.process_packed(dl, dn)
        else:
            if j == 2:
                before = dev.event_rate.state_dict()
                assert dev.enable_graph(G)
                after = dev.event_rate.state_dict()
                for k in ops.EventRateState._STATE:
                    assert torch.equal(_bits(before[k]), _bits(after[k])), k
            got = (dev.process_packed_graph(dl, dn) if n == G
                   else dev.process_packed_graph_partial(dl, dn))
        compare(got, want, n, j)
        _assert_same_state(dev.event_rate, ref.event_rate)
        total_hits += int(want["rate_hits"].sum())
    assert dev.seen_lines == ref.seen_lines == sum(sizes)
    assert total_hits > 0
    # 7 * 256 + 100 = 1892 = 94 * 20 + 12: pad rows of the partial replay
    # were not counted
    assert ref.event_rate.ctl.tolist() == [12, 94]
