"""dmx_hashset_insert / dmx_hashset_probe on small tables, where probe
chains are long: keys that share a home slot, chains that wrap past the last
slot, the same key many times in one launch, keys with the top bit set, and
full and over-full tables. The tables are read back and checked against a
Python set per column; probes are compared with that set and with the CPU
``GpuHashSets``. Exact comparison."""
import random

import pytest
import torch

from detectmateservice_amd import ops
from kernel_refs import home_slot, keys_with_home

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_extension(), "HIP extension _dmx_C not built/loadable"
    yield


def _column_keys(rng, W, capacity, wrap):
    """capacity // 2 keys per column, all of one column on one home slot.
    Column 0's home is the last slot when ``wrap`` (the chain wraps to slot
    0), the columns' key sets are disjoint."""
    taken: set = set()
    homes = [(capacity - 1 if wrap else 2) if w == 0 else (3 * w) % capacity
             for w in range(W)]
    return homes, [keys_with_home(rng, capacity // 2, homes[w], capacity, taken)
                   for w in range(W)]


def _batch(rng, B, keys):
    """[B, W] int64: each column cycles through its keys (so a key repeats
    up to B / len(keys) times in the launch) with a zero, i.e. an absent
    field, in about every fifth cell. Shuffled rows."""
    W = len(keys)
    rows = [[0 if rng.random() < 0.2 else keys[w][i % len(keys[w])] for w in range(W)]
            for i in range(B)]
    rng.shuffle(rows)
    return torch.tensor(rows, dtype=torch.int64).view(B, W)


def _check_tables(tables, inserted, capacity):
    """Per table: the non-zero words are exactly the column's distinct
    non-zero keys, each once, and each reachable from its home slot."""
    tables = tables.cpu().tolist()
    for w, want in enumerate(inserted):
        words = [x for x in tables[w] if x != 0]
        assert len(words) == len(set(words)), (w, "a key is stored twice")
        assert set(words) == want, w
        for pos, key in enumerate(tables[w]):
            if key == 0:
                continue
            s = home_slot(key, capacity)
            while s != pos:
                assert tables[w][s] != 0, (w, key, "empty slot before the key")
                s = (s + 1) % capacity


def _expected_probe(hashes, sets):
    return [[1 if (v != 0 and v not in sets[w]) else 0 for w, v in enumerate(row)]
            for row in hashes.tolist()]


SHAPES = [  # capacity, W, B, wrap
    (8, 1, 1, False), (8, 1, 85, True), (8, 3, 86, True), (8, 3, 300, False),
    (16, 1, 300, True), (16, 3, 85, False), (16, 3, 86, True),
    (64, 1, 86, False), (64, 3, 1, True), (64, 3, 300, True),
]


@pytest.mark.parametrize("capacity,W,B,wrap", SHAPES)
def test_collisions_insert_readback_probe(capacity, W, B, wrap):
    rng = random.Random(capacity * 1000 + W * 100 + B)
    homes, keys = _column_keys(rng, W, capacity, wrap)
    hashes = _batch(rng, B, keys)
    inserted = [set(hashes[:, w].tolist()) - {0} for w in range(W)]
    gpu = ops.GpuHashSets(W, capacity, device="cuda")
    cpu = ops.GpuHashSets(W, capacity, device="cpu")
    gpu.insert(hashes.cuda())
    cpu.insert(hashes)
    _check_tables(gpu.tables, inserted, capacity)
    # column 0's keys were inserted in column 0 only
    for w in range(1, W):
        assert not (set(gpu.tables[w].cpu().tolist()) & set(keys[0]))

    # probe: zeros, every inserted key, and keys never inserted whose homes
    # lie before, at the start of, inside and just behind the cluster
    n = capacity // 2
    taken = {k for col in keys for k in col}
    rows = []
    for off in (-1, 0, 1, n - 1, n, n + 1):
        rows.append([keys_with_home(rng, 1, (homes[w] + off) % capacity, capacity, taken)[0]
                     for w in range(W)])
    probe = torch.cat([hashes, torch.zeros((1, W), dtype=torch.int64),
                       torch.tensor(rows, dtype=torch.int64).view(-1, W)])
    got = gpu.probe(probe.cuda()).cpu()
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(probe.shape)
    assert got.tolist() == _expected_probe(probe, inserted)
    assert got[: B].sum() == 0 and got[B].sum() == 0
    assert torch.equal(got, cpu.probe(probe))


@pytest.mark.parametrize("capacity,W", [(8, 3), (64, 1)])
def test_two_launches_equal_one(capacity, W):
    rng = random.Random(capacity + W)
    homes, keys = _column_keys(rng, W, capacity, True)
    hashes = _batch(rng, 300, keys)
    one = ops.GpuHashSets(W, capacity, device="cuda")
    one.insert(hashes.cuda())
    two = ops.GpuHashSets(W, capacity, device="cuda")
    two.insert(hashes[:180].cuda())
    two.insert(hashes[120:].cuda())          # overlaps the first launch
    inserted = [set(hashes[:, w].tolist()) - {0} for w in range(W)]
    _check_tables(one.tables, inserted, capacity)
    _check_tables(two.tables, inserted, capacity)
    taken = {k for col in keys for k in col}
    fresh = [[keys_with_home(rng, 1, (homes[w] + off) % capacity, capacity, taken)[0]
              for w in range(W)] for off in range(4)]
    probe = torch.cat([hashes, torch.tensor(fresh, dtype=torch.int64).view(-1, W)]).cuda()
    assert torch.equal(one.probe(probe), two.probe(probe))


@pytest.mark.parametrize("capacity", [8, 16, 64])
def test_exactly_full_table(capacity):
    """``capacity`` distinct keys: all are stored, each probes as known, and
    an absent key probes as unseen after a full circuit."""
    rng = random.Random(capacity)
    taken: set = set()
    keys = [keys_with_home(rng, 1, rng.randrange(capacity), capacity, taken)[0]
            for _ in range(capacity)]
    gpu = ops.GpuHashSets(1, capacity, device="cuda")
    gpu.insert(torch.tensor(keys, dtype=torch.int64).view(-1, 1).cuda())
    _check_tables(gpu.tables, [set(keys)], capacity)
    assert 0 not in gpu.tables.cpu().tolist()[0]
    absent = [keys_with_home(rng, 1, h, capacity, taken)[0] for h in (0, capacity - 1)]
    probe = torch.tensor(keys + absent, dtype=torch.int64).view(-1, 1)
    assert gpu.probe(probe.cuda()).cpu().flatten().tolist() == [0] * capacity + [1, 1]


@pytest.mark.parametrize("capacity", [8, 16, 64])
def test_over_full_table_drops(capacity):
    """``capacity + 5`` distinct keys: the table holds ``capacity`` of them,
    which ones is up to the scheduling; the dropped ones probe as unseen."""
    rng = random.Random(capacity + 5)
    taken: set = set()
    keys = [keys_with_home(rng, 1, rng.randrange(capacity), capacity, taken)[0]
            for _ in range(capacity + 5)]
    gpu = ops.GpuHashSets(1, capacity, device="cuda")
    gpu.insert(torch.tensor(keys, dtype=torch.int64).view(-1, 1).cuda())
    stored = gpu.tables.cpu().tolist()[0]
    assert len(set(stored)) == capacity and set(stored) <= set(keys)
    got = gpu.probe(torch.tensor(keys, dtype=torch.int64).view(-1, 1).cuda())
    assert got.cpu().flatten().tolist() == [0 if k in set(stored) else 1 for k in keys]


@pytest.mark.parametrize("capacity,W", [(16, 3)])
def test_checkpoint_between_devices(capacity, W):
    rng = random.Random(99)
    homes, keys = _column_keys(rng, W, capacity, True)
    hashes = _batch(rng, 85, keys)
    taken = {k for col in keys for k in col}
    fresh = [[keys_with_home(rng, 1, (homes[w] + off) % capacity, capacity, taken)[0]
              for w in range(W)] for off in range(capacity // 2 + 2)]
    probe = torch.cat([hashes, torch.tensor(fresh, dtype=torch.int64).view(-1, W)])
    inserted = [set(hashes[:, w].tolist()) - {0} for w in range(W)]
    want = _expected_probe(probe, inserted)

    gpu = ops.GpuHashSets(W, capacity, device="cuda")
    gpu.insert(hashes.cuda())
    cpu = ops.GpuHashSets(W, capacity, device="cpu")
    cpu.load_state_dict(gpu.state_dict())
    assert cpu.probe(probe).tolist() == want

    cpu2 = ops.GpuHashSets(W, capacity, device="cpu")
    cpu2.insert(hashes)
    gpu2 = ops.GpuHashSets(W, capacity, device="cuda")
    gpu2.load_state_dict(cpu2.state_dict())
    _check_tables(gpu2.tables, inserted, capacity)
    assert gpu2.probe(probe.cuda()).cpu().tolist() == want
