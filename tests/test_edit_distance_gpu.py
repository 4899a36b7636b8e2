"""dmx_edit_distance against the two-row DP of kernel_refs.py at the lengths
where the wavefront changes shape: 0, 1, 2, the lane strides 63/64/65 and
127/128/129, 255 and ED_MAX_LEN = 256; structured pairs with known
distances; one-row batches; rows narrower than ED_MAX_LEN with length words
that exceed the row or are negative. Exact comparison."""
import random

import pytest
import torch

from detectmateservice_amd import ops
from kernel_refs import levenshtein, pack_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_extension(), "HIP extension _dmx_C not built/loadable"
    yield


LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256]
ALPHABETS = {"ab": b"ab", "forty": bytes(range(48, 88))}


def _rand(rng, alphabet, n):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _kernel(a, a_len, b, b_len):
    return ops._C.edit_distance(a.cuda(), a_len.cuda(), b.cuda(), b_len.cuda()).cpu()


def _expect(a_strs, b_strs, got, cells=None):
    """Every cell of ``got`` (or the listed ones) equals the reference."""
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(a_strs), len(b_strs))
    if cells is None:
        cells = [(i, j) for i in range(len(a_strs)) for j in range(len(b_strs))]
    got = got.tolist()
    for i, j in cells:
        assert got[i][j] == levenshtein(a_strs[i], b_strs[j]), (
            i, j, len(a_strs[i]), len(b_strs[j]))


@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_all_pairs_of_edge_lengths(alphabet):
    """11 x 11 = 121 pairs, so the last workgroup of four holds one pair."""
    rng = random.Random(len(alphabet))
    a_strs = [_rand(rng, ALPHABETS[alphabet], n) for n in LENGTHS]
    b_strs = [_rand(rng, ALPHABETS[alphabet], n) for n in LENGTHS]
    _expect(a_strs, b_strs, _kernel(*pack_rows(a_strs, 256), *pack_rows(b_strs, 256)))


@pytest.mark.parametrize("n", [65, 256])
def test_structured_pairs(n):
    rng = random.Random(n)
    s = _rand(rng, b"abcdefgh", n)

    def sub(k):
        return s[:k] + (b"z") + s[k + 1:]

    pairs = [
        (s, s, 0),
        (s, sub(0), 1), (s, sub(n // 2), 1), (s, sub(n - 1), 1),
        (s, s[1:] + b"z", None),         # shifted by one
        (s, s[: n // 2], n - n // 2),    # against its prefix
        (b"a" * n, b"b" * n, n),         # the maximum
    ]
    a_strs = [p[0] for p in pairs]
    b_strs = [p[1] for p in pairs]
    got = _kernel(*pack_rows(a_strs, 256), *pack_rows(b_strs, 256))
    # the launch computes all 49 cells; the reference is run on the seven
    # pairs and on one row and one column of the rest
    k = len(pairs)
    _expect(a_strs, b_strs, got,
            [(i, i) for i in range(k)] + [(0, j) for j in range(k)] + [(i, 6) for i in range(k)])
    for i, (_, _, d) in enumerate(pairs):
        if d is not None:
            assert int(got[i, i]) == d, i
    assert int(got[4, 4]) <= 2


@pytest.mark.parametrize("Na,Nb", [(1, 1), (1, 5), (5, 1)])
def test_one_row_batches(Na, Nb):
    rng = random.Random(10 * Na + Nb)
    a_strs = [_rand(rng, b"abc", rng.choice([64, 129, 256])) for _ in range(Na)]
    b_strs = [_rand(rng, b"abc", rng.choice([63, 128, 255])) for _ in range(Nb)]
    _expect(a_strs, b_strs, _kernel(*pack_rows(a_strs, 256), *pack_rows(b_strs, 256)))


@pytest.mark.parametrize("max_len", [64, 100])
def test_narrow_rows_and_hostile_length_words(max_len):
    """Rows of max_len < ED_MAX_LEN bytes. A length word of 200 reads as
    max_len and one of -3 as 0: the kernel clamps to [0, min(max_len,
    ED_MAX_LEN)] (kernels.h). Each over-long row has at least four rows
    behind it, so that even a kernel that took 200 for the length would read
    inside the tensor and fail here by value."""
    rng = random.Random(max_len)
    lengths = [0, 1, 2, 63, 64, max_len - 1, max_len, max_len, 5, max_len, 17, max_len]
    alphabet = b"abcd"
    # every row is filled to max_len: the bytes behind a length are text too
    a_rows = [_rand(rng, alphabet, max_len) for _ in lengths]
    b_rows = [_rand(rng, alphabet, max_len) for _ in lengths]
    a_words, b_words = list(lengths), list(lengths[::-1])
    long_a, long_b, neg_a = 6, 5, 3
    assert len(lengths) - 1 - max(long_a, long_b) >= 4
    a_words[long_a], b_words[long_b], a_words[neg_a] = 200, 200, -3
    a = torch.frombuffer(bytearray(b"".join(a_rows)), dtype=torch.uint8).view(-1, max_len).clone()
    b = torch.frombuffer(bytearray(b"".join(b_rows)), dtype=torch.uint8).view(-1, max_len).clone()
    got = _kernel(a, torch.tensor(a_words, dtype=torch.int32),
                  b, torch.tensor(b_words, dtype=torch.int32))
    a_strs = [r[: min(max(w, 0), max_len)] for r, w in zip(a_rows, a_words)]
    b_strs = [r[: min(max(w, 0), max_len)] for r, w in zip(b_rows, b_words)]
    assert len(a_strs[long_a]) == max_len and len(b_strs[long_b]) == max_len
    assert a_strs[neg_a] == b""
    _expect(a_strs, b_strs, got)
