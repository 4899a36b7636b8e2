"""The layered dense kernels (``fused_linear``, ``layernorm``, ``attention``,
``attention_qkv``) against the f64 references and the derived element-wise
bounds of dense_refs.py, at the smallest shapes that take each path (run on
an MI355X with `-m gpu`).

No fixed tolerance: every bound is u |ref| for the one bf16 rounding of the
output (u = 2^-8) plus gamma_n = n 2^-24 terms for the f32 arithmetic before
it; the derivations are in the ``*_bound`` docstrings of dense_refs.py.
Inputs carry per-row / per-column offsets, so that a transposed operand or a
tile stored in the wrong place is a gross error.
"""
import numpy as np
import pytest
import torch

import dense_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from detectmateservice_amd import ops

    assert ops.have_extension(), "HIP extension _dmx_C not built/loadable"
    yield


def _check(out, ref, bound, what):
    """out (bf16, GPU) within bound of ref, element-wise; names the worst."""
    o = out.double().cpu()
    assert o.shape == ref.shape, (o.shape, ref.shape)
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    excess = (o - ref).abs() - bound
    worst = int(excess.argmax())
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(ref.shape)))
    assert excess.max() <= 0, (
        f"{what}: element {idx} is {o[idx]:.6g}, reference {ref[idx]:.6g}, "
        f"bound {bound[idx]:.3g}; {int((excess > 0).sum())} of {ref.numel()} "
        f"elements out of bound")


# ---------------------------------------------------------------------------
# attention (VALU kernel: P stays f32)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("Dh", [8, 40, 64])
@pytest.mark.parametrize("S", [1, 7, 63, 64, 65, 127, 128])
def test_attention_valu(S, Dh):
    """S around the one-key-per-lane / two-keys-per-lane boundary and the
    rows-per-wave rounding, Dh below, between and at the vector widths.
    Bound: u |ref| + 2 ds (P |V|), dense_refs.attention_bound."""
    from detectmateservice_amd import ops

    for kind in ("sharp", "overflow"):
        q, k, v = R.attention_inputs(3, S, Dh, kind, seed=1000 * S + Dh)
        out = ops.attention(q.cuda(), k.cuda(), v.cuda())
        _check(out, R.ref_attention(q, k, v), R.attention_bound(q, k, v),
               f"attention {kind} S={S} Dh={Dh}")


# ---------------------------------------------------------------------------
# attention_qkv (MFMA kernel: P rounded to bf16)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("Dh", [32, 64])
@pytest.mark.parametrize("S", [32, 64, 96, 128])
@pytest.mark.parametrize("H", [1, 3])
def test_attention_qkv_mfma(H, S, Dh):
    """One and two query tiles per wave, one and two k-steps, an odd head
    count (row stride 3 H Dh). Bound: u (P |V| + |ref|) + 2 ds (P |V|)."""
    from detectmateservice_amd import ops

    B = 2
    for kind in ("sharp", "overflow"):
        qkv = R.qkv_inputs(B, S, H, Dh, kind, seed=100 * S + 10 * H + Dh)
        out = ops.attention_qkv(qkv.cuda(), S, H, Dh).double().cpu()
        ref = R.ref_attention_qkv(qkv, S, H, Dh)
        bound = R.attention_qkv_bound(qkv, S, H, Dh)
        assert out.shape == ref.shape == (B, S, H * Dh)
        assert torch.isfinite(out).all(), f"{kind}: non-finite output"
        excess = ((out - ref).abs() - bound).amax(-1)   # [B, S]: per query row
        err = (out - ref).abs().amax(-1)
        assert excess.max() <= 0, (
            f"attention_qkv {kind} H={H} S={S} Dh={Dh}: query rows out of bound "
            f"(batch, row, max error): "
            f"{[(int(b), int(s), float(err[b, s])) for b, s in (excess > 0).nonzero()]}; "
            f"per-row max error {err.tolist()}")


# ---------------------------------------------------------------------------
# layernorm
# ---------------------------------------------------------------------------


def _ln_rows(M, D, seed, special):
    """x, r [M, D] bf16: random rows with a per-row offset; with ``special``
    the last two rows (or the only one) are a constant row and a row of mean
    100 with values in {100, 100.5}."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) + torch.linspace(-3.0, 3.0, M)[:, None]
    r = torch.randn(M, D, generator=g) * 0.5
    if special in ("both", "constant"):
        x[-1], r[-1] = 1.5, -0.25          # x + r constant too
    if special in ("both", "mean100"):
        row = -2 if special == "both" else -1
        x[row] = 100.0 + 0.5 * torch.randint(0, 2, (D,), generator=g)
        r[row] = 0.0
    return x.bfloat16(), r.bfloat16()


@pytest.mark.parametrize("M", [1, 5, 33])
@pytest.mark.parametrize("D", [64, 128, 256, 512, 192, 320, 1024, 1536, 2048])
def test_layernorm(D, M):
    """D in {64, 128, 256, 512} is the row-group kernel, {192, 320} the
    wave-per-row kernel's strided path, {1024, 1536, 2048} its 8-wide vector
    path; M = 1, a partial block and a last block of one row; with and
    without residual and xres. Bound: u |y| + gamma_{D+4} (|v - mu| + |mu|)
    rstd |g| (dense_refs.layernorm_bound); xres must be bit-equal to
    bf16(x + r), and a constant row must give beta bit for bit."""
    from detectmateservice_amd import ops

    g = torch.Generator().manual_seed(D + M)
    gam = (torch.randn(D, generator=g) * 0.3 + 1.0).bfloat16()
    bet = (torch.randn(D, generator=g) * 0.5).bfloat16()
    specials = ("both",) if M >= 3 else ("none", "constant", "mean100")
    for special in specials:
        x, r = _ln_rows(M, D, seed=7 * D + M, special=special)
        for res in (r, None):
            for want_xres in (False, True):
                what = (f"layernorm D={D} M={M} rows={special} "
                        f"residual={res is not None} xres={want_xres}")
                out = ops.layernorm(x.cuda(), gam.cuda(), bet.cuda(),
                                    residual=None if res is None else res.cuda(),
                                    return_xres=want_xres)
                y = out[0] if want_xres else out
                ref, _ = R.ref_layernorm(x, gam, bet, res)
                _check(y, ref, R.layernorm_bound(x, gam, bet, res), what)
                if want_xres:
                    assert torch.equal(out[1].cpu(), R.xres_expected(x, res)), (
                        f"{what}: xres is not bf16(x + r)")
                if special in ("both", "constant"):
                    assert torch.equal(y[-1].cpu(), bet), (
                        f"{what}: constant row is not beta")


# ---------------------------------------------------------------------------
# fused_linear
# ---------------------------------------------------------------------------

LINEAR_SHAPES = [
    (1, 8, 64),          # one row, one partial tile, one K tile
    (129, 130, 64),      # 2 x 2 grid, one K tile (prefetch body skipped)
    (384, 384, 64),      # 9 workgroups: XCD swizzle q = 1, r = 1
    (300, 1100, 192),    # 27 workgroups: q = 3, r = 3; three K tiles (odd)
    (16, 128, 128),      # M = 16, two K tiles
]


@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES)
def test_fused_linear(M, N, K):
    """Every epilogue and the missing bias at each shape. Bound:
    u |act(ref)| + L gamma_{K+2} (|x| |w|^T + |b|), dense_refs.linear_bound."""
    from detectmateservice_amd import ops

    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * 0.5
         + torch.linspace(-1.0, 1.0, M)[:, None]).bfloat16()
    wt = (torch.randn(N, K, generator=g) * 0.1
          + torch.linspace(-0.25, 0.25, N)[:, None]).bfloat16()
    bias = torch.randn(N, generator=g)
    xg, wg, bg = x.cuda(), wt.cuda(), bias.cuda()
    for activation, b in (("none", bias), ("gelu", bias), ("relu", bias), ("none", None)):
        out = ops.fused_linear(xg, wg, None if b is None else bg, activation=activation)
        _check(out, R.ref_linear(x, wt, b, activation),
               R.linear_bound(x, wt, b, activation),
               f"fused_linear {M}x{N}x{K} {activation} bias={b is not None}")
