"""The fused BERT kernel against the f64 reference of dense_refs.py at three
scales of weights (run on an MI355X with `-m gpu`).

At the scale of the older tests (``small``) the attention logits stay below
0.3, the softmax is uniform to 2% and whole phases of the kernel have no
visible effect. ``sharp`` gives logits of up to 12 and a peaked softmax,
``tiny`` a LayerNorm input whose variance is within sight of eps. The bound
is not a constant: it is twice ``E_chain``, the distance between the
reference and the same reference rounded to bf16 where the kernel stores
bf16, computed for the test's own batch. tests/test_dense_refs_cpu.py checks
that every wrong variant of the reference moves the result by at least three
times that bound in one of the regimes.
"""
import functools

import pytest
import torch

import dense_refs as R

pytestmark = pytest.mark.gpu

H = 128


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from detectmateservice_amd import ops

    assert ops.have_extension(), "HIP extension _dmx_C not built/loadable"
    yield


@functools.lru_cache(maxsize=None)
def _case(regime, layers, B):
    """(gpu model, batch on the GPU, reference hidden states, reference
    scores, E_chain pooled, E_chain score), computed once per case."""
    seed = R.fused_model_seed(layers)
    cpu = R.regime_model(layers, seed, regime, "cpu")
    gpu = R.regime_model(layers, seed, regime, "cuda")
    for k, t in cpu.state_dict().items():
        assert torch.equal(gpu.state_dict()[k], t), f"{k} differs between devices"
    assert gpu._fused_ok()
    batch = R.fused_batch(B)
    ref, e_emb, e_score = R.e_chain(cpu, batch)
    assert torch.isfinite(ref).all()
    return gpu, tuple(t.cuda() for t in batch), ref, R.ref_score(cpu, ref), e_emb, e_score


@pytest.mark.parametrize("B", R.FUSED_BATCH_ROWS)
@pytest.mark.parametrize("layers", R.FUSED_LAYERS)
@pytest.mark.parametrize("regime", R.REGIMES)
def test_fused_against_f64_reference(regime, layers, B):
    """max |emb - ref.mean(1)| <= 2 E_chain, and the same for the score with
    E_chain taken on the score.

    E_chain is what the kernel's bf16 storage costs when everything between
    two stores is exact. The factor 2 is for what the chain model cannot
    reproduce: f32 accumulation in another order, __expf, v_rcp and rsqrtf
    move a value by about 1e-6 relative before a bf16 rounding, which can
    flip that rounding and turn a half-ulp error into a full ulp.

    Measured E_fused / E_chain on an MI355X (pooled embedding | score), B = 22:

        layers   small         sharp         tiny
        1        1.00 | 1.00   1.00 | 0.88   1.00 | 1.00
        2        1.00 | 1.00   0.94 | 1.07   1.00 | 1.00
        4        1.00 | 1.00   0.80 | 1.25   1.00 | 0.96

    At B = 1 the largest are 1.14 (sharp, 2 layers, embedding) and 1.05
    (small, 2 layers, score). A ratio of 1.00 means the kernel and the chain
    model round the same way everywhere. Before the second FFN half was made
    to read the LN1 output (it read x after the first half's W2 update) the
    same table read 2.2 - 2.5 in small at 1 and 2 layers and 350 - 530 in
    sharp.
    """
    gpu, (lines, start, end), ref, ref_score, e_emb, e_score = _case(regime, layers, B)
    emb = gpu.embed_spans(lines, start, end).double().cpu()
    score = gpu.score_spans(lines, start, end).double().cpu()
    assert emb.shape == (B, H) and score.shape == (B,)
    assert torch.isfinite(emb).all() and torch.isfinite(score).all()
    err_emb = (emb - ref.mean(1)).abs()
    err_score = (score - ref_score).abs()
    print(f"RATIO {regime} layers={layers} B={B}: "
          f"emb {err_emb.max():.3e} / E_chain {e_emb:.3e} = {err_emb.max() / e_emb:.2f} | "
          f"score {err_score.max():.3e} / E_chain {e_score:.3e} = {err_score.max() / e_score:.2f}")
    row, col = divmod(int(err_emb.argmax()), H)
    assert err_emb.max() <= R.FUSED_FACTOR * e_emb, (
        f"pooled embedding: line {row} column {col} off by {err_emb.max():.3e}, "
        f"bound 2 x {e_emb:.3e}; per-line max {err_emb.amax(1).tolist()}")
    assert err_score.max() <= R.FUSED_FACTOR * e_score, (
        f"score: line {int(err_score.argmax())} off by {err_score.max():.3e}, "
        f"bound 2 x {e_score:.3e}")


@pytest.mark.parametrize("layers", R.FUSED_LAYERS)
def test_sharp_output_is_not_an_average(layers):
    """So that a stuck row or column cannot hide in a max norm: the kernel's
    output is further from the reference's ``uniform`` variant (softmax
    replaced by an average) than the bound, and the all-padding line differs
    from a full line in most columns."""
    from test_bert_fused_epilogue import EDGE_SPANS

    gpu, (lines, start, end), ref, _, e_emb, _ = _case("sharp", layers, 22)
    bound = R.FUSED_FACTOR * e_emb
    emb = gpu.embed_spans(lines, start, end).double().cpu()
    cpu = R.regime_model(layers, R.fused_model_seed(layers), "sharp")
    uniform = R.ref_bert(cpu, R.fused_batch(22), mutant="uniform").mean(1)
    away = (emb - uniform).abs().amax(1)
    print(f"layers={layers}: distance from the uniform variant, per line, in "
          f"bounds: {(away / bound).tolist()}")
    assert away.max() > bound
    pad, full = EDGE_SPANS.index((0, 0)), EDGE_SPANS.index((0, 64))
    assert int(end[pad]) == 0 and int(end[full] - start[full]) == 64
    differs = (emb[pad] - emb[full]).abs() > bound
    assert int(differs.sum()) > H // 2, f"only {int(differs.sum())} columns differ"


def test_sharp_distance_head():
    """embed_distance_spans against the formula on the kernel's own emb,
    rtol 1e-4 as in test_distance_formula."""
    gpu, (lines, start, end), ref, _, _, _ = _case("sharp", 2, 22)
    g = torch.Generator().manual_seed(9)
    mu = (ref.mean(1).mean(0).float() + torch.randn(H, generator=g) * 0.1).cuda()
    inv_var = (10.0 ** (torch.rand(H, generator=g) + 1.0)).cuda()
    dist, emb = gpu.embed_distance_spans(lines, start, end, mu, inv_var, return_emb=True)
    assert torch.equal(emb, gpu.embed_spans(lines, start, end))
    expect = ((emb.double() - mu.double()) ** 2 * inv_var.double()).mean(1).sqrt()
    torch.testing.assert_close(dist.double(), expect, rtol=1e-4, atol=0.0)
    assert torch.equal(gpu.embed_distance_spans(lines, start, end, mu, inv_var), dist)
