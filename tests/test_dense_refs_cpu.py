"""Reference-only conditions of the dense-kernel tests (no GPU, no extension):
the f64 references of dense_refs.py agree with torch's own operators, the
bf16 chain model reduces to the reference when its roundings are off, and
every wrong variant ("mutant") of the references would turn an assertion of
the GPU tests red on exactly the batch, seeds and regimes those tests use. A
later edit that quietly disarms a GPU test (a smaller gain, another seed, a
wider bound) fails here first.

Known limit: the erf form of GELU differs from the tanh form by less than
5e-4, below the bf16 storage error of the FFN output, so "erf where tanh
belongs" is not among the mutants: no test at bf16 can kill it.
"""
import math

import pytest
import torch

import dense_refs as R
from dense_refs import FUSED_BATCH_ROWS as BATCH_ROWS
from dense_refs import FUSED_LAYERS as LAYERS
from dense_refs import fused_batch as batch_for
from dense_refs import fused_model_seed as model_seed

# ---------------------------------------------------------------------------
# the references against torch's own operators
# ---------------------------------------------------------------------------


def test_layered_refs_agree_with_torch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(9, 192, generator=g).bfloat16()
    r = torch.randn(9, 192, generator=g).bfloat16()
    w = torch.randn(40, 192, generator=g).bfloat16()
    b = torch.randn(40, generator=g)
    gam = torch.randn(192, generator=g).bfloat16()
    bet = torch.randn(192, generator=g).bfloat16()
    F = torch.nn.functional
    lin = F.linear(x.double(), w.double(), b.double())
    torch.testing.assert_close(R.ref_linear(x, w, b), lin, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(R.ref_linear(x, w, b, "gelu"),
                               F.gelu(lin, approximate="tanh"), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(R.ref_linear(x, w, None, "relu"),
                               F.linear(x.double(), w.double()).relu(),
                               rtol=1e-13, atol=1e-13)
    y, xres = R.ref_layernorm(x, gam, bet, r)
    v = x.double() + r.double()
    torch.testing.assert_close(
        y, F.layer_norm(v, (192,), gam.double(), bet.double(), 1e-5),
        rtol=1e-12, atol=1e-12)
    assert torch.equal(xres, v)
    q, k, vv = R.attention_inputs(3, 7, 8, "sharp", seed=2)
    sdpa = F.scaled_dot_product_attention(q.double(), k.double(), vv.double())
    torch.testing.assert_close(R.ref_attention(q, k, vv), sdpa, rtol=1e-12, atol=1e-12)
    # the packed layout is the one the model's qkv projection emits
    qkv = R.qkv_inputs(2, 32, 3, 32, "sharp", seed=3)
    q, k, vv = R.split_qkv(qkv, 32, 3, 32)
    assert torch.equal(q[4], qkv[1, :, 32:64])          # b=1, h=1: q
    assert torch.equal(k[4], qkv[1, :, 96 + 32:96 + 64])
    assert torch.equal(vv[4], qkv[1, :, 192 + 32:192 + 64])
    out = R.ref_attention_qkv(qkv, 32, 3, 32)
    assert torch.equal(out[1, :, 32:64], R.ref_attention(q, k, vv)[4])


def _torch_bert(model, tokens):
    """The model written with torch's own layer_norm / softmax / gelu, one
    FFN matmul instead of two halves: an independent spelling of ref_bert."""
    F = torch.nn.functional
    d = lambda t: t.double()  # noqa: E731
    B, S = tokens.shape
    x = d(model.tok_emb)[tokens] + d(model.pos_emb)[:S]
    for L in model.layers:
        qkv = F.linear(x, d(L["wqkv_t"]), d(L["bqkv"]))
        q, k, v = (t.reshape(B, S, 2, 64).transpose(1, 2) for t in qkv.chunk(3, -1))
        a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, S, 128)
        x = F.layer_norm(x + F.linear(a, d(L["wo_t"]), d(L["bo"])), (128,),
                         d(L["ln1_g"]), d(L["ln1_b"]), 1e-5)
        h = F.gelu(F.linear(x, d(L["w1_t"]), d(L["b1"])), approximate="tanh")
        x = F.layer_norm(x + F.linear(h, d(L["w2_t"]), d(L["b2"])), (128,),
                         d(L["ln2_g"]), d(L["ln2_b"]), 1e-5)
    return x


@pytest.mark.parametrize("regime", R.REGIMES)
def test_ref_bert_agrees_with_torch_and_chain_off_is_exact(regime):
    model = R.regime_model(2, model_seed(2), regime)
    batch = batch_for(22)
    tokens = R.span_tokens(*batch)
    # the oracle's tokenizer against the model's
    assert torch.equal(tokens, model.tokenize_spans(*batch))
    ref = R.ref_bert(model, tokens)
    assert ref.dtype == torch.float64 and ref.shape == (22, 64, 128)
    torch.testing.assert_close(ref, _torch_bert(model, tokens), rtol=1e-10, atol=1e-10)
    assert torch.equal(R.ref_bert(model, batch), ref)
    # the chain model with every rounding switched off IS the reference
    assert torch.equal(R.ref_bert(model, tokens, chain=True, points=()), ref)
    # and each rounding point on its own moves the result
    for point in R.CHAIN_POINTS:
        one = R.ref_bert(model, tokens, chain=True, points=(point,))
        assert not torch.equal(one, ref), point


def test_regimes_are_what_they_claim():
    """sharp has a peaked softmax and logits of several units, small is
    uniform to a few percent, tiny puts a variance of about 15 eps into LN1
    of layer 0 (1/7 of the eps mutant's 1e-3)."""
    tokens = R.span_tokens(*batch_for(22))

    def layer0(regime):
        m = R.regime_model(2, model_seed(2), regime)
        L = {k: R.f64(t) for k, t in m.layers[0].items()}
        x = R.bf16_round(R.f64(m.tok_emb)[tokens] + R.f64(m.pos_emb)[:64])
        qkv = x @ L["wqkv_t"].T + L["bqkv"]
        q, k, v = (t.reshape(22, 64, 2, 64).transpose(1, 2) for t in qkv.split(128, -1))
        s = q @ k.transpose(-1, -2) / 8.0
        p = torch.softmax(s, -1)
        a = (p @ v).transpose(1, 2).reshape(22, 64, 128)
        pre_ln1 = x + a @ L["wo_t"].T + L["bo"]
        return s.abs().max().item(), p.amax(-1).median().item(), pre_ln1.var(-1, unbiased=False)

    smax, pmed, _ = layer0("small")
    assert smax < 0.01 and pmed < 1.05 / 64
    smax, pmed, _ = layer0("sharp")
    print(f"sharp layer 0: max |s| {smax:.2f}, median max p {pmed:.3f}")
    assert smax > 8.0 and pmed > 0.2
    _, _, var = layer0("tiny")
    print(f"tiny pre-LN1 variance: {var.min():.2e} .. {var.max():.2e}")
    # within sight of eps = 1e-5 and below the 1e-3 of the ``eps`` mutant
    assert var.max() < 1e-3 and var.max() < 20 * R.EPS


# ---------------------------------------------------------------------------
# every fused mutant dies in some regime, at every layer count
# ---------------------------------------------------------------------------

#: the regime whose GPU test kills the mutant (measured in units of E_chain
#: at 2 layers: sharp uniform 121, exp2 54, droplast 13, swapheads 224,
#: sum16 351, noattn 457, bias_shift 37, relu 92, half1 836, b2twice 23,
#: start+1 120; tiny eps 26; the margin asked for is 6)
KILLED_IN = {m: "sharp" for m in R.MUTANTS}
KILLED_IN["eps"] = "tiny"


@pytest.mark.parametrize("layers", LAYERS)
def test_every_fused_mutant_is_killed(layers):
    batch = batch_for(max(BATCH_ROWS))
    cache = {}
    for mutant in R.MUTANTS:
        regime = KILLED_IN[mutant]
        if regime not in cache:
            model = R.regime_model(layers, model_seed(layers), regime)
            cache[regime] = (model,) + R.e_chain(model, batch)
        model, ref, e_emb, _ = cache[regime]
        moved = (R.ref_bert(model, batch, mutant=mutant).mean(1) - ref.mean(1)).abs().max().item()
        need = R.KILL_MARGIN * R.FUSED_FACTOR * e_emb
        print(f"layers={layers} {regime:5s} {mutant:10s}: {moved / e_emb:7.1f} x E_chain")
        assert moved >= need, (mutant, regime, moved, need)


def test_softmax_mutants_survive_the_small_regime():
    """Why the regimes exist: at the scale of the older tests the five
    softmax mutants stay inside the bound, so those tests cannot see them."""
    model = R.regime_model(2, model_seed(2), "small")
    batch = batch_for(22)
    ref, e_emb, _ = R.e_chain(model, batch)
    for mutant in ("uniform", "exp2", "droplast", "swapheads"):
        moved = (R.ref_bert(model, batch, mutant=mutant).mean(1) - ref.mean(1)).abs().max().item()
        assert moved < R.FUSED_FACTOR * e_emb, (mutant, moved, e_emb)


def test_sharp_padding_row_differs_from_full_row():
    """The reference-side twin of the GPU assertion: the all-padding line and
    the full line differ by the kill margin in most columns."""
    for layers in LAYERS:
        model = R.regime_model(layers, model_seed(layers), "sharp")
        ref, e_emb, _ = R.e_chain(model, batch_for(22))
        emb = ref.mean(1)
        far = (emb[1] - emb[3]).abs() > R.KILL_MARGIN * R.FUSED_FACTOR * e_emb
        assert int(far.sum()) > 64, (layers, int(far.sum()))


# ---------------------------------------------------------------------------
# attention mutants against the derived bound
# ---------------------------------------------------------------------------

ATTN_SHAPES = [(3, 64, 64), (3, 128, 64), (3, 65, 40), (3, 7, 8)]


@pytest.mark.parametrize("BH,S,Dh", ATTN_SHAPES)
def test_attention_mutants_exceed_the_bound_on_sharp_inputs(BH, S, Dh):
    q, k, v = R.attention_inputs(BH, S, Dh, "sharp", seed=S + Dh)
    ref = R.ref_attention(q, k, v)
    # the looser of the two bounds (MFMA)
    bound = R.attention_bound(q, k, v, p_bf16=True)
    print(f"S={S} Dh={Dh}: bound max {bound.max():.4f}")
    for mutant in ("uniform", "exp2", "droplast"):
        err = (R.ref_attention(q, k, v, mutant=mutant) - ref).abs()
        over = (err - R.KILL_MARGIN * bound).max().item()
        print(f"  {mutant}: max err {err.max():.3f}")
        assert over > 0, (mutant, err.max().item())
    # a model of the MFMA kernel's two roundings stays inside the bound
    s = R.f64(q) @ R.f64(k).transpose(-1, -2) / math.sqrt(Dh)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    model = R.bf16_round((R.bf16_round(e) @ R.f64(v)) / e.sum(-1, keepdim=True))
    assert ((model - ref).abs() <= bound).all()


def test_attention_nomax_overflows_on_overflow_inputs():
    q, k, v = R.attention_inputs(3, 64, 64, "overflow", seed=5)
    assert torch.isfinite(R.ref_attention(q, k, v)).all()
    assert not torch.isfinite(R.ref_attention(q, k, v, mutant="nomax")).all()


@pytest.mark.parametrize("S", [64, 128])
def test_attention_mutants_pass_the_old_bound_on_small_inputs(S):
    """The inputs of test_attention_vs_torch (seed 4, BH = 12, Dh = 64,
    randn * 0.5) and its fixed 0.03: ``exp2`` stays within it at both
    lengths, ``droplast`` at S = 128, ``nomax`` cannot overflow. The derived
    bound sees the first two."""
    g = torch.Generator().manual_seed(4)
    q, k, v = ((torch.randn(12, S, 64, generator=g) * 0.5).bfloat16() for _ in range(3))
    ref = R.ref_attention(q, k, v)
    survivors = ("exp2", "droplast", "nomax") if S == 128 else ("exp2", "nomax")
    for mutant in survivors:
        err = (R.ref_attention(q, k, v, mutant=mutant) - ref).abs().max().item()
        print(f"S={S} {mutant}: {err:.4f}")
        assert err < 0.03, (mutant, err)
    bound = R.attention_bound(q, k, v, p_bf16=True)
    for mutant in ("exp2", "droplast"):
        err = (R.ref_attention(q, k, v, mutant=mutant) - ref).abs()
        assert (err - R.KILL_MARGIN * bound).max() > 0, mutant
