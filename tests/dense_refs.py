"""Plain float64 references, derived error bounds and wrong variants for the
floating-point kernels: ``fused_linear``, ``layernorm``, ``attention``,
``attention_qkv`` and the fused BERT kernel. Nothing here imports from
``detectmateservice_amd.ops``: the CPU branches there are implementations,
this module is the oracle.

* ``ref_linear`` / ``ref_layernorm`` / ``ref_attention`` /
  ``ref_attention_qkv`` take the kernels' bf16 inputs, upcast them to f64 and
  return f64; the ``*_bound`` functions give the element-wise error a correct
  kernel may show (derivations in their docstrings).
* ``ref_bert`` is the whole model in f64. With ``chain=True`` it rounds to
  bf16 exactly where ``bert_fused.hip`` does and nowhere else; the distance
  between the two is the yardstick of the fused tests (``e_chain``).
* ``MUTANTS`` / ``ATTENTION_MUTANTS`` name deliberately wrong variants of the
  references. They are variants of the reference: nothing mutates or
  inspects a kernel. ``tests/test_dense_refs_cpu.py`` checks that every one
  of them would turn a GPU assertion red.
* ``regime_model`` builds the model at three scales of weights, bit-identical
  on every device.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

#: bf16 unit roundoff (8 significant bits, round to nearest even)
U = 2.0 ** -8
#: fused bound = FUSED_FACTOR * E_chain; a mutant is killed at KILL_MARGIN *
#: that bound
FUSED_FACTOR = 2.0
KILL_MARGIN = 3.0

S_FUSED = 64
EPS = 1e-5


def gamma(n: int) -> float:
    """n f32 roundings in a row: n * 2^-24."""
    return n * 2.0 ** -24


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().double()


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """f64 -> f32 -> bf16 (both to nearest even) -> f64: what a kernel that
    holds the value in an f32 register and stores it as bf16 does."""
    return t.float().bfloat16().double()


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    c = math.sqrt(2.0 / math.pi)
    return 0.5 * x * (1.0 + torch.tanh(c * (x + 0.044715 * x ** 3)))


# ---------------------------------------------------------------------------
# fused_linear
# ---------------------------------------------------------------------------

#: Lipschitz constant of the activation: sup |gelu_tanh'| = 1.129 at x = 1.41
ACT_LIPSCHITZ = {"none": 1.0, "relu": 1.0, "gelu": 1.13}


def _act(y: torch.Tensor, activation: str) -> torch.Tensor:
    if activation == "gelu":
        return gelu_tanh(y)
    if activation == "relu":
        return torch.relu(y)
    assert activation == "none", activation
    return y


def ref_linear(x, wt, bias=None, activation="none") -> torch.Tensor:
    """act(x @ wt^T + bias) in f64; x [M, K] and wt [N, K] bf16, bias f32."""
    y = f64(x) @ f64(wt).T
    if bias is not None:
        y = y + f64(bias)
    return _act(y, activation)


def linear_bound(x, wt, bias=None, activation="none") -> torch.Tensor:
    """|kernel - ref_linear| <= u |act(ref)| + L gamma_{K+2} (|x| |w|^T + |b|).

    The products of two bf16 are exact in f32, so the pre-activation value is
    a sum of K exact terms and the bias, accumulated in f32 in some order:
    at most K roundings on any term, gamma_K (|x| |w|^T + |b|) whatever the
    order. Two more roundings cover the activation's own arithmetic, and the
    activation carries the pre-activation error to its output with its
    Lipschitz constant L (1 for none / relu, 1.13 for tanh-GELU). The single
    rounding of the result to bf16 adds u |act(ref)|."""
    K = x.shape[1]
    mag = f64(x).abs() @ f64(wt).abs().T
    if bias is not None:
        mag = mag + f64(bias).abs()
    ref = ref_linear(x, wt, bias, activation)
    return U * ref.abs() + ACT_LIPSCHITZ[activation] * gamma(K + 2) * mag


# ---------------------------------------------------------------------------
# layernorm
# ---------------------------------------------------------------------------


def _ln_parts(x, residual, eps):
    v = f64(x)
    if residual is not None:
        v = v + f64(residual)
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    return v, mu, 1.0 / torch.sqrt(var + eps)


def ref_layernorm(x, gamma_, beta, residual=None, eps=EPS):
    """(y, xres) in f64: y = (v - mean) rstd gamma + beta with v = x +
    residual and the biased variance; xres = v."""
    v, mu, rstd = _ln_parts(x, residual, eps)
    return (v - mu) * rstd * f64(gamma_) + f64(beta), v


def layernorm_bound(x, gamma_, beta, residual=None, eps=EPS) -> torch.Tensor:
    """|kernel - y| <= u |y| + gamma_{D+4} (|v - mu| + |mu|) rstd |g|.

    v = x + r is exact in f32 for the bf16 inputs used here. The f32 mean of
    D values is off by at most gamma_D |mu'| with mu' the mean of |v|
    (<= |v - mu| + |mu| element-wise after the subtraction); the two-pass
    variance and rsqrtf move rstd by a few ulp relative, which scales
    |v - mu|; the subtraction, the two multiplications and the addition of
    beta are four more roundings. Together at most D + 4 roundings on a
    quantity no larger than (|v - mu| + |mu|) rstd |g|. The single rounding
    of y to bf16 adds u |y|."""
    D = x.shape[-1]
    v, mu, rstd = _ln_parts(x, residual, eps)
    y, _ = ref_layernorm(x, gamma_, beta, residual, eps)
    return U * y.abs() + gamma(D + 4) * ((v - mu).abs() + mu.abs()) * rstd * f64(gamma_).abs()


def xres_expected(x, residual=None) -> torch.Tensor:
    """The bits the kernel must write as xres."""
    v = x.float()
    if residual is not None:
        v = v + residual.float()
    return v.bfloat16()


# ---------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------

ATTENTION_MUTANTS = ("uniform", "exp2", "droplast", "nomax")


def _softmax_pv(s: torch.Tensor, v: torch.Tensor, mutant: Optional[str]):
    """softmax(s) and softmax(s) @ v, or a wrong variant of them."""
    if mutant == "nomax":  # f32, no max subtraction: overflows
        e = torch.exp(s.float())
        p = (e / e.sum(-1, keepdim=True)).double()
        return p, p @ v
    if mutant == "droplast":
        s, v = s[..., :-1], v[..., :-1, :]
    if mutant == "uniform":
        p = torch.full_like(s, 1.0 / s.shape[-1])
    elif mutant == "exp2":
        p = torch.softmax(s * math.log(2.0), dim=-1)
    else:
        assert mutant in (None, "droplast"), mutant
        p = torch.softmax(s, dim=-1)
    return p, p @ v


def ref_attention(q, k, v, scale=None, mutant=None) -> torch.Tensor:
    """softmax(q k^T scale) v in f64 for [BH, S, Dh] bf16 inputs."""
    q, k, v = f64(q), f64(k), f64(v)
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    return _softmax_pv(q @ k.transpose(-1, -2) * scale, v, mutant)[1]


def split_qkv(qkv, S, H, Dh):
    """[B, S, 3*H*Dh] (q | k | v, heads inside each) -> three [B*H, S, Dh]."""
    B = qkv.shape[0]
    parts = qkv.reshape(B, S, 3, H, Dh).permute(2, 0, 3, 1, 4)
    return tuple(p.reshape(B * H, S, Dh) for p in parts)


def merge_heads(o, B, S, H, Dh):
    """[B*H, S, Dh] -> [B, S, H*Dh]."""
    return o.reshape(B, H, S, Dh).permute(0, 2, 1, 3).reshape(B, S, H * Dh)


def ref_attention_qkv(qkv, S, H, Dh, scale=None, mutant=None) -> torch.Tensor:
    q, k, v = split_qkv(qkv, S, H, Dh)
    return merge_heads(ref_attention(q, k, v, scale, mutant), qkv.shape[0], S, H, Dh)


def attention_bound(q, k, v, scale=None, p_bf16=False) -> torch.Tensor:
    """|kernel - ref_attention| element-wise, [BH, S, Dh].

    Logits: s_ij is a sum of Dh exact products accumulated in f32 and one
    multiplication by scale, so |ds_ij| <= gamma_{Dh+2} scale (|q| |k|^T)_ij.
    ``__expf`` reduces its argument with a rounded log2(e), an error that
    grows with the argument: 2^-21 (1 + max |s|) covers it and the
    subtraction of the row maximum. With ds the largest of these over the
    row, every p_ij = e_ij / sum_j e_ij moves by at most 2 ds relative
    (numerator and denominator), so the output moves by at most
    2 ds (P |V|).

    The VALU kernel keeps P in f32 and rounds only the output:
        u |ref| + 2 ds (P |V|).
    The MFMA kernel also rounds the unnormalised P to bf16 before P V, a
    relative error u on every term of the sum:
        u (P |V| + |ref|) + 2 ds (P |V|).
    """
    q, k, v = f64(q), f64(k), f64(v)
    Dh = q.shape[-1]
    if scale is None:
        scale = 1.0 / math.sqrt(Dh)
    s = q @ k.transpose(-1, -2) * scale
    p = torch.softmax(s, dim=-1)
    ref = p @ v
    pv = p @ v.abs()
    mag = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    ds = gamma(Dh + 2) * scale * mag + 2.0 ** -21 * (1.0 + s.abs().amax(-1, keepdim=True))
    bound = U * ref.abs() + 2.0 * ds * pv
    if p_bf16:
        bound = bound + U * pv
    return bound


def attention_qkv_bound(qkv, S, H, Dh, scale=None) -> torch.Tensor:
    q, k, v = split_qkv(qkv, S, H, Dh)
    return merge_heads(attention_bound(q, k, v, scale, p_bf16=True),
                       qkv.shape[0], S, H, Dh)


#: gain of q and k; v is randn plus a per-column offset, so that a transposed
#: or misplaced V is a gross error
ATTENTION_GAIN = {"small": 0.5, "sharp": 2.0, "overflow": 6.0}


def attention_inputs(BH, S, Dh, kind, seed):
    """(q, k, v) bf16 [BH, S, Dh] on the CPU. ``small`` is the scale of the
    older tests (q, k and v all randn * 0.5, no offset)."""
    g = torch.Generator().manual_seed(seed)
    gain = ATTENTION_GAIN[kind]
    q = torch.randn(BH, S, Dh, generator=g) * gain
    k = torch.randn(BH, S, Dh, generator=g) * gain
    v = torch.randn(BH, S, Dh, generator=g)
    if kind == "small":
        v = v * 0.5
    else:
        v = v + torch.linspace(-2.0, 2.0, Dh)
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def qkv_inputs(B, S, H, Dh, kind, seed):
    """The same inputs packed as the qkv projection emits them."""
    q, k, v = attention_inputs(B * H, S, Dh, kind, seed)
    parts = [t.reshape(B, H, S, Dh).permute(0, 2, 1, 3) for t in (q, k, v)]
    return torch.stack(parts, dim=2).reshape(B, S, 3 * H * Dh).contiguous()


# ---------------------------------------------------------------------------
# the fused BERT kernel
# ---------------------------------------------------------------------------

MUTANTS = ("uniform", "exp2", "droplast", "swapheads", "sum16", "noattn",
           "bias_shift", "relu", "half1", "b2twice", "eps", "start+1")

#: the places where bert_fused.hip rounds to bf16, in program order
CHAIN_POINTS = ("embed", "qkv", "p", "attn", "proj", "ln1", "ffn", "w2_0",
                "w2_1", "ln2")


def span_tokens(lines, start, end, shift=0) -> torch.Tensor:
    """[B, 64] token ids of the content spans [start + shift, end): byte + 3,
    0 where the span or the line has ended (embed() of bert_fused.hip)."""
    lines, start, end = lines.cpu(), start.cpu().long() + shift, end.cpu().long()
    max_len = lines.shape[1]
    idx = start[:, None] + torch.arange(S_FUSED)[None, :]
    valid = (idx < end[:, None]) & (idx < max_len)
    byte = lines.long().gather(1, idx.clamp(max=max_len - 1))
    return torch.where(valid, byte + 3, torch.zeros_like(byte))


def _ln(v, g, b, eps):
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    return (v - mu) / torch.sqrt(var + eps) * g + b


def ref_bert(model, tokens, *, mutant: Optional[str] = None, chain: bool = False,
             points: Sequence[str] = CHAIN_POINTS) -> torch.Tensor:
    """Final hidden states [B, 64, 128] in f64 of ``model`` (any object with
    BertTinyDetectorModel's weight attributes). ``tokens`` is [B, 64] ids or,
    as the ``start+1`` mutant needs, the triple (lines, start, end).

    Post-LN encoder, tanh-form GELU, eps 1e-5, no padding mask (the kernel
    has none), FFN in two halves of 256 as the kernel runs it. The pooled
    embedding is ``.mean(1)``; ``ref_score`` gives the score.

    With ``chain`` the value is rounded to bf16 at the ``points`` (default:
    all of CHAIN_POINTS) where the kernel stores bf16, cited below by line of
    ops/csrc/bert_fused.hip; everything between two points stays f64.
    """
    assert mutant is None or mutant in MUTANTS, mutant
    on = set(points) if chain else set()
    assert on <= set(CHAIN_POINTS), on

    def rnd(point, t):
        return bf16_round(t) if point in on else t

    if isinstance(tokens, (tuple, list)):
        tokens = span_tokens(*tokens, shift=1 if mutant == "start+1" else 0)
    else:
        assert mutant != "start+1", "start+1 needs (lines, start, end)"
    tokens = tokens.cpu().long()
    B, S = tokens.shape
    H = model.config.hidden
    heads, Dh = model.config.heads, model.config.head_dim
    half = model.config.ffn // 2
    scale = 1.0 / math.sqrt(Dh)
    eps = 1e-3 if mutant == "eps" else EPS

    # embed(), line 340: x = bf16(tok_emb + pos_emb)
    x = rnd("embed", f64(model.tok_emb)[tokens] + f64(model.pos_emb)[:S])
    for layer in model.layers:
        w = {k: f64(t) for k, t in layer.items()}
        # qkv GEMM, bias seeded into the accumulator (line 186), stored as
        # bf16 at line 241 (Q | K) and line 228 (V, transposed)
        qkv = rnd("qkv", x @ w["wqkv_t"].T + w["bqkv"])
        q, k, v = (t.reshape(B, S, heads, Dh).transpose(1, 2)
                   for t in qkv.split(H, dim=-1))          # [B, heads, S, Dh]
        s = q @ k.transpose(-1, -2) * scale
        if mutant == "droplast":
            s, v = s[..., :-1], v[..., :-1, :]
        if mutant == "uniform":
            e = torch.ones_like(s)
        elif mutant == "exp2":
            e = torch.exp2(s - s.amax(-1, keepdim=True))
        else:
            e = torch.exp(s - s.amax(-1, keepdim=True))
        # line 385: the row sum is taken over the unrounded f32 values
        denom = (e[..., :16] if mutant == "sum16" else e).sum(-1, keepdim=True)
        # line 395: the UNNORMALISED probabilities leave as bf16 P tiles
        p = rnd("p", e)
        if mutant == "swapheads":
            p = p.flip(1)
        # lines 415-416: O * (1 / sum), stored as bf16
        attn = rnd("attn", (p @ v) / denom)
        attn = attn.transpose(1, 2).reshape(B, S, H)
        if mutant == "noattn":
            attn = torch.zeros_like(attn)
        bo = w["bo"].roll(1) if mutant == "bias_shift" else w["bo"]
        # Wo GEMM in residual mode, lines 232-235: x = bf16(x + attn Wo^T + bo)
        x = rnd("proj", x + attn @ w["wo_t"].T + bo)
        # block_layernorm, lines 459-462
        x = rnd("ln1", _ln(x, w["ln1_g"], w["ln1_b"], eps))
        x1 = x  # both halves of the FFN read the LN1 output
        for h in range(2):
            if h == 1 and mutant == "half1":
                break
            rows = slice(h * half, (h + 1) * half)
            pre = x1 @ w["w1_t"][rows].T + w["b1"][rows]
            # line 239-242: bf16(gelu(x W1_h^T + b1_h))
            hid = rnd("ffn", torch.relu(pre) if mutant == "relu" else gelu_tanh(pre))
            upd = hid @ w["w2_t"][:, rows].T
            if h == 0 or mutant == "b2twice":
                upd = upd + w["b2"]      # b2 once, with half 0 (line 638)
            # lines 232-235 again: x = bf16(x + half W2_h^T [+ b2])
            x = rnd("w2_0" if h == 0 else "w2_1", x + upd)
        x = rnd("ln2", _ln(x, w["ln2_g"], w["ln2_b"], eps))
    return x


def ref_score(model, hidden: torch.Tensor) -> torch.Tensor:
    """Scores [B] of final hidden states: mean over tokens, then the head."""
    return (hidden.mean(1) @ f64(model.w_score) + f64(model.b_score)).squeeze(-1)


def e_chain(model, tokens):
    """(ref, E_chain pooled, E_chain score): the reference hidden states and
    the distance the kernel's own bf16 storage puts between it and them."""
    ref = ref_bert(model, tokens)
    chained = ref_bert(model, tokens, chain=True)
    e_emb = (chained.mean(1) - ref.mean(1)).abs().max().item()
    e_score = (ref_score(model, chained) - ref_score(model, ref)).abs().max().item()
    return ref, e_emb, e_score


# ---------------------------------------------------------------------------
# models at three scales, and the batch of the fused tests
# ---------------------------------------------------------------------------

FUSED_LAYERS = (1, 2, 4)
FUSED_BATCH_ROWS = (1, 22)


def fused_model_seed(layers: int) -> int:
    """Model seed of the fused tests (affines: the seed after it)."""
    return 40 + layers


def fused_batch(B: int):
    """(lines, start, end) on the CPU: random bytes 0..255, spans cycling
    through EDGE_SPANS of test_bert_fused_epilogue.py. B = 1 is the
    truncating span; B = 22 runs through all eleven twice."""
    from test_bert_fused_epilogue import _edge_batch

    return _edge_batch(B, seed=56 + B)


REGIMES = ("small", "sharp", "tiny")
SHARP_EMB_GAIN = 50.0
SHARP_W_GAIN = 5.0
TINY_EMB_GAIN = 1.0 / 16.0


def _randomize_affine(model, seed):
    """Random biases and LN affines, drawn as test_bert_fused_epilogue.py
    draws them (the model initialises them to 0 / 1, which would hide a bias
    fetched from the wrong column)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(like, std, mean=0.0):
        return (torch.randn(like.shape, generator=g) * std + mean).to(like.dtype)

    for layer in model.layers:
        for k in ("bqkv", "bo", "b1", "b2"):
            layer[k] = rnd(layer[k], 0.05)
        for k in ("ln1_g", "ln2_g"):
            layer[k] = rnd(layer[k], 0.1, 1.0)
        for k in ("ln1_b", "ln2_b"):
            layer[k] = rnd(layer[k], 0.05)
    model.b_score = rnd(model.b_score, 0.05)


def regime_model(layers: int, seed: int, regime: str, device="cpu"):
    """BertTinyDetectorModel(seed) with affines randomised from seed + 1,
    scaled for ``regime`` in f32 on the CPU, cast to bf16 there and loaded
    into a model on ``device`` through load_state_dict, so that every device
    holds the same bits.

    small: the scale of the older tests; the softmax is uniform to 2%.
    sharp: embeddings x 50, wqkv / wo / w1 / w2 x 5: logits of several units,
           a peaked softmax, GELU well outside its linear part.
    tiny:  embeddings x 1/16 and layer 0's bo = 0: the variance entering LN1
           of layer 0 is comparable to eps.
    """
    from detectmateservice_amd.models.bert_tiny import (
        BertTinyConfig,
        BertTinyDetectorModel,
    )

    assert regime in REGIMES, regime
    cfg = BertTinyConfig(layers=layers)
    cpu = BertTinyDetectorModel(cfg, device="cpu", seed=seed)
    _randomize_affine(cpu, seed + 1)

    def scaled(t, gain):
        return (t.float() * gain).to(t.dtype)

    if regime == "sharp":
        cpu.tok_emb = scaled(cpu.tok_emb, SHARP_EMB_GAIN)
        cpu.pos_emb = scaled(cpu.pos_emb, SHARP_EMB_GAIN)
        for layer in cpu.layers:
            for k in ("wqkv_t", "wo_t", "w1_t", "w2_t"):
                layer[k] = scaled(layer[k], SHARP_W_GAIN)
    elif regime == "tiny":
        cpu.tok_emb = scaled(cpu.tok_emb, TINY_EMB_GAIN)
        cpu.pos_emb = scaled(cpu.pos_emb, TINY_EMB_GAIN)
        cpu.layers[0]["bo"] = torch.zeros_like(cpu.layers[0]["bo"])
    out = BertTinyDetectorModel(cfg, device=device, seed=seed)
    out.load_state_dict(cpu.state_dict())
    return out
