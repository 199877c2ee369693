"""Row f21: the front of CodeFormer (everything in ``CodeFormer.forward`` up to ``quant_feat``) restated block by block from its formulas, in float64 or, with
``dtype=torch.float32``, as the float32 restatement the kernel tests take their bars from; the cases of tests/golden/g31_codeformer.npz; single-change mutants
that the CPU test requires to move the outputs.  Nothing here imports ``e4s2024_amd.ops`` or the library: weights come from ``seeded`` alone.

    GroupNorm(32, 1e-6)   per group of C / 32 channels: (x - mean) / sqrt(var + 1e-6) gamma_c + beta_c, var biased; swish s -> s / (1 + exp(-s))
    ResBlock              conv2(swish(norm2(conv1(swish(norm1(x)))))) + (conv_out(x) | x)
    Downsample            one zero column right, one zero row below, then 3 x 3 stride 2 without padding
    AttnBlock             x + proj_out(v softmax_j(q_i . k_j C^-0.5)^T) on the 1 x 1 projections of norm(x)
    transformer layer     t += out_proj(MHA(q = k = norm1(t) + pos, v = norm1(t))); t += linear2(gelu(linear1(norm2(t)))), gelu in its erf form
    head                  logits = LayerNorm(t) W^T; the top-1 code; quant = codebook[idx]; AdaIN with the UNBIASED variance and eps inside the root
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from e4s2024_amd import seeded  # noqa: E402

CASES = {
    "CF-S": dict(cfg=(64, 2, 2, 40, 6), shape=(2, 3, 64, 96), seed=211),
    "CF-T": dict(cfg=(64, 2, 2, 40, 4), shape=(1, 3, 32, 128), seed=212),
    "CF-F": dict(cfg=(512, 8, 9, 1024, 256), shape=(1, 3, 512, 512), seed=213),
}
CONNECT = ("32", "64", "128", "256")
TAP_BLOCKS = {14: "32", 11: "64", 8: "128", 5: "256"}
NAMES = ("lq_feat", "logits", "quant_feat", "tap32", "tap64", "tap128", "tap256")
MUTANTS = ("adain_biased", "adain_eps_outside", "pos_on_v", "no_swish_before_last_norm", "down_symmetric")
FULL_LIMIT, SAMPLES, CLOSE_FACTOR, CLOSE_SHARE = 16384, 4096, 64.0, 0.02


def encoder_plan():
    chans = [64 * m for m in (1, 2, 2, 4, 4, 8)]
    out, cin = [("conv", 3, 64)], 64
    for i, c in enumerate(chans):
        for _ in range(2):
            out.append(("res", cin, c))
            cin = c
            if i == 5:
                out.append(("attn", c, c))
        if i != 5:
            out.append(("down", c, c))
    return out + [("res", 512, 512), ("attn", 512, 512), ("res", 512, 512), ("norm", 512, 512), ("conv", 512, 256)]


def case_input(tag):
    """A float32 image in [-1, 1] with structure at 8 pixels and at 1: coarse cells plus fine noise."""
    n, c, h, w = CASES[tag]["shape"]
    seed = CASES[tag]["seed"]
    coarse = seeded.seeded_array(seed, "cf.coarse", (n, c, h // 8, w // 8), dist="normal")
    fine = seeded.seeded_array(seed, "cf.fine", (n, c, h, w), dist="normal")
    x = 0.6 * np.repeat(np.repeat(coarse, 8, axis=2), 8, axis=3) + 0.25 * fine
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def case_weights(tag):
    return seeded.seeded_codeformer_state_dict(CASES[tag]["seed"], *CASES[tag]["cfg"], CONNECT)


def group_norm(x, w, b, swish):
    n, c = x.shape[:2]
    g = x.reshape(n, 32, -1)
    m = g.mean(2, keepdim=True)
    var = ((g - m) ** 2).mean(2, keepdim=True)
    s = ((g - m) / torch.sqrt(var + 1e-6)).reshape(x.shape) * w.view(1, c, 1, 1) + b.view(1, c, 1, 1)
    return s / (1 + torch.exp(-s)) if swish else s


def softmax_rows(s):
    e = torch.exp(s - s.max(-1, keepdim=True)[0])
    return e / e.sum(-1, keepdim=True)


def attention(q, k, v, heads, scale):
    """Channel-major ``[n, heads d, T]`` operands: out[b, h d + c, i] = sum_j softmax_j(scale q_i . k_j) v[c, j]."""
    n, C, T = q.shape
    d = C // heads
    q, k, v = (t.reshape(n, heads, d, T) for t in (q, k, v))
    p = softmax_rows(torch.einsum("bhci,bhcj->bhij", q, k) * scale)
    return torch.einsum("bhij,bhcj->bhci", p, v).reshape(n, C, T)


def layer_norm_cm(x, w, b):
    """LayerNorm over the channels of a channel-major ``[n, C, T]`` tensor."""
    m = x.mean(1, keepdim=True)
    var = ((x - m) ** 2).mean(1, keepdim=True)
    return (x - m) / torch.sqrt(var + 1e-5) * w.view(1, -1, 1) + b.view(1, -1, 1)


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / np.sqrt(2.0)))


def adain(content, style, biased=False, eps_outside=False, eps=1e-5):
    n, c = content.shape[:2]

    def stat(t):
        t = t.reshape(n, c, -1)
        m = t.mean(2, keepdim=True)
        var = ((t - m) ** 2).sum(2, keepdim=True) / (t.shape[2] - (0 if biased else 1))
        return m.view(n, c, 1, 1), (torch.sqrt(var) + eps if eps_outside else torch.sqrt(var + eps)).view(n, c, 1, 1)
    (sm, ss), (cm, cs) = stat(style), stat(content)
    return (content - cm) / cs * ss + sm


def front(sd, x, cfg, dtype=torch.float64, adain_on=True, mutant=None, idx=None):
    """dict(lq_feat, logits [n, T, K], idx, quant_feat, tap32 .. tap256, top1, top2) of the image ``x`` under the weights ``sd`` at ``cfg`` = (dim_embd, n_head,
    n_layers, codebook_size, latent_size); ``idx``: the codes to look up instead of the model's own."""
    assert mutant is None or mutant in MUTANTS, mutant
    E, n_head, n_layers, K, T = cfg
    P = {k: v.to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(x).to(dtype)
    out = {}
    plan = encoder_plan()
    for i, (kind, cin, cout) in enumerate(plan):
        p = f"encoder.blocks.{i}."
        if kind == "conv":
            x = F.conv2d(x, P[p + "weight"], P[p + "bias"], padding=1)
        elif kind == "res":
            drop = mutant == "no_swish_before_last_norm" and i == len(plan) - 3
            h = F.conv2d(group_norm(x, P[p + "norm1.weight"], P[p + "norm1.bias"], True), P[p + "conv1.weight"], P[p + "conv1.bias"], padding=1)
            h = F.conv2d(group_norm(h, P[p + "norm2.weight"], P[p + "norm2.bias"], not drop), P[p + "conv2.weight"], P[p + "conv2.bias"], padding=1)
            x = h + (F.conv2d(x, P[p + "conv_out.weight"], P[p + "conv_out.bias"]) if cin != cout else x)
        elif kind == "attn":
            n, c, hh, ww = x.shape
            hn = group_norm(x, P[p + "norm.weight"], P[p + "norm.bias"], False)
            q, k, v = (F.conv2d(hn, P[p + m + ".weight"], P[p + m + ".bias"]).reshape(n, c, hh * ww) for m in "qkv")
            x = x + F.conv2d(attention(q, k, v, 1, float(c) ** -0.5).reshape(n, c, hh, ww), P[p + "proj_out.weight"], P[p + "proj_out.bias"])
        elif kind == "down":
            if mutant == "down_symmetric":
                x = F.conv2d(x, P[p + "conv.weight"], P[p + "conv.bias"], stride=2, padding=1)
            else:
                n, c, hh, ww = x.shape
                padded = torch.zeros((n, c, hh + 1, ww + 1), dtype=dtype)
                padded[:, :, :hh, :ww] = x
                x = F.conv2d(padded, P[p + "conv.weight"], P[p + "conv.bias"], stride=2)
        else:
            x = group_norm(x, P[p + "weight"], P[p + "bias"], False)
        if i in TAP_BLOCKS:
            out["tap" + TAP_BLOCKS[i]] = x
    lq = out["lq_feat"] = x
    n, c, hh, ww = lq.shape
    assert hh * ww == T, (lq.shape, T)
    lin = lambda t, w, b=None: torch.einsum("oc,bct->bot", w, t) + (0 if b is None else b.view(1, -1, 1))      # noqa: E731  (channel-major linear)
    pos = P["position_emb"].t().unsqueeze(0)                                                                  # [1, E, T]
    t = lin(lq.reshape(n, c, T), P["feat_emb.weight"], P["feat_emb.bias"])
    for li in range(n_layers):
        p = f"ft_layers.{li}."
        w, b = P[p + "self_attn.in_proj_weight"], P[p + "self_attn.in_proj_bias"]
        n1 = layer_norm_cm(t, P[p + "norm1.weight"], P[p + "norm1.bias"])
        qk_in = n1 + pos
        q, k = lin(qk_in, w[:E], b[:E]), lin(qk_in, w[E:2 * E], b[E:2 * E])
        v = lin(qk_in if mutant == "pos_on_v" else n1, w[2 * E:], b[2 * E:])
        a = attention(q, k, v, n_head, float(E // n_head) ** -0.5)
        t = t + lin(a, P[p + "self_attn.out_proj.weight"], P[p + "self_attn.out_proj.bias"])
        n2 = layer_norm_cm(t, P[p + "norm2.weight"], P[p + "norm2.bias"])
        t = t + lin(gelu(lin(n2, P[p + "linear1.weight"], P[p + "linear1.bias"])), P[p + "linear2.weight"], P[p + "linear2.bias"])
    logits = lin(layer_norm_cm(t, P["idx_pred_layer.0.weight"], P["idx_pred_layer.0.bias"]), P["idx_pred_layer.1.weight"]).transpose(1, 2)
    out["logits"] = logits                                                                                    # [n, T, K]
    top = torch.topk(logits, 2, dim=2)[0]
    out["top1"], out["top2"] = top[..., 0], top[..., 1]
    own = (logits == top[..., :1]).to(torch.int64).argmax(2)                                                  # the lowest index at the maximum
    out["idx"] = own if idx is None else torch.as_tensor(idx)
    quant = P["quantize.embedding.weight"][out["idx"].reshape(-1)].reshape(n, hh, ww, c).permute(0, 3, 1, 2)
    out["quant_feat"] = adain(quant, lq, biased=mutant == "adain_biased", eps_outside=mutant == "adain_eps_outside") if adain_on else quant
    return out


# ------------------------------------------------------------------------------------------------ what the fixture stores of an array
def sample_stride(size):
    """1 for an array the fixture stores in full; otherwise the odd stride at which its flat index is sampled."""
    q = size // SAMPLES                               # the largest odd stride that still gives SAMPLES samples
    return 1 if size <= FULL_LIMIT else (q if q % 2 else q - 1)


def sampled(a, stride):
    a = np.asarray(a)
    return a if stride == 1 else a.reshape(-1)[::stride][:SAMPLES]


def token_stride(tag):
    n, T, K = CASES[tag]["shape"][0], CASES[tag]["cfg"][4], CASES[tag]["cfg"][3]
    return 4 if n * T * K > 65536 else 1


def stored(tag, name, a):
    """What the fixture holds of output ``name``: the logits every ``token_stride``-th token, anything else in full or as strided samples."""
    a = np.asarray(a)
    if name == "logits":
        return a[:, ::token_stride(tag)]
    return sampled(a, sample_stride(a.size))


def close_tokens(top1, top2, e32_logits):
    """The tokens whose float64 top-1 - top-2 margin is below 64 float32 errors of the logits: their code may legitimately differ."""
    return (np.asarray(top1) - np.asarray(top2)) < CLOSE_FACTOR * float(e32_logits)
