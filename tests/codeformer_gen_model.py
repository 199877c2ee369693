"""Row f22: the back of CodeFormer (``CodeFormer.forward`` from ``quant_feat`` to ``out``: the VQGAN generator with its four ``Fuse_sft_block``s) restated block by
block from its formulas on top of ``codeformer_model.front``, in float64 or, with ``dtype=torch.float32``, as the float32 restatement the kernel tests take their
bars from; what tests/golden/g32_codeformer_gen.npz stores; single-change mutants that the CPU test requires to move the outputs.  Nothing here imports
``e4s2024_amd.ops`` or the library.

    generator            conv_in, ResBlock, AttnBlock, ResBlock, then per level (512, 256, 256, 128, 128, 64 channels) two ResBlocks (each followed by an
                         AttnBlock at the first level) and, but for the last level, Upsample; GroupNorm without swish; the 3 x 3 convolution to 3 channels
    Upsample             nearest x 2 (out[y, x] = in[y // 2, x // 2]), then a 3 x 3 convolution
    Fuse_sft_block       e = ResBlock(2 C, C)(cat([enc, dec], 1)); scale = conv(leaky(conv(e))), shift likewise, leaky(v) = v if v >= 0 else 0.2 v;
                         out = dec + w (dec scale + shift), in that order
    fuse points          behind generator blocks 9, 12, 15, 18 for the encoder taps '32', '64', '128', '256', by block index; none at w <= 0
    tensor2img           uint8(rint((clamp(x, -1, 1) - (-1)) / 2 * 255)), every step in float32 (``image_u8``)
"""
import numpy as np
import torch
import torch.nn.functional as F

import codeformer_model as M

FUSE_BLOCKS = {9: "32", 12: "64", 15: "128", 18: "256"}
CHANNELS = {"32": 256, "64": 256, "128": 128, "256": 128}
FEATS = ("dec32", "dec64", "dec128", "dec256")
NAMES = ("out",) + FEATS
MUTANTS = ("sft_no_product", "cat_dec_first", "fuse_one_block_early", "up_after_conv", "leaky_as_relu", "w_ignored")
W = 0.8


def generator_plan():
    chans = [64 * m for m in (1, 2, 2, 4, 4, 8)]
    cin = chans[-1]
    out = [("conv", 256, cin), ("res", cin, cin), ("attn", cin, cin), ("res", cin, cin)]
    for i in reversed(range(6)):
        for _ in range(2):
            out.append(("res", cin, chans[i]))
            cin = chans[i]
            if i == 5:
                out.append(("attn", cin, cin))
        if i != 0:
            out.append(("up", cin, cin))
    return out + [("norm", cin, cin), ("conv", cin, 3)]


def res_block(P, p, x, cin, cout):
    h = F.conv2d(M.group_norm(x, P[p + "norm1.weight"], P[p + "norm1.bias"], True), P[p + "conv1.weight"], P[p + "conv1.bias"], padding=1)
    h = F.conv2d(M.group_norm(h, P[p + "norm2.weight"], P[p + "norm2.bias"], True), P[p + "conv2.weight"], P[p + "conv2.bias"], padding=1)
    return h + (F.conv2d(x, P[p + "conv_out.weight"], P[p + "conv_out.bias"]) if cin != cout else x)


def attn_block(P, p, x):
    n, c, hh, ww = x.shape
    hn = M.group_norm(x, P[p + "norm.weight"], P[p + "norm.bias"], False)
    q, k, v = (F.conv2d(hn, P[p + m + ".weight"], P[p + m + ".bias"]).reshape(n, c, hh * ww) for m in "qkv")
    return x + F.conv2d(M.attention(q, k, v, 1, float(c) ** -0.5).reshape(n, c, hh, ww), P[p + "proj_out.weight"], P[p + "proj_out.bias"])


def up2(x):
    n, c, hh, ww = x.shape
    return x[:, :, :, None, :, None].expand(n, c, hh, 2, ww, 2).reshape(n, c, 2 * hh, 2 * ww)


def leaky(x, slope=0.2):
    return torch.where(x >= 0, x, slope * x)


def sft(dec, scale, shift, w):
    t = dec * scale
    t = t + shift
    t = w * t
    return dec + t


def fuse(P, s, enc, dec, w, mutant=None):
    """``Fuse_sft_block`` '``s``' on the dict ``P`` of tensors of one dtype."""
    p, C = f"fuse_convs_dict.{s}.", CHANNELS[s]
    e = res_block(P, p + "encode_enc.", torch.cat([dec, enc] if mutant == "cat_dec_first" else [enc, dec], 1), 2 * C, C)
    slope = 0.0 if mutant == "leaky_as_relu" else 0.2
    branch = lambda b: F.conv2d(leaky(F.conv2d(e, P[p + b + ".0.weight"], P[p + b + ".0.bias"], padding=1), slope), P[p + b + ".2.weight"], P[p + b + ".2.bias"], padding=1)  # noqa: E731
    scale, shift = branch("scale"), branch("shift")
    if mutant == "sft_no_product":
        return dec + w * (scale + shift)
    return sft(dec, scale, shift, 1.0 if mutant == "w_ignored" else w)


def generate(sd, front, w=W, dtype=torch.float64, mutant=None):
    """dict(out, dec32 .. dec256, before32 .. before256) of the generator on ``front`` (what ``codeformer_model.front`` returns: its ``quant_feat`` and, with
    ``w > 0``, ``tap32 .. tap256`` are read) under the weights ``sd``: ``dec<s>`` the decoder feature behind fuse block ``s``, ``before<s>`` in front of it.
    The mutant ``fuse_one_block_early`` moves the fuse blocks '64' and '256' in front of the ResBlock they follow (behind the Upsample, where the channel count
    already fits)."""
    assert mutant is None or mutant in MUTANTS, mutant
    P = {k: v.to(dtype) for k, v in sd.items() if k.startswith(("generator.", "fuse_convs_dict."))}
    x = torch.as_tensor(front["quant_feat"]).to(dtype)
    fuse_at = dict(FUSE_BLOCKS)
    if mutant == "fuse_one_block_early":
        fuse_at = {9: "32", 11: "64", 15: "128", 17: "256"}
    out = {}
    for i, (kind, cin, cout) in enumerate(generator_plan()):
        p = f"generator.blocks.{i}."
        if kind == "conv":
            x = F.conv2d(x, P[p + "weight"], P[p + "bias"], padding=1)
        elif kind == "res":
            x = res_block(P, p, x, cin, cout)
        elif kind == "attn":
            x = attn_block(P, p, x)
        elif kind == "up":
            conv = lambda t: F.conv2d(t, P[p + "conv.weight"], P[p + "conv.bias"], padding=1)                # noqa: E731
            x = up2(conv(x)) if mutant == "up_after_conv" else conv(up2(x))
        else:
            x = M.group_norm(x, P[p + "weight"], P[p + "bias"], False)
        if i in fuse_at and w > 0:
            s = fuse_at[i]
            out["before" + s] = x
            x = out["dec" + s] = fuse(P, s, torch.as_tensor(front["tap" + s]).to(dtype), x, w, mutant)
    out["out"] = x
    return out


def image_u8(x):
    """The caller's ``tensor2img(x, min_max=(-1, 1))`` on a float32 numpy array, every step in float32."""
    v = np.minimum(np.maximum(np.asarray(x, dtype=np.float32), np.float32(-1)), np.float32(1))
    v = (v - np.float32(-1)) / np.float32(2)
    v = v * np.float32(255)
    return np.rint(v).astype(np.uint8)


def fuse_statistics(got):
    """(growth, term / dec) per fuse block and the share of ``out`` inside [-1, 1], of a ``generate`` dict (or the reference's tensors under its names)."""
    growth, ratio = [], []
    for s in M.CONNECT:
        before, after = np.asarray(got["before" + s], dtype=np.float64), np.asarray(got["dec" + s], dtype=np.float64)
        growth.append(after.std() / before.std())
        ratio.append((after - before).std() / before.std())
    out = np.asarray(got["out"])
    return np.array(growth), np.array(ratio), float((np.abs(out) <= 1).mean())
