"""Row f22: CodeFormer face restoration, stage 2 — everything in ``CodeFormer.forward`` (swap_face_fine/archs/codeformer_arch.py:264-276) from ``quant_feat`` to
``out``, eval mode, forward only, float32 NCHW on the device: the VQGAN generator with its four ``Fuse_sft_block``s, and the caller's uint8 tail.  It starts from
the dict ``ops_codeformer.codeformer_front`` (row f21) returns.

    a ResBlock, an AttnBlock   as in the encoder (``ops_codeformer._res`` / ``_attn_block``): e4s_cf_group_stats + e4s_cf_group_norm, e4s_cf_attention, e4s_conv2d_sb3
    Upsample                   e4s_esr_up2 (nearest x 2), then the 3 x 3 convolution
    the last two blocks        the plain GroupNorm, then the 3 x 3 convolution 64 -> 3 on e4s_conv2d_sb3 like every other one: its 32-wide output tile guards its
                               stores by ``cout``, and the exact e4s_conv2d would spend 2.7 times the matrix-pipe time on the largest plane of the network
    a Fuse_sft_block           ``encode_enc = ResBlock(2 C, C)`` on ``cat([enc, dec], 1)`` without the concatenation: ``norm1 = GroupNorm(32, 2 C)`` has groups of
                               C / 16 channels, none across the seam, so it is GroupNorm with 16 groups on ``enc`` under ``gamma[:C], beta[:C]`` and on ``dec``
                               under ``gamma[C:], beta[C:]``; ``conv1`` and the 1 x 1 ``conv_out`` take the two halves as ``x`` and ``x1`` of ``conv_sb``, ``enc``
                               first.  ``scale`` and ``shift``: 3 x 3, LeakyReLU(0.2) as the convolution's slope vector, 3 x 3.  Then e4s_cf_sft:
                               ``dec + w (dec scale + shift)``
    tensor2img(min_max=(-1, 1)) e4s_cf_image_u8; the reference's ``rgb2bgr=True`` and the caller's ``[:, :, ::-1]`` cancel: RGB stays RGB

The fuse blocks sit behind generator blocks 9, 12, 15, 18 (``CF_FUSE_BLOCKS``), chosen by block index: the reference's ``str(x.shape[-1])`` names the same blocks
at 512 x 512 only.  No host synchronisation; the same inputs give the same bits, a sample of a batch the bits it gets alone; after one eager call (which prepares
the weights) a call captures in a graph.  Every argument is checked before any launch."""
from __future__ import annotations

import math

import torch

from ._lib import lib
from .lossnet import conv_sb, prep_fwd
from .netweights import PreparedNet, _cuda_checked, _tensor_checked, prepare
from .ops import _p, _stream
from .ops_codeformer import (CF_CHANNELS, CF_CONNECT, CF_EMB, CF_MAX_TOKENS, _attn_block, _front_run, _gn_run, _image_checked, _net_of, _placed, _plan, _res,
                             _weights_checked)

GENERATOR_PLAN = tuple(_plan(True))
CF_FUSE_BLOCKS = {"32": 9, "64": 12, "128": 15, "256": 18}         # fuse_generator_block: the fuse block follows that generator block
CF_LEAKY = 0.2
_WIDEST = max(cin for _, cin, _ in GENERATOR_PLAN)                 # 512 channels: the GroupNorm kernel takes bs C <= 65535


class PreparedCodeFormerGenerator(PreparedNet):
    """The kernels' copies of the generator's and the fuse blocks' weights, rebuilt when a tensor changes version or storage: per generator block its convolutions
    as three-way split slabs with their biases (q | k | v of an AttnBlock concatenated to one convolution) and its GroupNorm vectors; per fuse block
    ``encode_enc`` with ``norm1``'s vectors cut at the seam, the four convolutions of ``scale`` and ``shift`` and the constant 0.2 slope vector."""

    __slots__ = ()
    _entry = "codeformer_generate"

    def _net(self, weights):
        return _net_of(weights)

    def _build(self, sd, variant, dev):
        sb = lambda k: prep_fwd(sd[k + ".weight"], None, sd[k + ".bias"])                                                               # noqa: E731
        gn = lambda k: (sd[k + ".weight"], sd[k + ".bias"])                                                                             # noqa: E731
        res = lambda p, cin, cout: dict(n1=gn(p + ".norm1"), c1=sb(p + ".conv1"), n2=gn(p + ".norm2"), c2=sb(p + ".conv2"),              # noqa: E731
                                        out=sb(p + ".conv_out") if cin != cout else None)
        blocks = []
        for i, (kind, cin, cout) in enumerate(GENERATOR_PLAN):
            p = f"generator.blocks.{i}"
            if kind == "conv":
                blocks.append(sb(p))
            elif kind == "res":
                blocks.append(res(p, cin, cout))
            elif kind == "attn":
                qkv = prep_fwd(torch.cat([sd[f"{p}.{m}.weight"] for m in "qkv"]), None, torch.cat([sd[f"{p}.{m}.bias"] for m in "qkv"]))
                blocks.append(dict(norm=gn(p + ".norm"), qkv=qkv, proj=sb(p + ".proj_out")))
            elif kind == "up":
                blocks.append(sb(p + ".conv"))
            else:
                blocks.append(gn(p))
        fuse = {}
        for s in variant[5]:
            p, C = f"fuse_convs_dict.{s}", CF_CHANNELS[s]
            F = res(p + ".encode_enc", 2 * C, C)
            g, b = F.pop("n1")
            F.update(n1e=(g[:C].contiguous(), b[:C].contiguous()), n1d=(g[C:].contiguous(), b[C:].contiguous()),
                     scale0=sb(p + ".scale.0"), scale2=sb(p + ".scale.2"), shift0=sb(p + ".shift.0"), shift2=sb(p + ".shift.2"),
                     slope=torch.full((C,), CF_LEAKY, dtype=torch.float32, device=dev))
            fuse[s] = F
        return dict(config=variant, blocks=blocks, fuse=fuse)


# ------------------------------------------------------------------------------------------------ the kernel-level operators
def _w_checked(name, w):
    if isinstance(w, bool) or not isinstance(w, (int, float)):
        raise TypeError(f"{name}: w must be a Python real (a tensor would need a host read), got {type(w).__name__}")
    if not math.isfinite(w):
        raise ValueError(f"{name}: w must be finite, got {w!r}")
    return float(w)


def _sft(dec, scale, shift, w):
    bs, C, h, wd = dec.shape
    out = torch.empty_like(dec)
    lib().call("e4s_cf_sft", _p(out), _p(dec), _p(scale), _p(shift), w, bs * C, h * wd, _stream())
    return out


def sft_fuse(dec: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, w) -> torch.Tensor:
    """``dec + w * (dec * scale + shift)`` of three float32 ``[bs, C, h, w]`` tensors, each product and sum rounded to float32 in that order; ``w`` a Python real."""
    name = "sft_fuse"
    w = _w_checked(name, w)
    for nm, t in (("dec", dec), ("scale", scale), ("shift", shift)):
        _tensor_checked(name, nm, t, torch.float32, 4, "a float32 [bs, C, h, w] tensor")
        if t.shape != dec.shape:
            raise ValueError(f"{name}: {nm} is {tuple(t.shape)}, dec is {tuple(dec.shape)}")
    if dec.shape[0] * dec.shape[1] > 0x7fffffff or dec.shape[2] * dec.shape[3] < 1:
        raise ValueError(f"{name}: dec is {tuple(dec.shape)}: the planes are not empty and bs C fits an int")
    _cuda_checked(name, dec=dec, scale=scale, shift=shift)
    if scale.device != dec.device or shift.device != dec.device:
        raise RuntimeError(f"{name}: device mismatch among the tensors")
    return _sft(dec.detach().contiguous(), scale.detach().contiguous(), shift.detach().contiguous(), w)


def image_u8(x: torch.Tensor) -> torch.Tensor:
    """``tensor2img(x, min_max=(-1, 1))`` of a float32 ``[n, 3, H, W]`` tensor as uint8 in the same layout and channel order:
    ``rint((clamp(x, -1, 1) + 1) / 2 * 255)``, every step in float32, ties to even."""
    name = "image_u8"
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [n, 3, H, W] tensor")
    if x.shape[1] != 3:
        raise ValueError(f"{name}: x: expected a float32 [n, 3, H, W] tensor, got {tuple(x.shape)}")
    _cuda_checked(name, x=x)
    x = x.detach().contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    lib().call("e4s_cf_image_u8", _p(out), _p(x), x.numel(), _stream())
    return out


# ------------------------------------------------------------------------------------------------ a fuse block, the generator
def _up2(x):
    bs, c, h, w = x.shape
    out = torch.empty((bs, c, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    lib().call("e4s_esr_up2", _p(out), _p(x), bs * c, h, w, _stream())
    return out


def _fuse(enc, dec, F, w):
    h = conv_sb(_gn_run(enc, *F["n1e"], True, 16), *F["c1"], k=3, x1=_gn_run(dec, *F["n1d"], True, 16))
    e = conv_sb(_gn_run(h, *F["n2"], True), *F["c2"], k=3, residual=conv_sb(enc, *F["out"], k=1, x1=dec))
    scale = conv_sb(conv_sb(e, *F["scale0"], k=3, slope=F["slope"]), *F["scale2"], k=3)
    shift = conv_sb(conv_sb(e, *F["shift0"], k=3, slope=F["slope"]), *F["shift2"], k=3)
    return _sft(dec, scale, shift, w)


def _generate(x, taps, P, w):
    """(out, {size: the decoder feature at that fuse point, behind the fuse block when ``w > 0``})."""
    feats, by_block = {}, {CF_FUSE_BLOCKS[s]: s for s in P["config"][5]}
    for i, ((kind, _, _), B) in enumerate(zip(GENERATOR_PLAN, P["blocks"])):
        if kind == "conv":
            x = conv_sb(x, *B, k=3)
        elif kind == "res":
            x = _res(x, B)
        elif kind == "attn":
            x = _attn_block(x, B)
        elif kind == "up":
            x = conv_sb(_up2(x), *B, k=3)
        else:
            x = _gn_run(x, *B, False)
        if i in by_block:
            s = by_block[i]
            if w > 0:
                x = _fuse(taps[s], x, P["fuse"][s], w)
            feats[s] = x
    return x, feats


def _batch_checked(name, bs, C, what):
    if bs * C > 65535:
        raise ValueError(f"{name}: {what}: a batch of {bs} at {C} channels: bs C <= 65535 (the GroupNorm kernel's grid)")


def _feat_checked(name, nm, t, shape, like=None):
    """``t`` is a float32 tensor of ``shape`` (on the device of ``like``)."""
    what = f"a float32 {list(shape)} tensor"
    _tensor_checked(name, nm, t, torch.float32, 4, what)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {nm}: expected {what}, got {tuple(t.shape)}")
    if like is not None and t.device != like.device:
        raise RuntimeError(f"{name}: device mismatch: {nm} on {t.device}, quant_feat on {like.device}")


def _front_checked(name, front, connect, w):
    """(quant_feat, taps) of the dict ``codeformer_front`` returns; the taps are read (and required) with ``w > 0`` only."""
    if not hasattr(front, "keys") or "quant_feat" not in front:
        raise TypeError(f"{name}: front must be the dict codeformer_front returns (its 'quant_feat' and 'taps' are read)")
    q = front["quant_feat"]
    _tensor_checked(name, "quant_feat", q, torch.float32, 4, f"a float32 [n, {CF_EMB}, h, w] tensor")
    n, c, h, wd = q.shape
    if c != CF_EMB or h < 1 or wd < 1:
        raise ValueError(f"{name}: quant_feat: expected a float32 [n, {CF_EMB}, h, w] tensor, got {tuple(q.shape)}")
    if h * wd > CF_MAX_TOKENS:
        raise ValueError(f"{name}: quant_feat is {h} x {wd}: T = {h * wd} tokens, at most {CF_MAX_TOKENS} (the generator's AttnBlocks)")
    _batch_checked(name, n, _WIDEST, f"quant_feat is {tuple(q.shape)}")
    taps = {}
    if w > 0:
        given = front.get("taps")
        for s in connect:
            if not hasattr(given, "keys") or s not in given:
                raise KeyError(f"{name}: front['taps'] lacks '{s}': with w > 0 the fuse blocks read the encoder taps {list(connect)}")
            k = CF_CONNECT.index(s) + 1
            _feat_checked(name, f"taps['{s}']", given[s], (n, CF_CHANNELS[s], h << k, wd << k), q)
            taps[s] = given[s].detach().contiguous()
    return q.detach().contiguous(), taps


def codeformer_fuse(enc_feat: torch.Tensor, dec_feat: torch.Tensor, weights, size: str, w) -> torch.Tensor:
    """One ``Fuse_sft_block``: ``fuse_convs_dict[size](enc_feat, dec_feat, w)`` for two float32 ``[n, CF_CHANNELS[size], h, w]`` tensors, ``size`` one of the
    module's ``connect_list``.  It runs at any finite ``w`` (``w = 0`` gives ``dec_feat``); skipping it at ``w <= 0`` is ``codeformer_generate``'s."""
    name = "codeformer_fuse"
    w = _w_checked(name, w)
    checked = _weights_checked(name, weights)
    if size not in checked[1][5]:
        raise ValueError(f"{name}: size {size!r} is not in the connect_list {list(checked[1][5])}")
    C = CF_CHANNELS[size]
    _tensor_checked(name, "dec_feat", dec_feat, torch.float32, 4, f"a float32 [n, {C}, h, w] tensor")
    if dec_feat.shape[1] != C or dec_feat.shape[2] < 1 or dec_feat.shape[3] < 1:
        raise ValueError(f"{name}: dec_feat: expected a float32 [n, {C}, h, w] tensor, got {tuple(dec_feat.shape)}")
    _feat_checked(name, "enc_feat", enc_feat, dec_feat.shape)
    _batch_checked(name, dec_feat.shape[0], C, f"dec_feat is {tuple(dec_feat.shape)}")
    _placed(name, "dec_feat", dec_feat, checked)
    _placed(name, "enc_feat", enc_feat, checked)
    with torch.no_grad():
        F = prepare(PreparedCodeFormerGenerator, weights, checked)["fuse"][size]
        return _fuse(enc_feat.detach().contiguous(), dec_feat.detach().contiguous(), F, w)


def codeformer_generate(front, weights, w=0.8, return_feats: bool = False):
    """``out [n, 3, 32 h, 32 w]`` of the VQGAN generator on ``front['quant_feat'] [n, 256, h, w]`` with the fuse blocks of the module's ``connect_list`` on
    ``front['taps']`` at weight ``w``; ``front`` is the dict ``codeformer_front`` returns.  ``w <= 0`` skips every fuse block, as the reference's ``if w > 0``
    does: no tap is read then, and ``taps`` may be missing.  With ``return_feats``: ``(out, {size: the decoder feature behind that fuse block})`` (at
    ``w <= 0``: behind the generator block the fuse block would follow).  Refused by name before any launch: a ``w`` that is no finite Python real, a module
    in training mode, a ``quant_feat`` or tap of another dtype or shape, a tap on another device, ``n * 512 > 65535``, CPU tensors."""
    name = "codeformer_generate"
    w = _w_checked(name, w)
    checked = _weights_checked(name, weights)
    quant, taps = _front_checked(name, front, checked[1][5], w)
    _placed(name, "quant_feat", quant, checked)
    with torch.no_grad():
        out, feats = _generate(quant, taps, prepare(PreparedCodeFormerGenerator, weights, checked), w)
    return (out, feats) if return_feats else out


def codeformer_restore(x: torch.Tensor, weights, w=0.8, adain: bool = True):
    """``(out, logits, lq_feat)`` of ``x [n, 3, H, W]``: what ``CodeFormer.forward(x, w, adain=adain)`` returns, ``codeformer_front`` then
    ``codeformer_generate``, with both halves' arguments checked before the first launch."""
    name = "codeformer_restore"
    w = _w_checked(name, w)
    checked = _weights_checked(name, weights)
    _image_checked(name, x, checked[1], adain)
    _batch_checked(name, x.shape[0], _WIDEST, f"x is {tuple(x.shape)}")
    _placed(name, "x", x, checked)
    with torch.no_grad():
        f = _front_run(x, weights, checked, adain)
        out, _ = _generate(f["quant_feat"], f["taps"], prepare(PreparedCodeFormerGenerator, weights, checked), w)
    return out, f["logits"], f["lq_feat"]


__all__ = ["PreparedCodeFormerGenerator", "GENERATOR_PLAN", "CF_FUSE_BLOCKS", "sft_fuse", "image_u8", "codeformer_fuse", "codeformer_generate", "codeformer_restore"]
