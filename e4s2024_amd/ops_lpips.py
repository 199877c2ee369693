"""LPIPS-AlexNet (``criteria/lpips``: lpips.py:28-34, networks.py:47-56 + 76-84, utils.py:6-9) on the HIP kernels: forward and gradient with
respect to the input image, for the perceptual term of the PTI and W-optimisation loops (training/video_swap_ft_coach.py:201-211,
optimization.py:111-146).

    conv1 (11x11 s4) + ReLU      csrc/lpips.hip, fp32, z-score and the f x f box mean of the scale fused into its load
    maxpool 3x3 s2               csrc/lpips.hip (backward: a gather fused with the tap's head gradient and the ReLU mask)
    conv2 (5x5) .. conv5 (3x3)   csrc/conv.hip, three-way split-bf16 (fp32-class: the 1 / |f| of the head amplifies forward error in the gradient)
    data gradients of conv2..5   csrc/conv.hip, two-way split-bf16 on the flipped, transposed weights (prepared once per weight version)
    head                         csrc/lpips.hip, per tap; per-workgroup partial sums reduced in a fixed order (bit-identical reruns)

Weights are a ``state_dict``-shaped mapping or a module with the reference's layout: ``net.mean``, ``net.std``,
``net.layers.{0,3,6,8,10}.{weight,bias}``, ``lin.{0..4}.1.weight``.  They are frozen: no weight gradient is computed.
Every launch goes on the current stream with no host synchronisation, so the term can be captured in a hipGraph (``pti.GraphedPTIStep``).
Validation of the weights (keys, shapes, dtypes: once per public call) and the cache of their prepared copies are ``netweights``', as for every
network of the package; the split-bf16 weight preparation and convolution wrapper and the multi-target helpers are ``lossnet``'s.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import lossnet, netweights
from ._lib import lib
from .lossnet import call_args, check_frame, check_image, check_targets, conv_sb, relu_mask, sum_partials, target_rows
from .netweights import PreparedNet, _Net, _validated, weights_key
from .ops import _c, _p, _stream

LAYERS = (0, 3, 6, 8, 10)                 # AlexNet ``features`` indices of the five convolutions
CHANNELS = (64, 192, 384, 256, 256)
KERNELS = (11, 5, 3, 3, 3)
PADS = (2, 2, 1, 1, 1)
MIN_SIDE = 31                             # the smallest (scaled) side for which every layer has an output


def state_dict_keys():
    """The keys of the drop-in ``LPIPS`` module's ``state_dict``, in its order."""
    return ["net.mean", "net.std"] + [f"net.layers.{i}.{n}" for i in LAYERS for n in ("weight", "bias")] + [f"lin.{i}.1.weight" for i in range(5)]


def state_dict_shapes(full: bool = True):
    """``{key: shape}`` of the drop-in ``LPIPS`` module's ``state_dict`` or, with ``full`` False, of its ``net`` alone (a ``BaseNet``: the 12 network
    tensors under their bare names, no ``lin``)."""
    p = "net." if full else ""
    out = {p + "mean": (1, 3, 1, 1), p + "std": (1, 3, 1, 1)}
    for i, (layer, c, k) in enumerate(zip(LAYERS, CHANNELS, KERNELS)):
        out[f"{p}layers.{layer}.weight"], out[f"{p}layers.{layer}.bias"] = (c, 3 if i == 0 else CHANNELS[i - 1], k, k), (c,)
    if full:
        out.update({f"lin.{i}.1.weight": (1, c, 1, 1) for i, c in enumerate(CHANNELS)})
    return out


def _full(name, sd):
    """True for the keys of an ``LPIPS``, False for those of its ``net`` alone (without either, ``mean`` is reported as missing)."""
    return "net.mean" in sd


_LPIPS_NET = _Net("LPIPS", state_dict_shapes, (), False, ("net.mean", "mean"), _full, None, ())


def check_loaded(weights):
    """``weights`` itself; raises if it is a module that has never had its weights loaded (the drop-in ``LPIPS`` / ``BaseNet`` start
    without weights and never download: a loss from their initial parameters would be a silently wrong objective)."""
    netweights.check_loaded(None, weights, "weights")
    return weights


def _checked(name, weights):
    """What ``_validated`` returns of ``weights``: what a public call makes once, before it looks at its images, and hands to ``netweights.prepare``
    and ``lin_weights``.  Refused in this order: weights never loaded, a missing key, a wrong shape or dtype."""
    netweights.check_loaded(name, weights, "weights")
    return _validated(name, weights, _LPIPS_NET)


def weight_tensors(weights, name: str = "lpips"):
    """The network and lin tensors of ``weights``, their shapes checked (see ``weights_key``)."""
    return _checked(name, weights)[2]


class PreparedLpips(PreparedNet):
    """The kernels' copies of the LPIPS weights, rebuilt when a tensor changes version or storage: conv1's weight with the output channel
    innermost, three-way split slabs of conv2..5 (forward) and two-way split slabs of their flipped, transposed weights (data gradient).
    Keyed on every tensor ``weights`` has, the five ``lin`` weights of a full ``LPIPS`` included although no copy of them is kept: the weights
    are frozen, so the wider key costs no rebuild."""

    __slots__ = ()
    _entry, _net = "lpips", _LPIPS_NET

    def _build(self, sd, full, dev):
        p = "net." if full else ""
        mean, std = sd[p + "mean"].reshape(3).contiguous(), sd[p + "std"].reshape(3).contiguous()
        ws, bs = [sd[f"{p}layers.{i}.weight"] for i in LAYERS], [sd[f"{p}layers.{i}.bias"] for i in LAYERS]
        w1t = ws[0].permute(1, 2, 3, 0).contiguous()                   # [3][11][11][64]
        fwd, bwd = [], []
        for w in ws[1:]:
            fwd.append(lossnet.prep_fwd(w)[0])
            bwd.append(lossnet.prep_dgrad(w))                  # the data gradient is a convolution with the flipped, transposed weights
        return mean, std, w1t, tuple(bs), tuple(fwd), tuple(bwd)


def prepare(weights):
    """Prepared copies for ``weights`` (cached on a module; a plain mapping is prepared on every call)."""
    return netweights.prepare(PreparedLpips, weights, _checked("lpips", weights))


def lin_weights(weights, checked=None, name: str = "lpips"):
    """The five ``lin`` weights of ``weights`` as flat fp32 vectors (views); ``checked``: what the caller's own validation of ``weights`` returned.
    Weights without them (a ``BaseNet``'s) are refused."""
    sd, full, _ = checked if checked is not None else _checked(name, weights)
    if not full:
        raise KeyError(f"{name}: the weights lack 'lin.0.1.weight': the loss needs the keys of LPIPS (ops_lpips.state_dict_shapes()), a BaseNet's give the "
                       "features alone")
    return [_c(sd[f"lin.{i}.1.weight"].detach(), f"lin.{i}.1.weight").reshape(-1) for i in range(5)]


def _checked_with_lins(name, weights):
    """(``_checked``'s triple, the lin weights): the weights of a call that computes the loss, refused before its images are looked at."""
    checked = _checked(name, weights)
    return checked, lin_weights(weights, checked, name)


def _conv_out(side: int, i: int) -> int:
    return (side + 2 * PADS[i] - KERNELS[i]) // (4 if i == 0 else 1) + 1


def _pool_out(side: int) -> int:
    return (side - 3) // 2 + 1


def _conv(x, slabs, bias, i: int, relu: bool, residual=None):
    return conv_sb(x, slabs, bias, k=KERNELS[i], pad=PADS[i], relu=relu, residual=residual)      # stride 1, "same" padding


def _maxpool(a):
    bs, c, h, w = a.shape
    out = torch.empty((bs, c, _pool_out(h), _pool_out(w)), dtype=torch.float32, device=a.device)
    lib().call("e4s_lpips_maxpool", _p(out), _p(a), bs * c, h, w, _stream())
    return out


def _features(x, P, f: int):
    """The five ReLU outputs (taps) of AlexNet on the z-scored f x f box mean of ``x``."""
    mean, std, w1t, biases, fwd, _ = P
    bs, _, h, w = x.shape
    a1 = torch.empty((bs, 64, _conv_out(h // f, 0), _conv_out(w // f, 0)), dtype=torch.float32, device=x.device)
    lib().call("e4s_lpips_conv1", _p(a1), _p(x), _p(mean), _p(std), _p(w1t), _p(biases[0]), bs, h, w, f, _stream())
    a2 = _conv(_maxpool(a1), fwd[0], biases[1], 1, True)
    a3 = _conv(_maxpool(a2), fwd[1], biases[2], 2, True)
    a4 = _conv(a3, fwd[2], biases[3], 3, True)
    a5 = _conv(a4, fwd[3], biases[4], 4, True)
    return [a1, a2, a3, a4, a5]


def _head(fx, fy, lins):
    bs = fx[0].shape[0]
    counts = [bs * ((a.shape[2] * a.shape[3] + 31) // 32) for a in fx]      # e4s_lpips_head: one partial per 32 pixels
    partial = torch.empty((sum(counts),), dtype=torch.float32, device=fx[0].device)
    off = 0
    for a, b, lin, n in zip(fx, fy, lins, counts):
        hw = a.shape[2] * a.shape[3]
        lib().call("e4s_lpips_head", _p(partial[off:]), _p(a), _p(b), _p(lin), bs, a.shape[1], hw, 1.0 / (bs * hw), _stream())
        off += n
    return sum_partials(partial, off)


def _input_grad(taps, gtaps, P, f: int, shape):
    """d loss / d image from the head's gradients ``gtaps`` at the five taps (overwritten)."""
    _, std, w1t, _, _, bwd = P
    a1, a2, a3, a4, a5 = taps
    g5 = gtaps[4]
    relu_mask(g5, a5)
    g4 = _conv(g5, bwd[3], None, 4, False, residual=gtaps[3])
    relu_mask(g4, a4)
    g3 = _conv(g4, bwd[2], None, 3, False, residual=gtaps[2])
    relu_mask(g3, a3)
    gp2 = _conv(g3, bwd[1], None, 2, False)
    g2 = torch.empty_like(a2)
    lib().call("e4s_lpips_maxpool_bwd_relu", _p(g2), _p(gp2), _p(gtaps[1]), _p(a2), a2.shape[0] * a2.shape[1], a2.shape[2], a2.shape[3], _stream())
    gp1 = _conv(g2, bwd[0], None, 1, False)
    g1 = torch.empty_like(a1)
    lib().call("e4s_lpips_maxpool_bwd_relu", _p(g1), _p(gp1), _p(gtaps[0]), _p(a1), a1.shape[0] * a1.shape[1], a1.shape[2], a1.shape[3], _stream())
    gx = torch.empty(shape, dtype=torch.float32, device=a1.device)
    lib().call("e4s_lpips_conv1_dgrad", _p(gx), _p(g1), _p(std), _p(w1t), shape[0], shape[2], shape[3], f, _stream())
    return gx


class _LpipsScale(torch.autograd.Function):
    """LPIPS(boxmean_f(x), boxmean_f(y)) with the gradient with respect to ``x`` (and ``y`` when it needs one)."""

    @staticmethod
    def forward(ctx, x, y, P, lins, f):
        fx = _features(x, P, f)
        fy = _features(y, P, f)
        ctx.P, ctx.lins, ctx.f, ctx.shape = P, lins, f, tuple(x.shape)
        ctx.save_for_backward(*fx, *fy)
        return _head(fx, fy, lins)

    @staticmethod
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        fx, fy = list(saved[:5]), list(saved[5:])
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gout = _c(gout.reshape(1), "grad_output")
        gxt = [torch.empty_like(a) for a in fx] if need_x else None
        gyt = [torch.empty_like(a) for a in fy] if need_y else None
        for k in range(5):
            a, b = fx[k], fy[k]
            hw = a.shape[2] * a.shape[3]
            dst_x = gxt[k] if need_x else torch.empty_like(a)
            lib().call("e4s_lpips_head_bwd", _p(dst_x), _p(gyt[k]) if need_y else None, _p(a), _p(b), _p(ctx.lins[k]), _p(gout), a.shape[0], a.shape[1],
                       hw, 1.0 / (a.shape[0] * hw), _stream())
        gx = _input_grad(fx, gxt, ctx.P, ctx.f, ctx.shape) if need_x else None
        gy = _input_grad(fy, gyt, ctx.P, ctx.f, ctx.shape) if need_y else None
        return gx, gy, None, None, None


class _LpipsScaleMulti(torch.autograd.Function):
    """sum_j tw[j] LPIPS(boxmean_f(x), target j) from the targets' cached taps; the gradient with respect to ``x`` only."""

    @staticmethod
    def forward(ctx, x, P, lins, f, ys, tw, frame):
        fx = _features(x, P, f)
        bs = x.shape[0]
        counts = [bs * ((a.shape[2] * a.shape[3] + 31) // 32) for a in fx]
        partial = torch.empty((sum(counts),), dtype=torch.float32, device=x.device)
        off = 0
        for t, (a, lin, n) in enumerate(zip(fx, lins, counts)):
            hw = a.shape[2] * a.shape[3]
            lib().call("e4s_lpips_head_multi", _p(partial[off:]), _p(a), *call_args([y[t] for y in ys], tw, frame, bs), _p(lin), bs, a.shape[1], hw,
                       1.0 / (bs * hw), _stream())
            off += n
        loss = sum_partials(partial, off)
        ctx.P, ctx.lins, ctx.f, ctx.shape, ctx.ys, ctx.tw, ctx.frame = P, lins, f, tuple(x.shape), ys, tw, frame
        ctx.save_for_backward(*fx)
        return loss

    @staticmethod
    def backward(ctx, gout):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None, None
        fx = list(ctx.saved_tensors)
        gout = _c(gout.reshape(1), "grad_output")
        gxt = [torch.empty_like(a) for a in fx]
        for t, a in enumerate(fx):
            hw = a.shape[2] * a.shape[3]
            lib().call("e4s_lpips_head_multi_bwd", _p(gxt[t]), _p(a), *call_args([y[t] for y in ctx.ys], ctx.tw, ctx.frame, a.shape[0]), _p(ctx.lins[t]),
                       _p(gout), a.shape[0], a.shape[1], hw, 1.0 / (a.shape[0] * hw), _stream())
        return _input_grad(fx, gxt, ctx.P, ctx.f, ctx.shape), None, None, None, None, None, None


def target_features(images: torch.Tensor, weights, scales: int = 3):
    """The raw AlexNet taps of ``images`` ``[n, 3, H, W]`` at the ``scales`` box-mean factors 1, 2, 4 — what ``lpips_multiscale_multi`` reads for a target:
    a flat list, scale-major (five taps per scale), of tensors ``[n, C, h, w]``.  Computed a frame at a time; no gradient."""
    checked = _checked("ops_lpips.target_features", weights)
    if not 1 <= scales <= 3:
        raise ValueError(f"scales must be 1, 2 or 3, got {scales}")
    for i in range(scales):
        _check(images, "images", 1 << i)
    P = netweights.prepare(PreparedLpips, weights, checked)
    with torch.no_grad():
        return target_rows(lambda x: [t for i in range(scales) for t in _features(x.contiguous(), P, 1 << i)], images.detach())


def lpips_multiscale_multi(x: torch.Tensor, targets, tw, weights, frame: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sum_j tw[j] * lpips_multiscale(x, y_j)`` (0-d, differentiable in ``x`` only) with one AlexNet forward pass and input gradient of ``x``:
    ``targets[j] = target_features(y_j, weights)`` (``bs`` rows, or frames x ``bs`` rows with ``frame``, a device int32 frame index)."""
    checked, lins = _checked_with_lins("lpips_multiscale_multi", weights)
    x = _check(x, "x", 1)
    scales = len(targets[0]) // 5 if targets else 0
    if not 1 <= scales <= 3 or any(len(t) != 5 * scales for t in targets):
        raise ValueError("targets: each must be a target_features list of 5, 10 or 15 taps")
    for i in range(scales):
        _check(x, "x", 1 << i)
    frame = check_frame(frame, x.device)
    P = netweights.prepare(PreparedLpips, weights, checked)
    loss = None
    for i in range(scales):
        f = 1 << i
        shapes = [(x.shape[0], c, side_h, side_w) for c, side_h, side_w in _tap_shapes(x.shape[2] // f, x.shape[3] // f)]
        ys = check_targets([torch.empty(s, device="meta") for s in shapes], [t[5 * i:5 * i + 5] for t in targets], tw, frame, "lpips_multiscale_multi")
        t = _LpipsScaleMulti.apply(x, P, lins, f, ys, [float(w) for w in tw], frame)
        loss = t if loss is None else loss + t
    return loss


def _tap_shapes(h: int, w: int):
    """(C, h, w) of the five taps of an h x w (scaled) image."""
    h1, w1 = _conv_out(h, 0), _conv_out(w, 0)
    h2, w2 = _pool_out(h1), _pool_out(w1)
    h3, w3 = _pool_out(h2), _pool_out(w2)
    return [(CHANNELS[0], h1, w1), (CHANNELS[1], h2, w2), (CHANNELS[2], h3, w3), (CHANNELS[3], h3, w3), (CHANNELS[4], h3, w3)]


def features(x: torch.Tensor, weights, factor: int = 1):
    """The five normalised AlexNet taps of ``x`` (``BaseNet.forward``; no gradient).  ``weights``: a ``BaseNet`` / ``LPIPS`` module or mapping."""
    checked = _checked("ops_lpips.features", weights)
    x = _check(x, "x", factor)
    with torch.no_grad():
        taps = _features(x, netweights.prepare(PreparedLpips, weights, checked), factor)
    return [t / (torch.sqrt((t * t).sum(1, keepdim=True) + 1e-16) + 1e-10) for t in taps]


def _check(x: torch.Tensor, name: str, factor: int) -> torch.Tensor:
    x = check_image(x, name)
    h, w = x.shape[2], x.shape[3]
    if h % factor or w % factor:
        raise ValueError(f"{name}: the sides {h} x {w} must be divisible by {factor}")
    if min(h, w) // factor < MIN_SIDE:
        raise ValueError(f"{name}: {h} x {w} / {factor} is smaller than AlexNet's {MIN_SIDE} x {MIN_SIDE} minimum")
    return x


def _lpips(x, y, weights, checked, lins, factor):
    """``lpips`` on weights its caller has validated."""
    if factor not in (1, 2, 4):
        raise ValueError(f"factor must be 1, 2 or 4, got {factor}")
    x, y = _check(x, "x", factor), _check(y, "y", factor)
    if x.shape != y.shape:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} differ")
    return _LpipsScale.apply(x, y, netweights.prepare(PreparedLpips, weights, checked), lins, factor)


def lpips(x: torch.Tensor, y: torch.Tensor, weights, factor: int = 1) -> torch.Tensor:
    """``LPIPS(boxmean_f(x), boxmean_f(y))`` (a 0-d tensor): ``x``, ``y`` fp32 ``[bs, 3, H, W]`` on the device, the sides divisible by ``factor``
    (1, 2 or 4: the exact f x f box mean is ``adaptive_avg_pool2d`` to ``H / f``).  Differentiable in ``x`` and ``y``."""
    return _lpips(x, y, weights, *_checked_with_lins("lpips", weights), factor)


def lpips_multiscale(x: torch.Tensor, y: torch.Tensor, weights, scales: int = 3, foreground_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sum_{i < scales} LPIPS(boxmean_{2^i}(x), boxmean_{2^i}(y))`` — the perceptual term of calc_loss (video_swap_ft_coach.py:201-211 at
    1024 x 1024: ``adaptive_avg_pool2d(., 1024 // 2**i)``).  ``foreground_mask`` (broadcast over channels): both images are multiplied by it
    first, as the video coach does (:188-190)."""
    checked, lins = _checked_with_lins("lpips_multiscale", weights)
    if not 1 <= scales <= 3:
        raise ValueError(f"scales must be 1, 2 or 3, got {scales}")
    if foreground_mask is not None:
        x, y = x * foreground_mask, y * foreground_mask
    loss = None
    for i in range(scales):
        t = _lpips(x, y, weights, checked, lins, 1 << i)
        loss = t if loss is None else loss + t
    return loss


__all__ = ["PreparedLpips", "check_loaded", "weights_key", "weight_tensors", "prepare", "lin_weights", "features", "lpips", "lpips_multiscale", "state_dict_keys",
           "state_dict_shapes", "LAYERS", "CHANNELS",
           "target_features", "lpips_multiscale_multi"]
