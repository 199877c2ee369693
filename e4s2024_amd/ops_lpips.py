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
The weight cache, the split-bf16 weight preparation and convolution wrapper and the multi-target helpers are ``lossnet``'s.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import lossnet
from ._lib import lib
from .lossnet import call_args, check_frame, check_image, check_targets, conv_sb, relu_mask, sum_partials, target_rows, weights_key
from .ops import _Prepared, _c, _p, _stream

LAYERS = (0, 3, 6, 8, 10)                 # AlexNet ``features`` indices of the five convolutions
CHANNELS = (64, 192, 384, 256, 256)
KERNELS = (11, 5, 3, 3, 3)
PADS = (2, 2, 1, 1, 1)
MIN_SIDE = 31                             # the smallest (scaled) side for which every layer has an output


def state_dict_keys():
    """The keys of the drop-in ``LPIPS`` module's ``state_dict``, in its order."""
    return ["net.mean", "net.std"] + [f"net.layers.{i}.{n}" for i in LAYERS for n in ("weight", "bias")] + [f"lin.{i}.1.weight" for i in range(5)]


def check_loaded(weights):
    """``weights`` itself; raises if it is a module that has never had its weights loaded (the drop-in ``LPIPS`` / ``BaseNet`` start
    without weights and never download: a loss from their initial parameters would be a silently wrong objective)."""
    if isinstance(weights, torch.nn.Module) and getattr(weights, "_loaded", True) is False:
        raise RuntimeError(f"{type(weights).__name__}: weights were never loaded (nothing is downloaded here); call load_state_dict first")
    return weights


def _tensors(weights):
    """(the 12 network tensors, the 5 lin weights) of ``weights``: an ``LPIPS`` module, its ``net`` (then no lin weights) or a mapping."""
    check_loaded(weights)
    if isinstance(weights, torch.nn.Module):
        weights = weights.state_dict()
    keys = state_dict_keys()
    if "net.mean" not in weights and "mean" in weights:                  # a BaseNet's own state_dict
        weights = {"net." + k: v for k, v in weights.items()}
        keys = keys[:12]
    try:
        ts = [weights[k] for k in keys]
    except KeyError as e:
        raise KeyError(f"LPIPS weights lack {e}: expected the keys {state_dict_keys()}") from None
    return ts[:12], ts[12:]


def weight_tensors(weights):
    """The network and lin tensors of ``weights`` (see ``weights_key``)."""
    net, lin = _tensors(weights)
    return net + lin


class PreparedLpips(_Prepared):
    """The kernels' copies of the LPIPS weights, rebuilt when a tensor changes version or storage: conv1's weight with the output channel
    innermost, three-way split slabs of conv2..5 (forward) and two-way split slabs of their flipped, transposed weights (data gradient)."""

    __slots__ = ()

    def get(self, weights):
        ts = _tensors(weights)[0]
        key = weights_key(ts) + (ts[0].device,)
        hit = self._lookup(key)
        if hit is not None:
            return hit
        ts = [_c(t.detach(), k) for t, k in zip(ts, state_dict_keys())]
        mean, std = ts[0].reshape(3).contiguous(), ts[1].reshape(3).contiguous()
        ws, bs = ts[2:12:2], ts[3:12:2]
        for i, (w, b) in enumerate(zip(ws, bs)):
            cin = 3 if i == 0 else CHANNELS[i - 1]
            if tuple(w.shape) != (CHANNELS[i], cin, KERNELS[i], KERNELS[i]) or tuple(b.shape) != (CHANNELS[i],):
                raise ValueError(f"net.layers.{LAYERS[i]}: weight {tuple(w.shape)} / bias {tuple(b.shape)} is not AlexNet's")
        w1t = ws[0].permute(1, 2, 3, 0).contiguous()                   # [3][11][11][64]
        fwd, bwd = [], []
        for w in ws[1:]:
            fwd.append(lossnet.prep_fwd(w)[0])
            bwd.append(lossnet.prep_dgrad(w))                  # the data gradient is a convolution with the flipped, transposed weights
        payload = (mean, std, w1t, tuple(bs), tuple(fwd), tuple(bwd))
        return self._publish(key, payload)


def prepare(weights):
    """Prepared copies for ``weights`` (cached on a module; a plain mapping is prepared on every call)."""
    return lossnet.prepare(PreparedLpips, weights)


def lin_weights(weights):
    """The five ``lin`` weights of ``weights`` as flat fp32 vectors (views)."""
    out = []
    for i, t in enumerate(_tensors(weights)[1]):
        if tuple(t.shape) != (1, CHANNELS[i], 1, 1):
            raise ValueError(f"lin.{i}.1.weight: {tuple(t.shape)}, expected (1, {CHANNELS[i]}, 1, 1)")
        out.append(_c(t.detach(), f"lin.{i}.1.weight").reshape(-1))
    return out


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
    check_loaded(weights)
    if not 1 <= scales <= 3:
        raise ValueError(f"scales must be 1, 2 or 3, got {scales}")
    for i in range(scales):
        _check(images, "images", 1 << i)
    P = prepare(weights)
    with torch.no_grad():
        return target_rows(lambda x: [t for i in range(scales) for t in _features(x.contiguous(), P, 1 << i)], images.detach())


def lpips_multiscale_multi(x: torch.Tensor, targets, tw, weights, frame: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sum_j tw[j] * lpips_multiscale(x, y_j)`` (0-d, differentiable in ``x`` only) with one AlexNet forward pass and input gradient of ``x``:
    ``targets[j] = target_features(y_j, weights)`` (``bs`` rows, or frames x ``bs`` rows with ``frame``, a device int32 frame index)."""
    check_loaded(weights)
    x = _check(x, "x", 1)
    scales = len(targets[0]) // 5 if targets else 0
    if not 1 <= scales <= 3 or any(len(t) != 5 * scales for t in targets):
        raise ValueError("targets: each must be a target_features list of 5, 10 or 15 taps")
    for i in range(scales):
        _check(x, "x", 1 << i)
    frame = check_frame(frame, x.device)
    P, lins = prepare(weights), lin_weights(weights)
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
    check_loaded(weights)
    x = _check(x, "x", factor)
    with torch.no_grad():
        taps = _features(x, prepare(weights), factor)
    return [t / (torch.sqrt((t * t).sum(1, keepdim=True) + 1e-16) + 1e-10) for t in taps]


def _check(x: torch.Tensor, name: str, factor: int) -> torch.Tensor:
    x = check_image(x, name)
    h, w = x.shape[2], x.shape[3]
    if h % factor or w % factor:
        raise ValueError(f"{name}: the sides {h} x {w} must be divisible by {factor}")
    if min(h, w) // factor < MIN_SIDE:
        raise ValueError(f"{name}: {h} x {w} / {factor} is smaller than AlexNet's {MIN_SIDE} x {MIN_SIDE} minimum")
    return x


def lpips(x: torch.Tensor, y: torch.Tensor, weights, factor: int = 1) -> torch.Tensor:
    """``LPIPS(boxmean_f(x), boxmean_f(y))`` (a 0-d tensor): ``x``, ``y`` fp32 ``[bs, 3, H, W]`` on the device, the sides divisible by ``factor``
    (1, 2 or 4: the exact f x f box mean is ``adaptive_avg_pool2d`` to ``H / f``).  Differentiable in ``x`` and ``y``."""
    check_loaded(weights)
    if factor not in (1, 2, 4):
        raise ValueError(f"factor must be 1, 2 or 4, got {factor}")
    x, y = _check(x, "x", factor), _check(y, "y", factor)
    if x.shape != y.shape:
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} differ")
    return _LpipsScale.apply(x, y, prepare(weights), lin_weights(weights), factor)


def lpips_multiscale(x: torch.Tensor, y: torch.Tensor, weights, scales: int = 3, foreground_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sum_{i < scales} LPIPS(boxmean_{2^i}(x), boxmean_{2^i}(y))`` — the perceptual term of calc_loss (video_swap_ft_coach.py:201-211 at
    1024 x 1024: ``adaptive_avg_pool2d(., 1024 // 2**i)``).  ``foreground_mask`` (broadcast over channels): both images are multiplied by it
    first, as the video coach does (:188-190)."""
    check_loaded(weights)
    if not 1 <= scales <= 3:
        raise ValueError(f"scales must be 1, 2 or 3, got {scales}")
    if foreground_mask is not None:
        x, y = x * foreground_mask, y * foreground_mask
    loss = None
    for i in range(scales):
        t = lpips(x, y, weights, 1 << i)
        loss = t if loss is None else loss + t
    return loss


__all__ = ["PreparedLpips", "check_loaded", "weights_key", "weight_tensors", "prepare", "lin_weights", "features", "lpips", "lpips_multiscale", "state_dict_keys", "LAYERS", "CHANNELS",
           "target_features", "lpips_multiscale_multi"]
