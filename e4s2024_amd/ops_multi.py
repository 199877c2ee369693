"""Shared pieces of the multi-target loss terms (``ops_lpips.lpips_multiscale_multi``, ``ops_id.id_loss_multi``, ``ops_fp.fp_loss_multi``) and the
pixel term ``mse_multi``: one reconstruction against k <= 4 targets, each with its own weight, on the multi-target heads of ``include/e4s_hip.h``.

PTI compares one reconstruction with the driven frame and with the recoloured driven frame (training/video_swap_ft_coach.py:274-287).  Both terms see the
same input, so each loss network runs its forward pass and input gradient once; only the heads read the k targets' features.  Target features are
tensors with ``rows`` samples: the batch of the step (``frame=None``), or ``n`` frames x batch from a clip-wide cache, one of which a device int32
``frame`` selects (a captured step picks its frame by writing that scalar before the replay, with no copy of the features)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from ._lib import MAX_TARGETS, lib, targets as _host_targets
from .ops import _c, _p, _stream


def check_frame(frame: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    """``frame``: None or a one-element int32 tensor on ``device``."""
    if frame is None:
        return None
    if not isinstance(frame, torch.Tensor) or frame.dtype != torch.int32 or frame.numel() != 1 or frame.device != torch.device(device):
        raise ValueError("frame: expected a one-element int32 tensor on the device of the images")
    return frame


def check_targets(taps: Sequence[torch.Tensor], targets, tw, frame, what: str):
    """Checks ``targets`` (k lists of tensors, one per tap of ``taps``) against the reconstruction's taps (the same per-sample shape; ``bs`` rows
    without ``frame``, a multiple of ``bs`` with one) and returns them as contiguous fp32 lists."""
    k = len(targets)
    if not 1 <= k <= MAX_TARGETS or len(tw) != k:
        raise ValueError(f"{what}: 1 .. {MAX_TARGETS} targets with one weight each, got {k} targets and {len(tw)} weights")
    bs = taps[0].shape[0]
    out = []
    for j, tg in enumerate(targets):
        if len(tg) != len(taps):
            raise ValueError(f"{what}: target {j} has {len(tg)} feature tensors, expected {len(taps)}")
        row = []
        for t, (a, y) in enumerate(zip(taps, tg)):
            y = _c(y, f"{what} target {j} tap {t}")
            rows = y.shape[0]
            if y.shape[1:] != a.shape[1:] or (rows != bs if frame is None else (rows < bs or rows % bs)):
                raise ValueError(f"{what}: target {j} tap {t} is {tuple(y.shape)}, expected {('' if frame is None else 'frames x ')}{tuple(a.shape)}")
            row.append(y)
        out.append(row)
    return out


def call_args(ys: Sequence[torch.Tensor], tw, frame: Optional[torch.Tensor], bs: int):
    """``(ys, tw, k, frame, fstride, nframes)`` of a multi-target entry point for the targets ``ys`` of one tap (fstride: elements per frame; the
    kernels clamp the device frame index to [0, nframes), so a bad index reads a wrong frame of the cache but never past it)."""
    ptrs, ws, k = _host_targets([y.data_ptr() for y in ys], tw)
    fstride = bs * (ys[0][0].numel()) if frame is not None else 0
    nframes = min(y.shape[0] for y in ys) // bs if frame is not None else 1
    return ptrs, ws, k, _p(frame), fstride, nframes


def target_rows(fn, images: torch.Tensor, chunk: int = 1):
    """``fn(images[i:i + chunk])`` (a list of tensors with the chunk's samples first) for every chunk, gathered into tensors of all the samples."""
    out = None
    n = images.shape[0]
    for i in range(0, n, chunk):
        part = fn(images[i:i + chunk])
        if out is None:
            out = [torch.empty((n,) + tuple(p.shape[1:]), dtype=p.dtype, device=p.device) for p in part]
        for dst, src in zip(out, part):
            dst[i:i + src.shape[0]].copy_(src)
    return out


PX_CHUNK = 4096                               # e4s_pix_mse_multi: pixels of a plane per partial sum


class _MseMulti(torch.autograd.Function):
    """sum_j w_j mean((x fg - y_j)^2) with the gradient with respect to ``x``."""

    @staticmethod
    def forward(ctx, x, fg, ys, tw, frame):
        bs, c, h, w = x.shape
        partial = torch.empty((bs * c * -(-(h * w) // PX_CHUNK),), dtype=torch.float32, device=x.device)
        lib().call("e4s_pix_mse_multi", _p(partial), _p(x), _p(fg), *call_args(ys, tw, frame, bs), bs, c, h * w, _stream())
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        lib().call("e4s_lpips_sum", _p(loss), _p(partial), partial.numel(), _stream())
        ctx.fg, ctx.ys, ctx.tw, ctx.frame = fg, ys, tw, frame
        ctx.save_for_backward(x)
        return loss

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        bs, c, h, w = x.shape
        gx = torch.empty_like(x)
        gout = _c(gout.reshape(1), "grad_output")
        lib().call("e4s_pix_mse_multi_bwd", _p(gx), _p(x), _p(ctx.fg), *call_args(ctx.ys, ctx.tw, ctx.frame, bs), _p(gout), bs, c, h * w, _stream())
        return gx, None, None, None, None


def mse_multi(x: torch.Tensor, foreground_mask: Optional[torch.Tensor], targets: Sequence[torch.Tensor], tw, frame: Optional[torch.Tensor] = None):
    """``sum_j tw[j] * mse_loss(x * fg, targets[j])`` (0-d, differentiable in ``x``): the pixel term of calc_loss (:196-199) against k targets at once.
    ``targets[j]``: the target images ALREADY multiplied by the foreground weight, ``[bs, 3, H, W]`` (or frames x bs rows with ``frame``);
    ``foreground_mask`` ``[bs, 1, H, W]`` or None (weight 1)."""
    x = _c(x, "x")
    if x.dim() != 4:
        raise ValueError(f"x: expected [bs, C, H, W], got {tuple(x.shape)}")
    fg = None
    if foreground_mask is not None:
        fg = _c(foreground_mask, "foreground_mask")
        if fg.shape != (x.shape[0], 1) + tuple(x.shape[2:]):
            raise ValueError(f"foreground_mask: expected {(x.shape[0], 1) + tuple(x.shape[2:])}, got {tuple(fg.shape)}")
    frame = check_frame(frame, x.device)
    ys = [row[0] for row in check_targets([x], [[t] for t in targets], tw, frame, "mse_multi")]
    return _MseMulti.apply(x, fg, ys, [float(w) for w in tw], frame)


__all__ = ["check_frame", "check_targets", "call_args", "target_rows", "mse_multi"]
