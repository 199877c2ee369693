"""The pixel term of the multi-target PTI objective: ``mse_multi``, one reconstruction against k <= 4 targets, each with its own weight, on
``e4s_pix_mse_multi`` of ``include/e4s_hip.h``.  The checks and call arguments it shares with the multi-target loss-network terms
(``ops_lpips.lpips_multiscale_multi``, ``ops_id.id_loss_multi``, ``ops_fp.fp_loss_multi``) live in ``lossnet`` and are re-exported here."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from ._lib import lib
from .lossnet import call_args, check_frame, check_targets, sum_partials, target_rows
from .ops import _c, _p, _stream


PX_CHUNK = 4096                               # e4s_pix_mse_multi: pixels of a plane per partial sum


class _MseMulti(torch.autograd.Function):
    """sum_j w_j mean((x fg - y_j)^2) with the gradient with respect to ``x``."""

    @staticmethod
    def forward(ctx, x, fg, ys, tw, frame):
        bs, c, h, w = x.shape
        partial = torch.empty((bs * c * -(-(h * w) // PX_CHUNK),), dtype=torch.float32, device=x.device)
        lib().call("e4s_pix_mse_multi", _p(partial), _p(x), _p(fg), *call_args(ys, tw, frame, bs), bs, c, h * w, _stream())
        loss = sum_partials(partial, partial.numel())
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
