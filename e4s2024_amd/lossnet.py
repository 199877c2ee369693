"""What the frozen loss networks of the PTI objective (``ops_lpips``, ``ops_id``, ``ops_fp``) have in common on the host side, and what the stage networks
(``ops_recolor``, ``ops_rrdb``, ``ops_parsenet``, ``ops_retinaface``, ``ops_reenact``, and through ``sg2net`` the two StyleGAN2 generators ``ops_gpen`` and
``ops_inpaint``) take from it: BatchNorm folding, weight preparation for and the calls of the convolutions of csrc/conv.hip (split-bf16: ``prep_fwd`` / ``prep_dgrad`` / ``conv_sb``; exact float32:
``prep_exact`` / ``conv_exact``), the banded resampler of csrc/idloss.hip and its adjoint, the cosine heads, two small kernels, and the checks and call
arguments of the multi-target heads.  Taking a network's weights from a caller (validation, the cache of prepared copies) is ``netweights``'.  The library is
resolved inside the calls only, so the module imports on a machine without it.

Multi-target terms: PTI compares one reconstruction with the driven frame and with the recoloured driven frame (training/video_swap_ft_coach.py:274-287).
Both terms see the same input, so each loss network runs its forward pass and input gradient once; only the heads read the k <= 4 targets' features.
Target features are tensors with ``rows`` samples: the batch of the step (``frame=None``), or ``n`` frames x batch from a clip-wide cache, one of
which a device int32 ``frame`` selects (a captured step picks its frame by writing that scalar before the replay, with no copy of the features)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import MAX_TARGETS, lib, targets as _host_targets
from .ops import _c, _p, _stream

BN_EPS = 1e-5
HEAD_BLOCK = 8192                            # e4s_id_head_partial: elements per partial sum
MULTI_STATS = 1 + 2 * MAX_TARGETS            # e4s_id_head_*_multi: |x|^2 (|x|), then (|y_j|^2, x.y_j) ((|y_j|, cos_j)) per target


# ------------------------------------------------------------------------------------------------ weights
def bn_fold(sd, prefix):
    """Eval-mode BatchNorm as float64 (scale, shift): y = x * scale + shift."""
    g, b = sd[prefix + ".weight"].double(), sd[prefix + ".bias"].double()
    mu, var = sd[prefix + ".running_mean"].double(), sd[prefix + ".running_var"].double()
    s = g / torch.sqrt(var + BN_EPS)
    return s, b - mu * s


def _slabs(n: int, cout: int, cin: int, k: int, device):
    return tuple(torch.empty(((cin + 15) // 16, k * k, 2, cout, 8), dtype=torch.int16, device=device) for _ in range(n))


def fold_conv_bn(sd, conv, norm):
    """Float64 (scale, shift) of ``norm(conv(x) + bias)``: the convolution's own bias goes through the eval-mode BatchNorm behind it."""
    scale, shift = bn_fold(sd, norm)
    return scale, shift + sd[conv + ".bias"].double() * scale


def prep_fwd(w, scale=None, shift=None, terms=3):
    """(split-bf16 slabs of ``w * scale[co]``: three-way, or two-way with ``terms=2``; the shift as fp32 bias or None) for ``conv_sb``."""
    cout, cin, k, _ = w.shape
    if scale is not None:
        w = (w.double() * scale[:, None, None, None]).float()
    w = w.contiguous()
    slabs = _slabs(terms, cout, cin, k, w.device)
    lib().call("e4s_conv_prep_weights_sb3" if terms == 3 else "e4s_conv_prep_weights_sb", *[_p(s) for s in slabs], None, _p(w), None, None, None, None, 0.0, None,
               cout, cin, k, k, _stream())
    return slabs, (shift.float().contiguous() if shift is not None else None)


def prep_exact(w, scale=None, shift=None):
    """(K-major fp32 weight ``[cin][k k][cout]`` of ``w * scale[co]``, folded in float64; the shift as fp32 bias or None) for ``conv_exact``.  Plain torch."""
    cout, cin, k, _ = w.shape
    if scale is not None:
        w = (w.double() * scale[:, None, None, None]).float()
    return w.permute(1, 2, 3, 0).reshape(cin, k * k, cout).contiguous(), (shift.float().contiguous() if shift is not None else None)


def prep_dgrad(w, out_scale=None, in_scale=None):
    """Two-way split slabs of the data-gradient convolution of ``w [cout, cin, k, k]``: flipped, transposed, times ``out_scale[co]`` (a BN after
    the conv) and ``in_scale[ci]`` (a BN before it).  Without scales the trip through float64 is exact."""
    wd = w.double()
    if out_scale is not None:
        wd = wd * out_scale[:, None, None, None]
    if in_scale is not None:
        wd = wd * in_scale[None, :, None, None]
    wf = wd.flip(2, 3).transpose(0, 1).float().contiguous()            # [cin][cout][k][k]
    cin, cout, k, _ = wf.shape
    s2 = _slabs(2, cin, cout, k, w.device)
    lib().call("e4s_conv_prep_weights_sb", _p(s2[0]), _p(s2[1]), None, _p(wf), None, None, None, None, 0.0, None, cin, cout, k, k, _stream())
    return s2


# ------------------------------------------------------------------------------------------------ convolution
def conv_sb(x, slabs, bias=None, *, k: int, stride: int = 1, pad: Optional[int] = None, relu: bool = False, residual=None, x1=None, slope=None, out=None, stream=None):
    """Split-bf16 convolution of csrc/conv.hip on prepared ``slabs``: three-way (``prep_fwd``) or two-way (``prep_dgrad``); ``pad`` defaults to k // 2.
    Input channels come from ``x`` and then ``x1`` (a concatenation that is never formed); ``slope [cout]`` makes the activation a PReLU; ``residual`` is
    added before it; ``out``: the ``[bs, cout, ho, wo]`` tensor (or view of a larger buffer) to write into; ``stream``: the current stream, where the caller has looked
    it up already."""
    bs, c0, h, w = x.shape
    cin = c0 if x1 is None else c0 + x1.shape[1]
    cout = slabs[0].shape[3]
    pad = k // 2 if pad is None else pad
    if out is None:
        out = torch.empty((bs, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1), dtype=torch.float32, device=x.device)
    lib().call("e4s_conv2d_sb3" if len(slabs) == 3 else "e4s_conv2d_sb", _p(out), _p(x), _p(x1), c0, *[_p(s) for s in slabs], _p(bias), None, None, _p(slope),
               _p(residual), 2 if slope is not None else 1 if relu else 0, bs, cin, cout, h, w, k, stride, pad, _stream() if stream is None else stream)
    return out


def conv_exact(x, wt, bias=None, *, k: int, stride: int = 1, pad: Optional[int] = None, relu: bool = False, slope=None, residual=None, out=None, stream=None):
    """Exact-float32 convolution of csrc/conv.hip (``e4s_conv2d``) on a K-major weight (``prep_exact``, or ``e4s_conv_prep_weights``' copy of that layout);
    ``pad``, ``slope``, ``residual``, ``out`` and ``stream`` as ``conv_sb`` takes them."""
    bs, cin, h, w = x.shape
    cout = wt.numel() // (cin * k * k)
    pad = k // 2 if pad is None else pad
    if out is None:
        out = torch.empty((bs, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1), dtype=torch.float32, device=x.device)
    lib().call("e4s_conv2d", _p(out), _p(x), None, 0, _p(wt), _p(bias), None, None, _p(slope), _p(residual), 2 if slope is not None else 1 if relu else 0,
               bs, cin, cout, h, w, k, stride, pad, _stream() if stream is None else stream)
    return out


# ------------------------------------------------------------------------------------------------ pre-processing operator
def pool_matrix(n_in: int, n_out: int) -> np.ndarray:
    """AdaptiveAvgPool1d(n_out) on n_in samples: rows are the windows floor(i n_in / n_out) .. ceil((i + 1) n_in / n_out)."""
    A = np.zeros((n_out, n_in))
    for i in range(n_out):
        lo, hi = (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)
        A[i, lo:hi] = 1.0 / (hi - lo)
    return A


def bands(A: np.ndarray):
    """[rows][2] = [lo, hi) of each row's nonzeros and [cols][2] of each column's (empty: [0, 0)); the nonzeros of a row / column are contiguous."""
    def rng(M):
        out = np.zeros((M.shape[0], 2), dtype=np.int32)
        for r in range(M.shape[0]):
            nz = np.nonzero(M[r])[0]
            if nz.size:
                assert nz[-1] - nz[0] + 1 == nz.size, "pre-processing band is not contiguous"
                out[r] = (nz[0], nz[-1] + 1)
        return out
    return rng(A), rng(A.T)


class Resampler:
    """out = A_y X A_x^T per plane (csrc/idloss.hip) for float64 axis matrices ``ay [side, h]``, ``ax [side, w]`` with banded rows and columns, and
    its adjoint: the device copies of both matrices, their row bands (the forward's) and their column bands (the adjoint's)."""

    def __init__(self, ay: np.ndarray, ax: np.ndarray, device):
        (ry, cy), (rx, cx) = bands(ay), bands(ax)
        T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)   # noqa: E731
        self.side = ay.shape[0]
        self.ay, self.ax = T(ay, torch.float32), T(ax, torch.float32)
        self.rows = T(ry, torch.int32), T(rx, torch.int32)
        self.cols = T(cy, torch.int32), T(cx, torch.int32)

    def apply(self, x, out=None):
        bs, c, h, w = x.shape
        if out is None:
            out = torch.empty((bs, c, self.side, self.side), dtype=torch.float32, device=x.device)
        lib().call("e4s_id_resample", _p(out), _p(x), _p(self.ay), _p(self.ax), _p(self.rows[0]), _p(self.rows[1]), bs * c, h, w, self.side, _stream())
        return out

    def adjoint(self, g, shape):
        """d loss / d x ``[shape]`` from ``g`` = d loss / d ``apply(x)``."""
        bs, c, h, w = shape
        gx = torch.empty(shape, dtype=torch.float32, device=g.device)
        lib().call("e4s_id_resample_adjoint", _p(gx), _p(g), _p(self.ay), _p(self.ax), _p(self.cols[0]), _p(self.cols[1]), bs * c, h, w, self.side, 0,
                   _stream())
        return gx


_RESAMPLERS = {}


def resampler(h: int, w: int, side: int, device, axes) -> Resampler:
    """The cached ``Resampler`` of an h x w image to side x side on ``device``; ``axes()`` gives its (ay, ax) when it has to be built."""
    key = (h, w, side, str(device))
    hit = _RESAMPLERS.get(key)
    if hit is None:
        hit = _RESAMPLERS[key] = Resampler(*axes(), device)
    return hit


# ------------------------------------------------------------------------------------------------ heads and small kernels
def cos_heads(fx, fy):
    """(loss, sim_improvement, stats [ntap][bs][3]) of ``sum over taps of mean_i (1 - cos(fx_i, fy_i))``; ``fx``, ``fy``: lists of ``[bs, D]``."""
    bs = fx[0].shape[0]
    nbs = [-(-f.shape[1] // HEAD_BLOCK) for f in fx]
    part = torch.empty((3 * bs * sum(nbs),), dtype=torch.float32, device=fx[0].device)
    off = 0
    for a, b, nb in zip(fx, fy, nbs):
        lib().call("e4s_id_head_partial", _p(part[off:]), _p(a), _p(b), bs, a.shape[1], _stream())
        off += 3 * bs * nb
    loss = torch.empty((), dtype=torch.float32, device=fx[0].device)
    sim = torch.empty((), dtype=torch.float32, device=fx[0].device)
    stats = torch.empty((len(fx), bs, 3), dtype=torch.float32, device=fx[0].device)
    nb5 = nbs + [0] * (5 - len(nbs))
    lib().call("e4s_id_head_sum", _p(loss), _p(sim), _p(stats), _p(part), bs, len(fx), *nb5, _stream())
    return loss, sim, stats


def cos_heads_multi(fx, ys, tw, frame):
    """(loss, stats [ntap][bs][9]) of the multi-target heads: ``ys[j][t]`` is target j's tap t."""
    bs = fx[0].shape[0]
    nbs = [-(-f.shape[1] // HEAD_BLOCK) for f in fx]
    part = torch.empty((MULTI_STATS * bs * sum(nbs),), dtype=torch.float32, device=fx[0].device)
    off = 0
    for t, (a, nb) in enumerate(zip(fx, nbs)):
        lib().call("e4s_id_head_partial_multi", _p(part[off:]), _p(a), *call_args([y[t] for y in ys], tw, frame, bs), bs, a.shape[1], _stream())
        off += MULTI_STATS * bs * nb
    loss = torch.empty((), dtype=torch.float32, device=fx[0].device)
    stats = torch.empty((len(fx), bs, MULTI_STATS), dtype=torch.float32, device=fx[0].device)
    _, ws, k = _host_targets([0] * len(tw), tw)
    lib().call("e4s_id_head_sum_multi", _p(loss), _p(stats), _p(part), ws, k, bs, len(fx), *(nbs + [0] * (5 - len(nbs))), _stream())
    return loss, stats


def relu_mask(g, a):
    """``g`` *= (a > 0) in place, over ``g``'s elements (``a`` may be longer: its head is read)."""
    lib().call("e4s_lpips_relu_mask", _p(g), _p(a), g.numel(), _stream())


def sum_partials(partial, n: int):
    """The first ``n`` partial sums added in a fixed order into a device scalar."""
    loss = torch.empty((), dtype=torch.float32, device=partial.device)
    lib().call("e4s_lpips_sum", _p(loss), _p(partial), n, _stream())
    return loss


def check_image(x: torch.Tensor, name: str) -> torch.Tensor:
    """``x`` as a contiguous fp32 device tensor ``[bs >= 1, 3, H, W]``."""
    x = _c(x, name)
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
        raise ValueError(f"{name}: expected [bs >= 1, 3, H, W], got {tuple(x.shape)}")
    return x


# ------------------------------------------------------------------------------------------------ multi-target helpers
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
