"""Row f24: the two ends of the whole-clip reenactment chain (face_swap_video_pipeline.py:248-253, Face_swap_with_two_imgs.py:723-743) on the device:
``sk_resize_tables``, ``sk_resize``, ``frames_u8`` (csrc/skresize.hip).

    sk_resize    ``resize(np.array(im) / 255.0, (Ho, Wo))``: ``skimage.transform.resize`` at skimage 0.19 / 0.20's defaults on a float64 image, to the float32
                 tensor ``make_animation`` takes (its callers convert to float32 there)
    frames_u8    ``(pred * 255).astype(np.uint8)`` on the float32 predictions

skimage's ``resize`` is two calls of ``scipy.ndimage`` and a clip: ``gaussian_filter(img, sigma, mode='mirror')`` with ``sigma = max(0, (in / out - 1) / 2)`` per
axis where any side shrinks, ``zoom(..., order=1, mode='mirror', grid_mode=True)``, and ``np.clip`` to the input image's own range.  The first two are linear and
separable, so an axis is one small matrix: ``sk_resize_tables`` makes it on the host in float64, once per (source, destination) size, and the kernel sums it in
float64 in a fixed order.  skimage and scipy are installed nowhere this project runs: tests/skresize_model.py restates the rule, and
tests/golden/g34_skresize.npz holds what ``scipy.ndimage`` itself gave for it."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._lib import lib
from .netweights import _cuda_checked, _tensor_checked
from .ops import _p, _stream

SK_MAX_SIDE = 16384
SK_MAX_TAPS = _lib._DEFINES["E4S_SK_MAX_TAPS"]                                # composite taps per destination index the kernel's table format holds
SK_TRUNCATE = 4.0                                                             # scipy.ndimage.gaussian_filter's default
_sk_tables = {}                              # (src, dst) -> host tables; (src, dst, device) -> device tables


def _mirror(i: int, n: int) -> int:
    """Index ``i`` of an axis of ``n`` samples under scipy's 'mirror' (d c b | a b c d | c b a), folded as often as it takes."""
    if n == 1:
        return 0
    p = 2 * n - 2
    i %= p
    return p - i if i >= n else i


def _side_checked(name, nm, v):
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= SK_MAX_SIDE:
        raise ValueError(f"{name}: {nm} is an int in 1..{SK_MAX_SIDE}, got {v!r}")
    return v


def sk_resize_tables(src: int, dst: int):
    """The composite table of one axis of ``skimage.transform.resize`` from ``src`` to ``dst`` samples: ``(start int32 [dst], count int32 [dst], weight float64
    [dst, T])`` with ``out[o] = sum_k weight[o, k] * in[start[o] + k]``, ``k < count[o]``; T is the widest count, rows are padded with zeros.  It is the product
    of the order-1 row of ``scipy.ndimage.zoom(mode='mirror', grid_mode=True)`` — source coordinate ``(o + 0.5) * src / dst - 0.5``, folded at the ends — and,
    where ``dst < src``, the rows of ``gaussian_filter`` at ``sigma = (src / dst - 1) / 2``: radius ``int(4 sigma + 0.5)``, normalised weights, 'mirror' indices.
    Pure host arithmetic in float64, kept per (src, dst).  1024 -> 256 holds 14 taps; an enlargement or equal sizes at most 2.  Refused: sizes that are not ints
    in 1..16384, and a table wider than ``SK_MAX_TAPS`` = 1024 taps (a shrink beyond about 255 : 1)."""
    name = "sk_resize_tables"
    _side_checked(name, "src", src)
    _side_checked(name, "dst", dst)
    hit = _sk_tables.get((src, dst))
    if hit is not None:
        return hit
    factor = np.float64(src) / np.float64(dst)
    gauss = {0: 1.0}
    radius = 0
    if dst < src:
        sigma = float(np.maximum(0, (factor - 1) / 2))
        radius = int(SK_TRUNCATE * sigma + 0.5)
        x = np.arange(-radius, radius + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        phi = phi / phi.sum()
        gauss = {int(k): float(g) for k, g in zip(x, phi)}
    rows = []
    for o in range(dst):
        cc = (o + 0.5) * factor - 0.5
        if src == 1:
            cc = 0.0
        elif cc < 0:                                                          # scipy's map_coordinate for 'mirror': -0.5 < cc here, one fold
            cc = -cc
        # (src - 1 < cc < src at the far end of an enlargement is left as it is: its second tap, index src, is folded below, as scipy folds it)
        i0 = math.floor(cc)
        frac = float(cc - i0)
        row = {}
        for i, a in ((i0, 1.0 - frac), (i0 + 1, frac)):
            if a == 0.0:
                continue
            for k, g in gauss.items():
                j = _mirror(i + k, src)
                row[j] = row.get(j, 0.0) + a * g
        rows.append(row)
    T = max(max(r) - min(r) + 1 for r in rows)
    if T > SK_MAX_TAPS:
        raise ValueError(f"{name}: {src} -> {dst} needs {T} composite taps per output sample: the kernel's tables hold {SK_MAX_TAPS} at the most (SK_MAX_TAPS; a "
                         "shrink of about 255 : 1)")
    start = np.array([min(r) for r in rows], dtype=np.int32)
    count = np.array([max(r) - min(r) + 1 for r in rows], dtype=np.int32)
    weight = np.zeros((dst, T), dtype=np.float64)
    for o, r in enumerate(rows):
        for j, w in r.items():
            weight[o, j - start[o]] = w
    for a in (start, count, weight):
        a.setflags(write=False)
    hit = _sk_tables[src, dst] = (start, count, weight)
    return hit


def _sk_device(src, dst, device):
    key = (src, dst, str(device))
    hit = _sk_tables.get(key)
    if hit is None:
        hit = _sk_tables[key] = tuple(torch.from_numpy(np.array(a)).to(device) for a in sk_resize_tables(src, dst))
    return hit


def _size_checked(name, size):
    try:
        Ho, Wo = size
    except (TypeError, ValueError):
        raise ValueError(f"{name}: size is a pair (Ho, Wo) of ints in 1..{SK_MAX_SIDE}, got {size!r}") from None
    for v in (Ho, Wo):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= SK_MAX_SIDE:
            raise ValueError(f"{name}: size is a pair (Ho, Wo) of ints in 1..{SK_MAX_SIDE}, got {size!r}")
    return Ho, Wo


def _sk_resize_checked(name, nm, img_u8, size):
    """What ``sk_resize`` refuses in front of the device check: (bs, H, W, Ho, Wo); the host tables exist afterwards."""
    _tensor_checked(name, nm, img_u8, torch.uint8, 4, "a uint8 [bs, H, W, 3] image batch")
    bs, H, W, C = img_u8.shape
    if C != 3 or H < 1 or W < 1 or H > SK_MAX_SIDE or W > SK_MAX_SIDE:
        raise ValueError(f"{name}: {nm}: expected a uint8 [bs, H, W, 3] image batch with 1 <= H, W <= {SK_MAX_SIDE}, got {tuple(img_u8.shape)}")
    Ho, Wo = _size_checked(name, size)
    for src, dst in ((H, Ho), (W, Wo)):
        try:
            sk_resize_tables(src, dst)
        except ValueError as e:
            raise ValueError(f"{name}: {str(e).partition(': ')[2]}") from None
    return bs, H, W, Ho, Wo


def _sk_resize_run(img_u8, Ho, Wo, chw):
    bs, H, W, _ = img_u8.shape
    dev = img_u8.device
    out = torch.empty((bs, 3, Ho, Wo) if chw else (bs, Ho, Wo, 3), dtype=torch.float32, device=dev)
    if bs:
        ys, yc, yw = _sk_device(H, Ho, dev)
        xs, xc, xw = _sk_device(W, Wo, dev)
        part = torch.empty((bs, 64, 2), dtype=torch.uint8, device=dev)
        lib().call("e4s_sk_resize_u8", _p(out), _p(part), _p(img_u8.contiguous()), _p(ys), _p(yc), _p(yw), yw.shape[1], _p(xs), _p(xc), _p(xw), xw.shape[1], bs, H, W,
                   Ho, Wo, int(bool(chw)), _stream())
    return out


def sk_resize(img_u8: torch.Tensor, size, chw: bool = True) -> torch.Tensor:
    """``float32(skimage.transform.resize(img / 255.0, (Ho, Wo)))`` for a batch on the device (``e4s_sk_resize_u8``): uint8 ``[bs, H, W, 3]`` to float32
    ``[bs, 3, Ho, Wo]`` (``chw``, what ``make_animation`` takes) or ``[bs, Ho, Wo, 3]``; ``size = (Ho, Wo)`` in skimage's order.  skimage 0.19 / 0.20's defaults
    on a float64 image: order 1, mode 'reflect', ``anti_aliasing`` where a side shrinks, ``clip`` to the image's own [min, max] (every sample its own, all
    channels together).  Float64 sums on the tables of ``sk_resize_tables``, one rounding to float32 at the end; a sample of a batch gets the bits it gets
    alone; no host read: after one eager call (the tables) a call captures in a graph.

    Refused before any launch: anything but a uint8 ``[bs, H, W, 3]`` tensor; a side outside 1..16384; a ``size`` that is not a pair of ints; a side whose
    composite tap count exceeds ``SK_MAX_TAPS`` = 1024; a CPU tensor."""
    name = "sk_resize"
    _, _, _, Ho, Wo = _sk_resize_checked(name, "img_u8", img_u8, size)
    _cuda_checked(name, img_u8=img_u8)
    return _sk_resize_run(img_u8, Ho, Wo, chw)


def _frames_u8_checked(name, nm, pred):
    _tensor_checked(name, nm, pred, torch.float32, 4, "float32 [n, 3, H, W] frames")
    n, C, H, W = pred.shape
    if C != 3 or H < 1 or W < 1 or H > SK_MAX_SIDE or W > SK_MAX_SIDE:
        raise ValueError(f"{name}: {nm}: expected float32 [n, 3, H, W] frames with 1 <= H, W <= {SK_MAX_SIDE}, got {tuple(pred.shape)}")
    return n, H, W


def frames_u8(pred: torch.Tensor, flip: bool = False) -> torch.Tensor:
    """``(pred * 255).astype(np.uint8)`` on the float32 frames of ``make_animation``, transposed as the reference's callers hold them (``e4s_frames_u8``): float32
    ``[n, 3, H, W]`` to uint8 ``[n, H, W, 3]``.  The float32 product is truncated toward zero and clamped to 0..255 (numpy leaves a value outside that range
    undefined; a NaN gives 0).  ``flip`` stores the channels reversed.  A non-contiguous view is accepted and copied.  Refused before any launch: anything but a
    float32 ``[n, 3, H, W]`` tensor with sides in 1..16384; a CPU tensor."""
    name = "frames_u8"
    n, H, W = _frames_u8_checked(name, "pred", pred)
    _cuda_checked(name, pred=pred)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=pred.device)
    if n:
        lib().call("e4s_frames_u8", _p(out), _p(pred.contiguous()), n, H, W, int(bool(flip)), _stream())
    return out


__all__ = ["SK_MAX_SIDE", "SK_MAX_TAPS", "sk_resize_tables", "sk_resize", "frames_u8"]
