"""Row f23: CodeFormer face restoration, stage 3 — ``RealESRGANer.enhance`` (swap_face_fine/realesrgan_utils.py:69-250) as ``CodeFormerInfer.infer_image``
calls it (inference_codeformer.py:175: ``tile=400, tile_pad=40, pre_pad=0``, ``outscale=2``) for a batch of uint8 RGB images on the device: ``esrgan_tiles``,
``esrgan_enhance``, ``cv_resize_lanczos4``.

The network is ``ops_rrdb``'s (rows f11 and f16: ``RRDBNet(3, 3, 4, num_feat, num_block, 32)``, the x4plus checkpoint at 64 / 23), run tile by tile and sample by
sample on scratch made once per distinct tile shape.  Around it (csrc/esrgan_tile.hip):

    e4s_esrt_input              one tile window of the (never formed) pre-padded image -> v / 255, float32 [bs, 3, th, tw]
    e4s_esrt_tail               conv_last in exact float32 on the kept window of the tile's x4 output alone, clamp(0, 1), * 255.0, round half to even, stored at
                                the window's place in the x4 canvas
    e4s_cv_resize_lanczos4_u8   cv2.resize at INTER_LANCZOS4 in OpenCV's fixed-point arithmetic, on offset and coefficient tables made here on the host (pinned by
                                tests/esrgan_tile_model.py, never run against OpenCV)

The reference sets ``half=True`` on every GPU whose name does not contain ``1650`` or ``1660``.  The fp16 rounding of a 350-convolution network depends on the
device and the library and is not reproduced: this is the ``half=False`` arithmetic, which the reference itself runs on the CPU, on the three-way split
convolutions of rows f11 and f16."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import ops_rrdb
from ._lib import lib
from .netweights import _cuda_checked, _devices_checked, _validated, prepare
from .ops import _p, _stream
from .ops_gpen_sr import GPEN_SR_MAX_SIDE, PreparedGpenSRNet
from .ops_rrdb import _GSR_NET, RRDB_GROW

ESRGAN_SCALE = 4                             # set_realesrgan builds RealESRGAN_x4plus alone
ESRGAN_TILE, ESRGAN_TILE_PAD, ESRGAN_PRE_PAD = 400, 40, 0                 # inference_codeformer.py's RealESRGANer


# ------------------------------------------------------------------------------------------------ tile_process, host arithmetic
def esrgan_tiles(H: int, W: int, tile: int = ESRGAN_TILE, tile_pad: int = ESRGAN_TILE_PAD):
    """The tiles of ``RealESRGANer.tile_process`` (realesrgan_utils.py:98-161) on an ``H x W`` (pre-padded) image at scale 4, rows of tiles first: per tile
    ``((y0, y1, x0, x1), (oy0, oy1, ox0, ox1), (Y0, X0))`` — the padded input window, the kept window inside the tile's x4 output, and where that goes in the
    ``4H x 4W`` image.  ``tile <= 0``: one tile, the whole image (the reference's ``process``).  Pure host arithmetic."""
    for nm, v in (("H", H), ("W", W)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"esrgan_tiles: {nm} is a positive int, got {v!r}")
    for nm, v in (("tile", tile), ("tile_pad", tile_pad)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"esrgan_tiles: {nm} is an int, got {v!r}")
    if tile_pad < 0:
        raise ValueError(f"esrgan_tiles: tile_pad is not negative, got {tile_pad!r}")
    s = ESRGAN_SCALE
    if tile <= 0:
        return [((0, H, 0, W), (0, s * H, 0, s * W), (0, 0))]
    out = []
    for ty in range(-(-H // tile)):
        for tx in range(-(-W // tile)):
            ys, xs = ty * tile, tx * tile
            ye, xe = min(ys + tile, H), min(xs + tile, W)
            y0, y1, x0, x1 = max(ys - tile_pad, 0), min(ye + tile_pad, H), max(xs - tile_pad, 0), min(xe + tile_pad, W)
            oy0, ox0 = (ys - y0) * s, (xs - x0) * s
            out.append(((y0, y1, x0, x1), (oy0, oy0 + (ye - ys) * s, ox0, ox0 + (xe - xs) * s), (ys * s, xs * s)))
    return out


# ------------------------------------------------------------------------------------------------ cv2.resize, INTER_LANCZOS4, uint8
_S45 = 0.70710678118654752440084436210485
_LANCZOS_CS = ((1, 0), (-_S45, -_S45), (0, 1), (_S45, -_S45), (-1, 0), (_S45, _S45), (0, -1), (-_S45, _S45))
_lanczos_tables = {}                         # (src, dst) -> host tables; (src, dst, device) -> device tables


def _lanczos4_coeffs(f):
    """``interpolateLanczos4`` at the float32 fraction ``f``, then ``short(rint(c * 2048))``: eight ints.  libm's double sin / cos, float32 where OpenCV has floats."""
    f = np.float32(f)
    if f < np.finfo(np.float32).eps:
        return [0, 0, 0, 2048, 0, 0, 0, 0]
    x3 = np.float32(f + np.float32(3))
    y0 = -float(x3) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c, total = [], np.float32(0)
    for i, (a, b) in enumerate(_LANCZOS_CS):
        y = -float(np.float32(x3 - np.float32(i))) * math.pi * 0.25
        c.append(np.float32((a * s0 + b * c0) / (y * y)))
        total = np.float32(total + c[-1])
    inv = np.float32(np.float32(1) / total)
    return [int(np.rint(np.float32(np.float32(v * inv) * np.float32(2048)))) for v in c]


def _lanczos4_axis(src, dst):
    """(ofs int32 [dst] = s - 3, coef int16 [dst, 8]) of one axis, on the host."""
    hit = _lanczos_tables.get((src, dst))
    if hit is None:
        scale = 1.0 / (float(dst) / float(src))
        f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
        s = np.floor(f)
        f = (f - s).astype(np.float32)
        rows = {}
        coef = np.array([rows.get(v) or rows.setdefault(v, _lanczos4_coeffs(v)) for v in f.tolist()], dtype=np.int16).reshape(dst, 8)
        hit = _lanczos_tables[src, dst] = (s.astype(np.int32) - 3, coef)
    return hit


def _lanczos4_device(src, dst, device):
    key = (src, dst, str(device))
    hit = _lanczos_tables.get(key)
    if hit is None:
        ofs, coef = _lanczos4_axis(src, dst)
        hit = _lanczos_tables[key] = (torch.from_numpy(ofs).to(device), torch.from_numpy(coef).to(device))
    return hit


def _u8_image_checked(name, nm, img_u8, chw=False):
    what = "a uint8 [bs, 3, H, W] image" if chw else "a uint8 [bs, H, W, 3] image"
    if not isinstance(img_u8, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a torch.Tensor")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[1 if chw else 3] != 3:
        raise ValueError(f"{name}: {nm}: expected {what} (16-bit, grey and RGBA images are not offered), got {img_u8.dtype} {tuple(img_u8.shape)}")
    bs, H, W = (img_u8.shape[0], img_u8.shape[2], img_u8.shape[3]) if chw else tuple(img_u8.shape[:3])
    if H < 1 or W < 1 or H > GPEN_SR_MAX_SIDE or W > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: {nm}: expected {what} with 1 <= H, W <= {GPEN_SR_MAX_SIDE}, got {tuple(img_u8.shape)}")
    return bs, H, W


def _dsize_checked(name, dsize):
    try:
        Wo, Ho = dsize
    except (TypeError, ValueError):
        raise ValueError(f"{name}: dsize is a pair (Wo, Ho) of ints in 1..{GPEN_SR_MAX_SIDE}, got {dsize!r}") from None
    for v in (Wo, Ho):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= GPEN_SR_MAX_SIDE:
            raise ValueError(f"{name}: dsize is a pair (Wo, Ho) of ints in 1..{GPEN_SR_MAX_SIDE}, got {dsize!r}")
    return Wo, Ho


def _lanczos4_run(img_u8, Wo, Ho):
    bs, H, W, _ = img_u8.shape
    out = torch.empty((bs, Ho, Wo, 3), dtype=torch.uint8, device=img_u8.device)
    if bs:
        yofs, ycoef = _lanczos4_device(H, Ho, img_u8.device)
        xofs, xcoef = _lanczos4_device(W, Wo, img_u8.device)
        lib().call("e4s_cv_resize_lanczos4_u8", _p(out), _p(img_u8.contiguous()), _p(yofs), _p(ycoef), _p(xofs), _p(xcoef), bs, H, W, Ho, Wo, _stream())
    return out


def cv_resize_lanczos4(img_u8: torch.Tensor, dsize) -> torch.Tensor:
    """``cv2.resize(img, (Wo, Ho), interpolation=cv2.INTER_LANCZOS4)`` for a batch on the device (``e4s_cv_resize_lanczos4_u8``): uint8 ``[bs, H, W, 3]`` to uint8
    ``[bs, Ho, Wo, 3]`` at any sizes, ``dsize = (Wo, Ho)`` in cv2's order as ``cv_resize_linear`` takes it.  OpenCV's portable fixed-point arithmetic as
    tests/esrgan_tile_model.py restates it — eight taps per axis with clamped indices, the fraction not reset at the borders, 11-bit coefficients without a fix-up
    of their sum — on tables made on the host per (source, destination) size and kept.  cv2 is installed nowhere this project is built or tested: it has never been
    run against OpenCV, the restatement is the pin."""
    name = "cv_resize_lanczos4"
    _u8_image_checked(name, "img_u8", img_u8)
    Wo, Ho = _dsize_checked(name, dsize)
    _cuda_checked(name, img_u8=img_u8)
    return _lanczos4_run(img_u8, Wo, Ho)


# ------------------------------------------------------------------------------------------------ RealESRGANer.enhance
def _int_checked(name, nm, v, lo=None):
    if isinstance(v, bool) or not isinstance(v, int) or (lo is not None and v < lo):
        raise ValueError(f"{name}: {nm} is an int{'' if lo is None else f' >= {lo}'}, got {v!r}")
    return v


def _enhance_checked(name, img_u8, weights, outscale, tile, tile_pad, pre_pad, chw):
    """Every refusal of ``esrgan_enhance`` in front of the device checks: (validated weights, bs, H, W, dsize or None)."""
    if isinstance(weights, nn.Module) and weights.training:
        raise RuntimeError(f"{name}: {type(weights).__name__} is in training mode; the native path is the eval-mode forward: call .eval()")
    checked = _validated(name, weights, _GSR_NET)
    if checked[1][2] != ESRGAN_SCALE:
        raise ValueError(f"{name}: the network is RRDBNet at scale {checked[1][2]}: only the x4 network (3 -> 3 channels, RealESRGAN_x4plus) is offered; the "
                         "reference's mod_scale path for scale 1 and 2 is not built")
    bs, H, W = _u8_image_checked(name, "img_u8", img_u8, chw)
    _int_checked(name, "tile", tile)
    _int_checked(name, "tile_pad", tile_pad, 0)
    _int_checked(name, "pre_pad", pre_pad, 0)
    dsize = None
    if outscale is not None:
        if isinstance(outscale, bool) or not isinstance(outscale, (int, float)) or not math.isfinite(outscale) or outscale <= 0:
            raise ValueError(f"{name}: outscale is None or a finite positive real, got {outscale!r}")
        if outscale != float(ESRGAN_SCALE):
            dsize = (int(W * outscale), int(H * outscale))
            if not all(1 <= v <= GPEN_SR_MAX_SIDE for v in dsize):
                raise ValueError(f"{name}: outscale {outscale!r} takes the {H} x {W} image to {dsize[1]} x {dsize[0]}: sides are in 1..{GPEN_SR_MAX_SIDE}")
    if pre_pad >= H or pre_pad >= W:
        raise ValueError(f"{name}: pre_pad {pre_pad} on a {H} x {W} image: the reflect pad needs more rows / columns than that")
    if ESRGAN_SCALE * (H + pre_pad) > GPEN_SR_MAX_SIDE or ESRGAN_SCALE * (W + pre_pad) > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: img_u8 is {H} x {W} with pre_pad {pre_pad}: the x4 image may be {GPEN_SR_MAX_SIDE} x {GPEN_SR_MAX_SIDE} at the most")
    return checked, bs, H, W, dsize


def _tile_scratch(P, h, w, bs, device):
    """What ``ops_rrdb._sample`` needs for tiles of ``h x w``: the tile inputs of the batch and one sample's slabs (as ``ops_rrdb._run`` lays them out)."""
    C, G = P["num_feat"], RRDB_GROW
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)               # noqa: E731
    slabs = [new(1, C + 4 * G, h, w) for _ in range(3)]
    reads = [[S[:, :C + k * G] for k in range(5)] for S in slabs]
    writes = [[S[:, C + k * G:C + (k + 1) * G] for k in range(4)] for S in slabs]
    ups = [(new(1, C, 2 * h, 2 * w), new(1, C, 2 * h, 2 * w)), (new(1, C, 4 * h, 4 * w), new(1, C, 4 * h, 4 * w))]
    return new(bs, 3, h, w), reads, writes, new(1, C, h, w), ups


@torch.no_grad()
def esrgan_enhance(img_u8: torch.Tensor, weights, outscale=None, tile: int = ESRGAN_TILE, tile_pad: int = ESRGAN_TILE_PAD, pre_pad: int = ESRGAN_PRE_PAD,
                   chw: bool = False, return_x4: bool = False):
    """``RealESRGANer.enhance(img, outscale)`` (realesrgan_utils.py:174-250) for a batch of uint8 RGB images on the device: ``[bs, H, W, 3]`` (``chw``:
    ``[bs, 3, H, W]``, the layout of ``pipeline.codeformer_restore``) to uint8 ``[bs, Ho, Wo, 3]``; with ``return_x4`` the pair (that, the x4 image
    ``[bs, 4H, 4W, 3]``).

        pre_process    / 255 and the reflect pre-pad of ``pre_pad`` rows and columns at the bottom / right (e4s_esrt_input, per tile; the padded image is not formed)
        tile_process   every tile of ``esrgan_tiles(H + pre_pad, W + pre_pad, tile, tile_pad)`` through the network; ``tile <= 0``: ``process``, the whole image
        post_process   the crop of the pre-pad; clamp(0, 1), ``(x * 255.0).round()`` (e4s_esrt_tail, on each tile's kept window alone)
        cv2.resize     ``outscale`` not None and not 4: INTER_LANCZOS4 to ``(int(W * outscale), int(H * outscale))`` (``cv_resize_lanczos4``)

    The channel order is kept: the reference's ``cvtColor(BGR2RGB)`` and ``[2, 1, 0]`` with its caller's flips cancel, the network sees RGB.  ``weights``: a module
    with the network's keys in eval mode (``ops.GpenSRNet(23, 64, 4)``, ``ops.RRDBNet(23)``, the drop-in) or a mapping, as ``ops.gpen_sr_forward`` takes them;
    prepared once per parameter version.  This is the reference's ``half=False`` arithmetic (the module docstring says why), every convolution on the three-way
    split-bf16 kernel except conv_last, which is exact float32.

    Scratch is made once per distinct tile shape and shared by the tiles and samples; a sample of a batch gets the bits it gets alone; the same inputs give the
    same bits; no host read: after one eager call (weights and resize tables) a call captures in a graph.

    Refused before any launch: a network that is not scale 4 / 3 -> 3 channels; an image that is not uint8 with three channels; ``tile`` / ``tile_pad`` /
    ``pre_pad`` that are not ints (the pads not negative); an ``outscale`` that is not None or a finite positive real; ``pre_pad >= H`` or ``>= W`` (reflect is
    undefined there); a x4 side over 16384; a module in training mode; tensors on mismatched devices; a CPU tensor."""
    name = "esrgan_enhance"
    checked, bs, H, W, dsize = _enhance_checked(name, img_u8, weights, outscale, tile, tile_pad, pre_pad, chw)
    _devices_checked(name, "img_u8", img_u8, checked[2])
    _cuda_checked(name, img_u8=img_u8)
    dev, s = img_u8.device, ESRGAN_SCALE
    if bs == 0:
        x4 = torch.empty((0, s * H, s * W, 3), dtype=torch.uint8, device=dev)
        out = x4 if dsize is None else torch.empty((0, dsize[1], dsize[0], 3), dtype=torch.uint8, device=dev)
        return (out, x4) if return_x4 else out
    P = prepare(PreparedGpenSRNet, weights, checked)
    img = img_u8.contiguous()
    Hp, Wp = H + pre_pad, W + pre_pad
    canvas = torch.empty((bs, s * Hp, s * Wp, 3), dtype=torch.uint8, device=dev)
    pitch = s * Wp * 3
    scratch = {}
    for (y0, y1, x0, x1), (oy0, oy1, ox0, ox1), (Y0, X0) in esrgan_tiles(Hp, Wp, tile, tile_pad):
        th, tw = y1 - y0, x1 - x0
        if (th, tw) not in scratch:
            scratch[th, tw] = _tile_scratch(P, th, tw, bs, dev)
        x, reads, writes, feat0, ups = scratch[th, tw]
        lib().call("e4s_esrt_input", _p(x), _p(img), bs, H, W, Hp, Wp, int(bool(chw)), y0, x0, th, tw, _stream())
        tail = ("e4s_esrt_tail", (P["num_feat"],), (oy0, oy1, ox0, ox1, Y0, X0, s * Hp, s * Wp, pitch))
        for b in range(bs):
            ops_rrdb._sample(P, x[b:b + 1], None, canvas[b], tail, reads, writes, feat0, ups)
    x4 = canvas if pre_pad == 0 else canvas[:, :s * H, :s * W].contiguous()
    out = x4 if dsize is None else _lanczos4_run(x4, *dsize)
    return (out, x4) if return_x4 else out


__all__ = ["ESRGAN_SCALE", "ESRGAN_TILE", "ESRGAN_TILE_PAD", "ESRGAN_PRE_PAD", "esrgan_tiles", "esrgan_enhance", "cv_resize_lanczos4"]
