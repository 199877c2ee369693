"""Row f16: GPEN face enhancement, stage 5 — the RealESRNet pass of ``FaceEnhancement.process`` (swap_face_fine/gpen/sr_model/real_esrnet.py:8-60 around
``RRDBNet(3, 3, scale, num_feat=32, num_block=23, num_grow_ch=32)`` of sr_model/rrdbnet_arch.py:64-116) and the ``cv2.resize`` of the frame to the
super-resolved size (face_enhancement.py:66), forward only: ``gpen_sr_forward``, ``gpen_sr_image``, ``cv_resize_linear``.

This is row f11's network (``ops.RRDBNet``: ``num_feat=64``, scale 4, another checkpoint) with the feature width and the scale read off the weights; the
network itself, its mirror module ``GpenSRNet`` and its prepared weights are ``ops_rrdb``'s, shared with row f11.  Here are the two ends of
``RealESRNet.process`` and the resize:

    e4s_gsr_input             uint8 -> v / 255, the channel flip, the bottom / right reflect pad to a multiple of r and the pixel-unshuffle by r, one pass
                              (csrc/gpen_sr.hip)
    e4s_gsr_tail              conv_last in exact float32, clamp(0, 1), * 255.0, round half to even, the crop, the flip back, uint8 (csrc/rrdb.hip)
    e4s_cv_resize_linear_u8   cv2.resize at INTER_LINEAR in OpenCV's fixed-point arithmetic (pinned by tests/gpen_sr_model.py, never run against OpenCV;
                              csrc/gpen_sr.hip)"""
from __future__ import annotations

import torch

from . import ops_rrdb
from ._lib import lib
from .netweights import _cuda_checked, _devices_checked, _tensor_checked, _validated, prepare
from .ops import _p, _stream
from .ops_rrdb import GPEN_SR_FEATS, GPEN_SR_SCALES, _GSR_NET, _UNSHUFFLE, GpenSRNet, gpen_sr_state_dict_shapes

GPEN_SR_MAX_SIDE = 16384


def gpen_sr_weight_tensors(weights, name: str = "gpen_sr_forward"):
    """The tensors of the network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _GSR_NET)[2]


class PreparedGpenSRNet(ops_rrdb._PreparedRRDB):
    """``ops_rrdb._PreparedRRDB`` for a network whose block count, width and scale are read off its weights."""

    __slots__ = ()
    _entry, _net = "gpen_sr_forward", _GSR_NET


def _gsr_run(x, P, want_float, crop, bgr=False):
    """``ops_rrdb._run`` with ``e4s_gsr_tail`` at its end: ``C`` in front of (H, W), the crop (Ho, Wo) of the uint8 image and the flip behind them.  ``crop`` None:
    the float output alone."""
    Ho, Wo = crop or (4 * x.shape[2], 4 * x.shape[3])
    return ops_rrdb._run(x, P, want_float, crop, ("e4s_gsr_tail", (P["num_feat"],), (Ho, Wo, int(bgr))))


def gpen_sr_forward(x: torch.Tensor, weights) -> torch.Tensor:
    """``RRDBNet.forward`` (sr_model/rrdbnet_arch.py:102-116) in eval mode on the device: float32 ``[bs, 3, 4h / r, 4w / r]`` from a float32 ``[bs, 3, h, w]``
    image, ``r`` = 1, 2, 4 at scale 4, 2, 1 — the input scaled by ``scale``.  ``weights``: a module with the network's keys (``GpenSRNet``, the drop-in
    ``RRDBNet``) or a mapping, bare or the checkpoint with ``params_ema`` / ``params``; the block count, ``num_feat`` (32 or 64) and the scale (conv_first's
    3, 12 or 48 input channels) are read off the keys and shapes.  Refused: ``h`` or ``w`` not divisible by ``r`` (the reference's pixel_unshuffle asserts the
    same), an output side over 16384.  The pixel-unshuffle of a float input is a strided copy by PyTorch (``gpen_sr_image`` has it fused into its input
    kernel).  A module's prepared weights are cached per parameter version; a mapping is prepared on every call.  Every convolution runs on the three-way
    split-bf16 kernel except conv_last, which is exact float32 (``e4s_gsr_tail``).  The samples of a batch run one after another on scratch that does not grow
    with ``bs``.  Forward only, no gradient.  Every argument is checked before any launch."""
    name = "gpen_sr_forward"
    checked = _validated(name, weights, _GSR_NET)
    scale = checked[1][2]
    r = _UNSHUFFLE[scale]
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, 3, h, w] image")
    bs, c3, h, w = x.shape
    if c3 != 3 or h < 1 or w < 1:
        raise ValueError(f"{name}: x: expected a float32 [bs, 3, h, w] image with h, w >= 1, got {tuple(x.shape)}")
    if h % r or w % r:
        raise ValueError(f"{name}: x is {h} x {w}: at scale {scale} the network unshuffles by {r}, which both sides must be divisible by")
    if scale * h > GPEN_SR_MAX_SIDE or scale * w > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: x is {h} x {w}: the x{scale} output may be {GPEN_SR_MAX_SIDE} x {GPEN_SR_MAX_SIDE} at the most")
    _devices_checked(name, "x", x, checked[2])
    _cuda_checked(name, x=x)
    if bs == 0:
        return torch.empty((0, 3, scale * h, scale * w), dtype=torch.float32, device=x.device)
    with torch.no_grad():
        x = x.detach()
        if r > 1:
            x = x.reshape(bs, 3, h // r, r, w // r, r).permute(0, 1, 3, 5, 2, 4).reshape(bs, 3 * r * r, h // r, w // r)
        return _gsr_run(x.contiguous(), prepare(PreparedGpenSRNet, weights, checked), True, None)[0]


def gpen_sr_output_size(H: int, W: int, scale: int):
    """((Ho, Wo), (ph, pw)) of ``RealESRNet.process`` on an ``H x W`` image: the pad to a multiple of mod_scale, and ``Ho = scale (H + ph) - ph`` — the
    reference crops ``ph`` pixels of the OUTPUT, not ``scale * ph`` (real_esrnet.py:50-52), so an odd ``H`` at scale 2 gives ``2 H + 1``."""
    r = _UNSHUFFLE[scale]
    ph, pw = -H % r, -W % r
    return (scale * (H + ph) - ph, scale * (W + pw) - pw), (ph, pw)


def _image_checked(name, nm, img_u8):
    _tensor_checked(name, nm, img_u8, torch.uint8, 4, "a uint8 [bs, H, W, 3] image")
    bs, H, W, c3 = img_u8.shape
    if c3 != 3 or H < 1 or W < 1 or H > GPEN_SR_MAX_SIDE or W > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: {nm}: expected a uint8 [bs, H, W, 3] image with 1 <= H, W <= {GPEN_SR_MAX_SIDE}, got {tuple(img_u8.shape)}")
    return bs, H, W


def gpen_sr_image(img_u8: torch.Tensor, weights, bgr: bool = True) -> torch.Tensor:
    """``RealESRNet.process`` (sr_model/real_esrnet.py:26-60) for a batch on the device, as three steps: ``e4s_gsr_input`` (``/ 255``, the channel flip, the
    reflect pad to a multiple of mod_scale, the pixel-unshuffle), the network, ``e4s_gsr_tail`` (conv_last, the crop, ``clamp(0, 1)``, the flip back,
    ``(x * 255).round()``).  uint8 ``[bs, H, W, 3]`` (BGR as the reference takes it; ``bgr=False``: RGB in and out) to uint8 ``[bs, Ho, Wo, 3]`` with
    ``(Ho, Wo) = gpen_sr_output_size(H, W, scale)[0]``.  Refused with ``ValueError``: ``H <= ph`` or ``W <= pw`` (PyTorch's reflect pad raises there, in front of the
    reference's ``try``), an output side over 16384.  ``weights`` as ``gpen_sr_forward`` takes them."""
    name = "gpen_sr_image"
    checked = _validated(name, weights, _GSR_NET)
    scale = checked[1][2]
    bs, H, W = _image_checked(name, "img_u8", img_u8)
    (Ho, Wo), (ph, pw) = gpen_sr_output_size(H, W, scale)
    if H <= ph or W <= pw:
        raise ValueError(f"{name}: img_u8 is {H} x {W}: the reflect pad of {ph} x {pw} to a multiple of {_UNSHUFFLE[scale]} needs more rows / columns than that")
    if scale * (H + ph) > GPEN_SR_MAX_SIDE or scale * (W + pw) > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: img_u8 is {H} x {W}: the x{scale} output may be {GPEN_SR_MAX_SIDE} x {GPEN_SR_MAX_SIDE} at the most")
    _devices_checked(name, "img_u8", img_u8, checked[2])
    _cuda_checked(name, img_u8=img_u8)
    if bs == 0:
        return torch.empty((0, Ho, Wo, 3), dtype=torch.uint8, device=img_u8.device)
    r = _UNSHUFFLE[scale]
    with torch.no_grad():
        x = torch.empty((bs, 3 * r * r, (H + ph) // r, (W + pw) // r), dtype=torch.float32, device=img_u8.device)
        lib().call("e4s_gsr_input", _p(x), _p(img_u8.contiguous()), bs, H, W, r, int(bool(bgr)), _stream())
        return _gsr_run(x, prepare(PreparedGpenSRNet, weights, checked), False, (Ho, Wo), bool(bgr))[1]


def cv_resize_linear(img_u8: torch.Tensor, dsize) -> torch.Tensor:
    """``cv2.resize(img, (Wo, Ho))`` at its default ``INTER_LINEAR`` for a batch on the device (``e4s_cv_resize_linear_u8``): uint8 ``[bs, H, W, 3]`` to uint8
    ``[bs, Ho, Wo, 3]``, ``dsize = (Wo, Ho)`` in cv2's order.  OpenCV's portable fixed-point arithmetic as tests/gpen_sr_model.py restates it; cv2 itself has
    never been run against it.  Refused: the exact 2 : 1 downscale of both sides, which OpenCV routes to ``INTER_AREA``."""
    name = "cv_resize_linear"
    bs, H, W = _image_checked(name, "img_u8", img_u8)
    try:
        Wo, Ho = dsize
    except (TypeError, ValueError):
        raise ValueError(f"{name}: dsize is a pair (Wo, Ho) of ints in 1..{GPEN_SR_MAX_SIDE}, got {dsize!r}") from None
    for v in (Wo, Ho):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= GPEN_SR_MAX_SIDE:
            raise ValueError(f"{name}: dsize is a pair (Wo, Ho) of ints in 1..{GPEN_SR_MAX_SIDE}, got {dsize!r}")
    if H == 2 * Ho and W == 2 * Wo:
        raise ValueError(f"{name}: {H} x {W} to {Ho} x {Wo} is the exact 2 : 1 downscale, which cv2 routes to INTER_AREA: not offered")
    _cuda_checked(name, img_u8=img_u8)
    out = torch.empty((bs, Ho, Wo, 3), dtype=torch.uint8, device=img_u8.device)
    lib().call("e4s_cv_resize_linear_u8", _p(out), _p(img_u8.contiguous()), bs, H, W, Ho, Wo, _stream())
    return out


__all__ = ["GPEN_SR_FEATS", "GPEN_SR_SCALES", "GpenSRNet", "PreparedGpenSRNet", "gpen_sr_state_dict_shapes", "gpen_sr_weight_tensors", "gpen_sr_output_size",
           "gpen_sr_forward", "gpen_sr_image", "cv_resize_linear"]
