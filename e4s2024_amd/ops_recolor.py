"""Rows f8 and f9: Blender recolouring.  Stage 1 — the semantic colour reference on the device (``csrc/colorref.hip``).

``color_reference`` is ``get_color_refer`` (swap_face_fine/Blender/model_center/semantic_tools.py:50-167): per facial part a masked cross-attention from the
animated image's pixels A to the target's pixels T, ``ref_p[:, a] = sum_t softmax_t(tau cos(x_a, y_t)) rgb_T[:, t]``, and its inverse.  ``blender_part_masks`` and
``blender_packages`` are the mask and package glue of ``Referencer.forward`` (referencer.py:38-86) around it: everything of that forward after its FPN calls.

Two departures from the reference, both where its result is not a function of its inputs:

* batches are processed PER SAMPLE, each sample exactly as a batch-of-one call.  The reference pads every sample to the batch's largest part through ``topk``
  ties, so at batch > 1 its result depends on which tied pixels ``topk`` happens to return; it only ever runs batch 1.
* with two or more parts present but no ``inpainting`` pixels on one side the reference raises ``KeyError``; here ``inpaint_ref`` is zero.

``light=True`` (the top-1000 subsampling) is the same tie problem at batch 1 and is not offered.  Supported: 256 feature channels, ``h * w <= 4096``.

Row f9, stage 2 — the network that consumes the packages, ``ResUNet`` (swap_face_fine/Blender/model_center/res_u_net.py), eval mode, forward only
(``blender_unet``, ``blender_recolor``).  Seven residual blocks and a 1x1 sigmoid head; every convolution on csrc/conv.hip's three-way split-bf16 kernel
(fp32-class, no range guard, so nothing is read back), the glue on csrc/resunet.hip:

    input block        c1 = relu(bn1(conv1(x)))                   bn1 and conv1.bias folded into conv1's weights, ReLU in the epilogue
                       out = conv2(c1) + b2 + sqz(x)              sqz: the 1x1 shortcut on the raw input, added in conv2's epilogue
    residual block     a = relu(bn1(x))                           e4s_resunet_preact: a pass of its own, x itself still feeds the shortcut
                       c1 = relu(bn2(conv1(a)))                   bn2 and conv1.bias folded, the block's stride
                       out = conv2(c1) + b2 + sqz(x)              sqz at the block's stride
    decoder block      x = cat(up2(low), skip) is never formed: e4s_resunet_up_cat_preact writes a = relu(bn1(x)) and up2(low) in one pass, and sqz reads
                       (up2(low), skip) through the convolution's two input pointers.  The shortcut is taken in this direct form; the commuted one,
                       up2(W0 low) + W1 skip, was not measured and is not used.
    head               sigmoid(W x + b)                           e4s_resunet_head (full-precision exponential)

BatchNorm runs on its running statistics; a module in training mode is refused.  Prepared weights are cached per module and parameter version
(``lossnet.prepare`` / ``weights_key``); the width (64, or 16 for the reference's ``small_FPN``) is read off the weights.
"""
from __future__ import annotations

import ctypes
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lossnet
from ._lib import lib
from .lossnet import bn_fold, prep_fwd, weights_key
from .ops import _Prepared, _c, _p, _stream
from .ops_post import GREY_MORPH_MAX_RADIUS, grey_dilate

BLENDER_PARTS = ("skin", "hair", "eye", "nose", "lip", "tooth", "ear", "brow", "inpainting")
# the 19-class parser ids of the eight head parts (semantic_tools.py:170-179)
BLENDER_PART_IDS = {"skin": (1,), "hair": (17,), "eye": (4, 5), "nose": (10,), "lip": (12, 13), "tooth": (11,), "ear": (7, 8), "brow": (2, 3)}
COLORREF_CHANNELS = 256
COLORREF_MAX_PIXELS = 4096
_NPARTS = len(BLENDER_PARTS)
_IMAGENET_MEAN = (0.485, 0.456, 0.406)
_IMAGENET_STD = (0.229, 0.224, 0.225)
_CONSTS = {}


def _consts(device):
    """(label -> part index table, part indices, ImageNet mean, std) on ``device``, made once: their host-to-device copies cannot be captured in a graph, so
    the first call on a device runs eagerly (the warm-up every capture has anyway)."""
    c = _CONSTS.get(device)
    if c is None:
        lut = torch.full((256,), _NPARTS, dtype=torch.int64)
        for p, part in enumerate(BLENDER_PARTS[:-1]):
            for i in BLENDER_PART_IDS[part]:
                lut[i] = p
        c = _CONSTS[device] = (lut.to(device), torch.arange(_NPARTS - 1, device=device).view(1, -1, 1, 1),
                               torch.tensor(_IMAGENET_MEAN, device=device).view(1, 3, 1, 1), torch.tensor(_IMAGENET_STD, device=device).view(1, 3, 1, 1))
    return c


def _tensor_checked(name, nm, t, dtype, ndim, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a torch.Tensor")
    if t.dtype != dtype or t.dim() != ndim:
        raise ValueError(f"{name}: {nm}: expected {what}, got {t.dtype} {tuple(t.shape)}")


def _cuda_checked(name, **tensors):
    for nm, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {nm} must be a CUDA tensor")


def _labels_checked(name, labels_a, labels_t):
    for nm, t in (("labels_a", labels_a), ("labels_t", labels_t)):
        _tensor_checked(name, nm, t, torch.uint8, 3, "a uint8 [bs, H, W] label map")
    if labels_a.shape != labels_t.shape:
        raise ValueError(f"{name}: labels_a {tuple(labels_a.shape)} and labels_t {tuple(labels_t.shape)} differ in shape")
    radius = int(labels_a.shape[-1] * 0.1 / 2)                          # k = int(W * 0.1 / 2) * 2 + 1 = 2 radius + 1   (semantic_tools.py:197-200)
    if radius > GREY_MORPH_MAX_RADIUS:
        raise ValueError(f"{name}: a {labels_a.shape[-1]} wide map asks for a dilation radius of {radius}, grey_dilate goes up to {GREY_MORPH_MAX_RADIUS}")
    return radius


def _tau_checked(name, tau):
    """(host float, device tensor or None): a tensor is read by the kernel, never here."""
    if isinstance(tau, torch.Tensor):
        if tau.numel() != 1 or tau.dtype != torch.float32:
            raise ValueError(f"{name}: tau as a tensor has one float32 element, got {tau.dtype} {tuple(tau.shape)}")
        if not tau.is_cuda:
            raise RuntimeError(f"{name}: tau must be a CUDA tensor (or a Python float)")
        return 0.0, tau.detach()
    if isinstance(tau, bool) or not isinstance(tau, (int, float)):
        raise TypeError(f"{name}: tau is a float or a one-element float32 CUDA tensor, got {type(tau).__name__}")
    return float(tau), None


def _feats_checked(name, feats_a, feats_t, bs):
    for nm, t in (("feats_a", feats_a), ("feats_t", feats_t)):
        _tensor_checked(name, nm, t, torch.float32, 4, "float32 [bs, 256, h, w] features")
    if feats_a.shape != feats_t.shape or feats_a.shape[0] != bs:
        raise ValueError(f"{name}: feats_a {tuple(feats_a.shape)} and feats_t {tuple(feats_t.shape)} must agree, for {bs} images")
    _, d, h, w = feats_a.shape
    if d != COLORREF_CHANNELS:
        raise ValueError(f"{name}: {d} feature channels, the kernel is built for {COLORREF_CHANNELS}")
    if not 1 <= h * w <= COLORREF_MAX_PIXELS:
        raise ValueError(f"{name}: {h} x {w} features: h * w must be in 1..{COLORREF_MAX_PIXELS}")


def _reference_inputs(name, img_t, feats_a, feats_t, parts_a, parts_t):
    _tensor_checked(name, "img_t", img_t, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    for nm, t in (("parts_a", parts_a), ("parts_t", parts_t)):
        _tensor_checked(name, nm, t, torch.uint8, 4, f"uint8 [bs, {_NPARTS}, H, W] part masks")
    bs, c3, H, W = img_t.shape
    if c3 != 3:
        raise ValueError(f"{name}: img_t: expected a float32 [bs, 3, H, W] image, got {tuple(img_t.shape)}")
    _feats_checked(name, feats_a, feats_t, bs)
    for nm, t in (("parts_a", parts_a), ("parts_t", parts_t)):
        if tuple(t.shape) != (bs, _NPARTS, H, W):
            raise ValueError(f"{name}: {nm}: expected uint8 [{bs}, {_NPARTS}, {H}, {W}] part masks, got {tuple(t.shape)}")
    _cuda_checked(name, img_t=img_t, feats_a=feats_a, feats_t=feats_t, parts_a=parts_a, parts_t=parts_t)
    return img_t.contiguous(), feats_a.contiguous(), feats_t.contiguous(), parts_a.contiguous(), parts_t.contiguous()


def blender_part_masks(labels_a: torch.Tensor, labels_t: torch.Tensor):
    """The part masks of ``Referencer.forward`` (referencer.py:38-49) from two uint8 ``[bs, H, W]`` 19-class maps.

    Returns ``(parts_a, parts_t, head_a, head_t, e_at)``: uint8 ``[bs, 9, H, W]`` masks in the order of ``BLENDER_PARTS`` (``inpainting`` last) and float32
    ``[bs, 1, H, W]`` planes.  ``head`` is the sum of the eight part masks, ``dil`` the flat ``k x k`` maximum with ``k = int(W * 0.1 / 2) * 2 + 1``
    (``grey_dilate``), ``inpainting_T = clamp(dil(head_T) - head_T, 0, 1)``, ``e_AT = dil(clamp(head_A + head_T, 0, 1))`` and
    ``inpainting_A = clamp(e_AT - head_A, 0, 1)``.  ``ValueError`` when the radius exceeds ``GREY_MORPH_MAX_RADIUS``."""
    name = "blender_part_masks"
    radius = _labels_checked(name, labels_a, labels_t)
    _cuda_checked(name, labels_a=labels_a, labels_t=labels_t)
    lut, ids, _, _ = _consts(labels_a.device)

    def head_parts(labels):
        part = lut[labels.long()][:, None]                              # [bs, 1, H, W]: the part index of every pixel, 9 = none
        return (part == ids).to(torch.uint8), (part < _NPARTS - 1).float()

    pa, head_a = head_parts(labels_a)
    pt, head_t = head_parts(labels_t)
    dil = grey_dilate(torch.cat([head_t, (head_a + head_t).clamp_(0, 1)], dim=1), radius)
    e_at = dil[:, 1:2].contiguous()
    inp_t = (dil[:, 0:1] - head_t).clamp_(0, 1)
    inp_a = (e_at - head_a).clamp_(0, 1)
    return torch.cat([pa, inp_a.to(torch.uint8)], dim=1), torch.cat([pt, inp_t.to(torch.uint8)], dim=1), head_a, head_t, e_at


def _color_reference(name, img_t, feats_a, feats_t, parts_a, parts_t, tau, compute_inv):
    tau_f, tau_d = _tau_checked(name, tau)
    img_t, feats_a, feats_t, parts_a, parts_t = _reference_inputs(name, img_t, feats_a, feats_t, parts_a, parts_t)
    if tau_d is not None and tau_d.device != img_t.device:
        raise RuntimeError(f"{name}: tau is on {tau_d.device}, the images on {img_t.device}")
    bs, _, H, W = img_t.shape
    _, d, h, w = feats_a.shape
    dev = img_t.device
    refs = torch.zeros((bs, _NPARTS, 3, h, w), dtype=torch.float32, device=dev)
    present = torch.empty((bs, _NPARTS), dtype=torch.uint8, device=dev)
    inv = torch.empty((bs, 3, h, w), dtype=torch.float32, device=dev) if compute_inv else None
    inv_target = torch.empty_like(inv) if compute_inv else None
    if bs == 0:
        return refs, present, inv, inv_target
    nbytes = ctypes.c_int64(0)
    lib().call("e4s_colorref_scratch_bytes", bs, h, w, ctypes.byref(nbytes))
    scratch = torch.empty(((nbytes.value + 15) // 16, 4), dtype=torch.int32, device=dev)
    inv_parts = torch.zeros_like(refs) if compute_inv else None
    st = _stream()
    lib().call("e4s_colorref_lists", _p(scratch), _p(present), _p(parts_a), _p(parts_t), bs, H, W, h, w, st)
    lib().call("e4s_colorref_rows", _p(scratch), _p(inv_target), _p(feats_a), _p(feats_t), _p(img_t), _p(parts_t), bs, d, H, W, h, w, st)
    lib().call("e4s_colorref_attend", _p(refs), _p(inv_parts), _p(scratch), tau_f, _p(tau_d), bs, h, w, st)
    if compute_inv:
        lib().call("e4s_colorref_sum_parts", _p(inv), _p(inv_parts), bs, h, w, st)
    return refs, present, inv, inv_target


def color_reference(img_t: torch.Tensor, feats_a: torch.Tensor, feats_t: torch.Tensor, parts_a: torch.Tensor, parts_t: torch.Tensor, tau,
                    compute_inv: bool = True):
    """``get_color_refer`` (semantic_tools.py:50-167) on the device, one fused attention per part, no host round trip.

    ``img_t`` float32 ``[bs, 3, H, W]`` (ImageNet-normalised), ``feats_a`` / ``feats_t`` float32 ``[bs, 256, h, w]`` with ``h * w <= 4096``, ``parts_a`` /
    ``parts_t`` uint8 ``[bs, 9, H, W]`` 0/1 masks (``blender_part_masks``).  ``tau`` is a float or a one-element float32 CUDA tensor; a tensor is read by the
    kernel (a captured graph honours a value changed between replays).

    Masks and ``img_t`` are brought to ``h x w`` by the legacy nearest pick ``floor(i * (H / h))``; ``rgb_T = clamp(img_t * std + mean, 0, 1)``.  For a part
    with pixels ``A_p`` and ``T_p`` (absent when either is empty): ``x_a = feats_a[:, a]``, ``y_t = feats_t[:, t]`` where A's mask of the part is 1 at ``t`` and
    0 elsewhere (the reference masks T's features with A's mask, :102), both minus their channel mean; ``c[a, t] = x_a . y_t / (max(|x_a|, 1e-8) max(|y_t|, 1e-8))``;
    ``ref_p[:, a] = sum_t softmax_t(tau c[a, t]) rgb_T[:, t]`` and ``inv_p[:, t] = sum_a softmax_a(tau c[a, t]) ref_p[:, a]``.

    Returns ``(refs, present)`` or, with ``compute_inv``, ``(refs, present, inv, inv_target)``: ``refs`` float32 ``[bs, 9, 3, h, w]`` (zero outside a part's A
    pixels and for absent parts), ``present`` uint8 ``[bs, 9]`` on the device, ``inv = sum_p inv_p`` and ``inv_target = rgb_T * nearest(head_T + inpainting_T)``,
    float32 ``[bs, 3, h, w]``.  Every sample is computed as a batch of one (see the module text); the same inputs give the same bits."""
    refs, present, inv, inv_target = _color_reference("color_reference", img_t, feats_a, feats_t, parts_a, parts_t, tau, bool(compute_inv))
    return (refs, present, inv, inv_target) if compute_inv else (refs, present)


def blender_packages(img_a: torch.Tensor, img_t: torch.Tensor, labels_a: torch.Tensor, labels_t: torch.Tensor, feats_a: torch.Tensor,
                     feats_t: torch.Tensor, tau):
    """Everything of ``Referencer.forward`` (referencer.py:38-86) after its FPN calls: ``(packages, (inv, inv_target))``.

    ``packages`` float32 ``[bs, 12, H, W]`` = ``head_ref`` and ``inpaint_ref`` (3 channels each: the sum of the eight head parts' references and the
    ``inpainting`` reference, both zero where fewer than two of the nine parts are present, resized bilinearly with ``align_corners=True``), ``head_A``,
    ``inpainting_A``, ``grey_A = clamp(0.299 R + 0.587 G + 0.114 B, 0, 1) * head_A`` of the de-normalised ``img_a``, and ``img_bg = img_t * (1 - e_AT)``.
    The pair is ``color_reference``'s inverse.  Inputs as ``blender_part_masks`` and ``color_reference``; ``img_a`` like ``img_t``."""
    name = "blender_packages"
    tau_f, tau_d = _tau_checked(name, tau)
    _labels_checked(name, labels_a, labels_t)
    for nm, t in (("img_a", img_a), ("img_t", img_t)):
        _tensor_checked(name, nm, t, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    bs, _, H, W = img_t.shape
    if img_a.shape != img_t.shape or img_t.shape[1] != 3 or tuple(labels_a.shape) != (bs, H, W):
        raise ValueError(f"{name}: img_a {tuple(img_a.shape)}, img_t {tuple(img_t.shape)} and the {tuple(labels_a.shape)} label maps must be "
                         f"[bs, 3, H, W] and [bs, H, W]")
    _feats_checked(name, feats_a, feats_t, bs)
    _cuda_checked(name, img_a=img_a, img_t=img_t, labels_a=labels_a, labels_t=labels_t, feats_a=feats_a, feats_t=feats_t)
    parts_a, parts_t, head_a, _, e_at = blender_part_masks(labels_a, labels_t)
    refs, present, inv, inv_target = _color_reference(name, img_t, feats_a, feats_t, parts_a, parts_t, tau if tau_d is None else tau_d, True)
    h, w = refs.shape[-2:]
    packages = torch.empty((bs, 12, H, W), dtype=torch.float32, device=img_t.device)
    if bs == 0:
        return packages, (inv, inv_target)
    ref6 = torch.empty((bs, 6, H, W), dtype=torch.float32, device=img_t.device)
    lib().call("e4s_colorref_package", _p(ref6), _p(refs), _p(present), bs, H, W, h, w, _stream())
    # the mask, grey and background channels: the reference's own float32 expressions, operation by operation (they are compared with ==)
    _, _, mean, std = _consts(img_a.device)
    a01 = (img_a * std + mean).clamp(0, 1)
    grey = (a01[:, 0] * 0.299 + a01[:, 1] * 0.587 + a01[:, 2] * 0.114).clamp(0, 1)[:, None] * head_a
    packages[:, 0:6] = ref6
    packages[:, 6:7] = head_a
    packages[:, 7:8] = parts_a[:, _NPARTS - 1:_NPARTS].float()
    packages[:, 8:9] = grey
    packages[:, 9:12] = img_t * (1 - e_at)
    return packages, (inv, inv_target)


# ------------------------------------------------------------------------------------------------ row f9: the Res-U-Net
RESUNET_WIDTHS = (64, 16)                    # ResUNet(args): 64, or 16 with args.small_FPN
RESUNET_IN_CHANNELS = 12
_ENCODER = ("res_en_layer2", "res_en_layer3", "res_bridge_layer")
_DECODER = ("res_de_layer3", "res_de_layer2", "res_de_layer1")


class _Block(nn.Module):
    """The parameters of one residual block under the reference's names.  ``first``: the input block (conv1 -> bn1 -> relu -> conv2, no pre-activation);
    otherwise bn1 -> relu -> conv1 (stride) -> bn2 -> relu -> conv2.  Both add ``sqz_layer``, a 1x1 convolution of the block's raw input at its stride."""

    def __init__(self, cin: int, cout: int, stride: int = 1, first: bool = False):
        super().__init__()
        self.first, self.stride = first, stride
        if first:
            self.conv1 = nn.Conv2d(cin, cout, 3, 1, 1)
            self.bn1 = nn.BatchNorm2d(cout)
        else:
            self.bn1 = nn.BatchNorm2d(cin)
            self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1)
            self.bn2 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1)
        self.sqz_layer = nn.Conv2d(cin, cout, 1, stride, 0) if cin != cout else nn.Sequential()       # the network's blocks all change the width

    def forward(self, x):
        if self.first:
            y = F.relu(self.bn1(self.conv1(x)))
        else:
            y = F.relu(self.bn2(self.conv1(F.relu(self.bn1(x)))))
        return self.conv2(y) + self.sqz_layer(x)


class ResUNet(nn.Module):
    """The recolouring network's Res-U-Net with the reference's ``state_dict`` keys and shapes (``latest_netG.pth``'s ``unet.*`` entries, the prefix taken
    off, load with ``strict=True``).  ``width`` 64, or 16 for ``small_FPN``.  ``forward`` is the plain PyTorch composition — what the tests and the timing
    compare ``blender_unet`` with; ``blender_unet(packages, module)`` runs the same weights on the HIP kernels."""

    def __init__(self, width: int = 64):
        super().__init__()
        if width not in RESUNET_WIDTHS:
            raise ValueError(f"ResUNet: width {width}, expected one of {RESUNET_WIDTHS}")
        w = self.width = width
        self.input_encoder_layer = _Block(RESUNET_IN_CHANNELS, w, first=True)
        self.res_en_layer2 = _Block(w, 2 * w, 2)
        self.res_en_layer3 = _Block(2 * w, 4 * w, 2)
        self.res_bridge_layer = _Block(4 * w, 8 * w, 2)
        self.res_de_layer3 = _Block(8 * w + 4 * w, 4 * w)
        self.res_de_layer2 = _Block(4 * w + 2 * w, 2 * w)
        self.res_de_layer1 = _Block(2 * w + w, w)
        self.output_decoder_layer = nn.Sequential(nn.Conv2d(w, 3, 1), nn.Sigmoid())

    def forward(self, pkgs):
        skips = [self.input_encoder_layer(pkgs)]
        for name in _ENCODER:
            skips.append(getattr(self, name)(skips[-1]))
        x = skips.pop()
        for name in _DECODER:
            x = getattr(self, name)(torch.cat([F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True), skips.pop()], dim=1))
        return self.output_decoder_layer(x)


@functools.lru_cache(maxsize=2)
def _keys_shapes(width):
    with torch.device("meta"):
        return tuple((k, tuple(v.shape)) for k, v in ResUNet(width).state_dict().items())


def resunet_state_dict_shapes(width: int = 64):
    """``{key: shape}`` of ``ResUNet(width).state_dict()``, in its order."""
    return dict(_keys_shapes(width))


def _resunet_mapping(weights):
    if isinstance(weights, nn.Module):
        return weights.state_dict()
    if "input_encoder_layer.conv1.weight" not in weights and "unet.input_encoder_layer.conv1.weight" in weights:
        return {k[len("unet."):]: v for k, v in weights.items() if k.startswith("unet.")}
    return weights


def _resunet_checked(name, weights):
    """(mapping, width) of ``weights``: a module with the network's keys (``ResUNet``, the drop-in) in eval mode, or a mapping."""
    if isinstance(weights, nn.Module):
        if weights.training:
            raise RuntimeError(f"{name}: {type(weights).__name__} is in training mode; batch statistics are not offered: call .eval()")
    elif not hasattr(weights, "keys"):
        raise TypeError(f"{name}: weights must be a module or a mapping with the Res-U-Net's keys, got {type(weights).__name__}")
    sd = _resunet_mapping(weights)
    first = sd.get("input_encoder_layer.conv1.weight")
    if first is None:
        raise KeyError(f"{name}: the weights lack 'input_encoder_layer.conv1.weight': expected the keys of ResUNet (ops.resunet_state_dict_shapes())")
    width = int(first.shape[0])
    if width not in RESUNET_WIDTHS or tuple(first.shape[1:]) != (RESUNET_IN_CHANNELS, 3, 3):
        raise ValueError(f"{name}: the first convolution is {tuple(first.shape)}: the network's width must be one of {RESUNET_WIDTHS}")
    return sd, width


def resunet_weight_tensors(weights):
    """The float tensors of the network (``num_batches_tracked`` aside), in key order: what ``weights_key`` watches."""
    sd, width = _resunet_checked("blender_unet", weights)
    try:
        return [sd[k] for k in resunet_state_dict_shapes(width) if not k.endswith("num_batches_tracked")]
    except KeyError as e:
        raise KeyError(f"blender_unet: the weights lack {e}: expected the keys of ResUNet({width})") from None


class PreparedResUNet(_Prepared):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage.  Per block: ``pre`` the float32 (scale, shift) of
    the pre-activation BatchNorm (None for the input block), ``conv1`` with the BatchNorm after it and its own bias folded in (float64), ``conv2`` and
    ``sqz`` with their biases, all as three-way split slabs; ``head`` the output convolution's weight [3, width] and bias."""

    __slots__ = ()

    def get(self, weights):
        ts = resunet_weight_tensors(weights)
        key = weights_key(ts) + (ts[0].device,)
        hit = self._lookup(key)
        if hit is not None:
            return hit
        sd, width = _resunet_checked("blender_unet", weights)
        sd = {k: _c(sd[k].detach(), k) for k in resunet_state_dict_shapes(width) if not k.endswith("num_batches_tracked")}
        blocks = {}
        with torch.no_grad():
            for name in ("input_encoder_layer",) + _ENCODER + _DECODER:
                first = name == "input_encoder_layer"
                pre = None
                if not first:
                    s, t = bn_fold(sd, name + ".bn1")
                    pre = (s.float().contiguous(), t.float().contiguous())
                s, t = bn_fold(sd, name + (".bn1" if first else ".bn2"))
                blocks[name] = dict(pre=pre, stride=2 if name in _ENCODER else 1,
                                    conv1=prep_fwd(sd[name + ".conv1.weight"], s, t + sd[name + ".conv1.bias"].double() * s),
                                    conv2=prep_fwd(sd[name + ".conv2.weight"], None, sd[name + ".conv2.bias"]),
                                    sqz=prep_fwd(sd[name + ".sqz_layer.weight"], None, sd[name + ".sqz_layer.bias"]))
            head = (sd["output_decoder_layer.0.weight"].reshape(3, width).contiguous(), sd["output_decoder_layer.0.bias"].contiguous())
        return self._publish(key, dict(width=width, blocks=blocks, head=head))


def _conv3(x0, prepared, *, k, stride=1, relu=False, residual=None, x1=None):
    """``e4s_conv2d_sb3`` on prepared ``(slabs, bias)``; input channels from ``x0`` then ``x1`` (a concatenation that is never formed)."""
    slabs, bias = prepared
    bs, c0, h, w = x0.shape
    cin = c0 + (x1.shape[1] if x1 is not None else 0)
    cout, pad = slabs[0].shape[3], k // 2
    out = torch.empty((bs, cout, (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1), dtype=torch.float32, device=x0.device)
    lib().call("e4s_conv2d_sb3", _p(out), _p(x0), _p(x1), c0, *[_p(s) for s in slabs], _p(bias), None, None, None, _p(residual), 1 if relu else 0,
               bs, cin, cout, h, w, k, stride, pad, _stream())
    return out


def _block(B, x, act, x1=None):
    """conv1 (+ folded BatchNorm, ReLU) on ``act``, the 1x1 shortcut on the raw input (``x``, or ``x`` and ``x1``), conv2 + bias + shortcut."""
    c1 = _conv3(act, B["conv1"], k=3, stride=B["stride"], relu=True)
    shortcut = _conv3(x, B["sqz"], k=1, stride=B["stride"], x1=x1)
    return _conv3(c1, B["conv2"], k=3, residual=shortcut)


def _unet_forward(P, x):
    blocks = P["blocks"]
    skips = [_block(blocks["input_encoder_layer"], x, x)]
    for name in _ENCODER:
        B, x = blocks[name], skips[-1]
        bs, c, h, w = x.shape
        act = torch.empty_like(x)
        lib().call("e4s_resunet_preact", _p(act), _p(x), _p(B["pre"][0]), _p(B["pre"][1]), bs, c, h * w, _stream())
        skips.append(_block(B, x, act))
    x = skips.pop()
    for name in _DECODER:
        B, skip = blocks[name], skips.pop()
        bs, c_low, h, w = x.shape
        c_skip = skip.shape[1]
        up = torch.empty((bs, c_low, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
        act = torch.empty((bs, c_low + c_skip, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
        lib().call("e4s_resunet_up_cat_preact", _p(act), _p(up), _p(x), _p(skip), _p(B["pre"][0]), _p(B["pre"][1]), bs, c_low, c_skip, h, w, _stream())
        x = _block(B, up, act, x1=skip)
    bs, c, h, w = x.shape
    out = torch.empty((bs, 3, h, w), dtype=torch.float32, device=x.device)
    lib().call("e4s_resunet_head", _p(out), _p(x), _p(P["head"][0]), _p(P["head"][1]), bs, c, h * w, _stream())
    return out


def _unet_checked(name, packages, weights):
    _tensor_checked(name, "packages", packages, torch.float32, 4, f"float32 [bs, {RESUNET_IN_CHANNELS}, H, W] packages")
    bs, c, H, W = packages.shape
    if c != RESUNET_IN_CHANNELS:
        raise ValueError(f"{name}: packages: expected float32 [bs, {RESUNET_IN_CHANNELS}, H, W] packages, got {tuple(packages.shape)}")
    if H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"{name}: packages are {H} x {W}: both sizes must be multiples of 8 (three stride-2 blocks), at least 8")
    ts = resunet_weight_tensors(weights)
    if any(t.device != packages.device for t in ts):
        raise RuntimeError(f"{name}: device mismatch: packages on {packages.device}, the weights on {sorted({str(t.device) for t in ts})}")
    _cuda_checked(name, packages=packages)


def blender_unet(packages: torch.Tensor, weights) -> torch.Tensor:
    """``ResUNet.forward`` (res_u_net.py:96-108) in eval mode on the device: float32 ``[bs, 3, H, W]`` in [0, 1] from the float32 ``[bs, 12, H, W]``
    ``packages`` of ``blender_packages``; ``H`` and ``W`` multiples of 8.  ``weights``: a module with the network's keys (``ResUNet``, the drop-in
    ``res_u_net.ResUNet``) or a mapping; the width is read off them.  Forward only, no gradient.  Every argument is checked before any launch; no host
    synchronisation, the same inputs give the same bits, and after one eager call (which prepares the weights) the call captures in a graph."""
    name = "blender_unet"
    _unet_checked(name, packages, weights)
    bs, _, H, W = packages.shape
    if bs == 0:
        return torch.empty((0, 3, H, W), dtype=torch.float32, device=packages.device)
    with torch.no_grad():
        return _unet_forward(lossnet.prepare(PreparedResUNet, weights), packages.detach().contiguous())


def blender_recolor(img_a: torch.Tensor, img_t: torch.Tensor, labels_a: torch.Tensor, labels_t: torch.Tensor, feats_a: torch.Tensor, feats_t: torch.Tensor,
                    tau, weights):
    """``Blender.forward`` after its FPN calls: ``(pred, packages, (inv, inv_target))`` with ``packages`` and the pair from ``blender_packages`` and
    ``pred = blender_unet(packages, weights)``.  ``H`` and ``W`` multiples of 8."""
    name = "blender_recolor"
    _resunet_checked(name, weights)
    if isinstance(img_t, torch.Tensor) and img_t.dim() == 4 and (img_t.shape[2] % 8 or img_t.shape[3] % 8):
        raise ValueError(f"{name}: images are {img_t.shape[2]} x {img_t.shape[3]}: both sizes must be multiples of 8")
    packages, pair = blender_packages(img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau)
    return blender_unet(packages, weights), packages, pair


__all__ = ["BLENDER_PARTS", "BLENDER_PART_IDS", "COLORREF_CHANNELS", "COLORREF_MAX_PIXELS", "blender_part_masks", "color_reference", "blender_packages",
           "RESUNET_WIDTHS", "ResUNet", "PreparedResUNet", "resunet_state_dict_shapes", "resunet_weight_tensors", "blender_unet", "blender_recolor"]
