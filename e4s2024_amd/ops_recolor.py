"""Rows f8 to f11: Blender recolouring (``ct_mode='blender'``), four stages: f8 the semantic colour reference, f9 the Res-U-Net that consumes its packages,
f10 the SPADE feature network that feeds it, f11 the Real-ESRGAN step behind them.  The three networks share one weights path (``netweights._validated``:
keys, shapes and dtypes checked once per public call and handed on to ``netweights.prepare``) and one convolution call (``lossnet.conv_sb``).

Row f8, stage 1 — the semantic colour reference on the device (``csrc/colorref.hip``).

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
(``netweights.prepare`` / ``weights_key``); the width (64, or 16 for the reference's ``small_FPN``) is read off the weights.

Row f10, stage 3 — the feature network that produces ``feats_a`` / ``feats_t``, ``AdaptiveFeatureGenerator`` (swap_face_fine/Blender/model_center/backbone.py)
at the reference's default arguments, or ``SmallFPN``; eval mode, forward only (``blender_fpn``, ``blender_features``, ``blender_forward``).  Its 19
convolutions (five of the encoder, seven of the blocks, one gamma | beta per norm) run on csrc/conv.hip's three-way split-bf16 kernel, the glue on csrc/spade.hip.  That convolution pads with zeros only; the SPADE blocks pad
by reflection, so the glue WRITES reflection-padded planes and the convolution runs on them with ``pad=0``:

    encoder layer      x = leaky0.2(inorm(conv(x)))               e4s_plane_stats, then e4s_spade_modulate without gamma / beta; layer5 without the activation
    shared MLPs        actv_n = relu(conv3x3(reflpad1(nearest(img))))   all seven norms in one launch (e4s_spade_shared), written padded: gamma and beta
                                                                  depend on the image alone
    SPADE norm         gamma | beta = one convolution 128 -> 2C on actv_n's padded slice; act(inorm(x) (1 + gamma) + beta) in e4s_spade_modulate, padded for
                       conv_0 / conv_1 (leaky), unpadded with the identity for the 1x1 conv_s
    block              out = conv_1(...) + bias + x_s in one epilogue (the convolution's residual pointer); norm_0 and norm_s share the statistics of x

Spectral norm in eval mode makes no power iteration: ``weight_orig / (u . W v)`` is folded on the host in float64 when the weights are prepared.

Row f11, stage 4 — the Real-ESRGAN step, ``RRDBNet(3, 3, 64, num_block, 32, scale=4)`` between the two wrappers of ``RealESRBatchInfer``
(swap_face_fine/realesr/image_infer.py), forward only (``realesr_forward``, ``realesr_input``, ``realesr_image``).  The network is ``ops_rrdb``'s, shared with row f16, at width 64 and scale 4; the two ends of
``RealESRBatchInfer`` around it are here, on csrc/rrdb.hip (``e4s_esr_input``, ``e4s_esr_tail``).
"""
from __future__ import annotations

import ctypes
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops_rrdb
from ._lib import lib
from .lossnet import bn_fold, conv_sb, fold_conv_bn, prep_fwd
from .netweights import PreparedNet, _Net, _cuda_checked, _devices_checked, _keys_shapes, _tensor_checked, _validated, prepare
from .ops import _p, _stream
from .ops_post import GREY_MORPH_MAX_RADIUS, grey_dilate
from .ops_rrdb import GpenSRNet

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


def resunet_state_dict_shapes(width: int = 64):
    """``{key: shape}`` of ``ResUNet(width).state_dict()``, in its order."""
    return dict(_keys_shapes(ResUNet, width))


def _resunet_width(name, sd):
    first = sd.get("input_encoder_layer.conv1.weight")
    if first is None:
        raise KeyError(f"{name}: the weights lack 'input_encoder_layer.conv1.weight': expected the keys of ResUNet (ops.resunet_state_dict_shapes())")
    width = int(first.shape[0])
    if width not in RESUNET_WIDTHS or tuple(first.shape[1:]) != (RESUNET_IN_CHANNELS, 3, 3):
        raise ValueError(f"{name}: the first convolution is {tuple(first.shape)}: the network's width must be one of {RESUNET_WIDTHS}")
    return width


_RESUNET_NET = _Net("ResUNet", resunet_state_dict_shapes, ("unet.",), False, ("input_encoder_layer.conv1.weight",), _resunet_width,
                "batch statistics are not offered", ("num_batches_tracked",))


def resunet_weight_tensors(weights):
    """The float tensors of the network (``num_batches_tracked`` aside), in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated("blender_unet", weights, _RESUNET_NET)[2]


class PreparedResUNet(PreparedNet):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage.  Per block: ``pre`` the float32 (scale, shift) of
    the pre-activation BatchNorm (None for the input block), ``conv1`` with the BatchNorm after it and its own bias folded in (float64), ``conv2`` and
    ``sqz`` with their biases, all as three-way split slabs; ``head`` the output convolution's weight [3, width] and bias."""

    __slots__ = ()
    _entry, _net = "blender_unet", _RESUNET_NET

    def _build(self, sd, width, dev):
        blocks = {}
        for name in ("input_encoder_layer",) + _ENCODER + _DECODER:
            first = name == "input_encoder_layer"
            pre = None
            if not first:
                s, t = bn_fold(sd, name + ".bn1")
                pre = (s.float().contiguous(), t.float().contiguous())
            blocks[name] = dict(pre=pre, stride=2 if name in _ENCODER else 1,
                                conv1=prep_fwd(sd[name + ".conv1.weight"], *fold_conv_bn(sd, name + ".conv1", name + (".bn1" if first else ".bn2"))),
                                conv2=prep_fwd(sd[name + ".conv2.weight"], None, sd[name + ".conv2.bias"]),
                                sqz=prep_fwd(sd[name + ".sqz_layer.weight"], None, sd[name + ".sqz_layer.bias"]))
        head = (sd["output_decoder_layer.0.weight"].reshape(3, width).contiguous(), sd["output_decoder_layer.0.bias"].contiguous())
        return dict(width=width, blocks=blocks, head=head)


def _block(B, x, act, x1=None):
    """conv1 (+ folded BatchNorm, ReLU) on ``act``, the 1x1 shortcut on the raw input (``x``, or ``x`` and ``x1``), conv2 + bias + shortcut."""
    c1 = conv_sb(act, *B["conv1"], k=3, stride=B["stride"], relu=True)
    shortcut = conv_sb(x, *B["sqz"], k=1, stride=B["stride"], x1=x1)
    return conv_sb(c1, *B["conv2"], k=3, residual=shortcut)


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


def _unet(name, packages, weights, checked=None):
    """``blender_unet`` under the caller's name; ``checked``: the caller's own ``_validated`` weights."""
    _tensor_checked(name, "packages", packages, torch.float32, 4, f"float32 [bs, {RESUNET_IN_CHANNELS}, H, W] packages")
    bs, c, H, W = packages.shape
    if c != RESUNET_IN_CHANNELS:
        raise ValueError(f"{name}: packages: expected float32 [bs, {RESUNET_IN_CHANNELS}, H, W] packages, got {tuple(packages.shape)}")
    if H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"{name}: packages are {H} x {W}: both sizes must be multiples of 8 (three stride-2 blocks), at least 8")
    if checked is None:
        checked = _validated(name, weights, _RESUNET_NET)
    _devices_checked(name, "packages", packages, checked[2])
    _cuda_checked(name, packages=packages)
    if bs == 0:
        return torch.empty((0, 3, H, W), dtype=torch.float32, device=packages.device)
    with torch.no_grad():
        return _unet_forward(prepare(PreparedResUNet, weights, checked), packages.detach().contiguous())


def blender_unet(packages: torch.Tensor, weights) -> torch.Tensor:
    """``ResUNet.forward`` (res_u_net.py:96-108) in eval mode on the device: float32 ``[bs, 3, H, W]`` in [0, 1] from the float32 ``[bs, 12, H, W]``
    ``packages`` of ``blender_packages``; ``H`` and ``W`` multiples of 8.  ``weights``: a module with the network's keys (``ResUNet``, the drop-in
    ``res_u_net.ResUNet``) or a mapping; the width is read off them.  Forward only, no gradient.  Every argument is checked before any launch; no host
    synchronisation, the same inputs give the same bits, and after one eager call (which prepares the weights) the call captures in a graph."""
    return _unet("blender_unet", packages, weights)


def _recolor(name, img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau, weights, checked):
    if isinstance(img_t, torch.Tensor) and img_t.dim() == 4 and (img_t.shape[2] % 8 or img_t.shape[3] % 8):
        raise ValueError(f"{name}: images are {img_t.shape[2]} x {img_t.shape[3]}: both sizes must be multiples of 8")
    packages, pair = blender_packages(img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau)
    return _unet(name, packages, weights, checked), packages, pair


def blender_recolor(img_a: torch.Tensor, img_t: torch.Tensor, labels_a: torch.Tensor, labels_t: torch.Tensor, feats_a: torch.Tensor, feats_t: torch.Tensor,
                    tau, weights):
    """``Blender.forward`` after its FPN calls: ``(pred, packages, (inv, inv_target))`` with ``packages`` and the pair from ``blender_packages`` and
    ``pred = blender_unet(packages, weights)``.  ``H`` and ``W`` multiples of 8."""
    name = "blender_recolor"
    return _recolor(name, img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau, weights, _validated(name, weights, _RESUNET_NET))


# ------------------------------------------------------------------------------------------------ row f10: the feature network
FPN_CHANNELS = COLORREF_CHANNELS             # both feature networks end in 256 channels
SPADE_HIDDEN = 128                           # SPADE's nhidden (normalization.py:113)
IN_EPS = 1e-5                                # nn.InstanceNorm2d
_FPN_LAYERS = (("layer1", 3, 64, 1), ("layer2", 64, 128, 2), ("layer3", 128, 256, 1), ("layer4", 256, 512, 2), ("layer5", 512, 512, 1))
_FPN_BLOCKS = (("head_0", 512, 512), ("G_middle_0", 512, 512), ("G_middle_1", 512, 256))
_FPN_PREFIXES = ("referencer.FPN.", "FPN.")


def _fpn_norms():
    """The seven SPADE norms in the order their shared first layers are stacked for ``e4s_spade_shared``."""
    return tuple(f"{b}.{n}" for b, fin, fout in _FPN_BLOCKS for n in ("norm_0", "norm_1") + (("norm_s",) if fin != fout else ()))


class _SPADE(nn.Module):
    """``SPADE('spadeinstance3x3', norm_nc, 3)`` (cmodules/normalization.py:87-155) under the reference's parameter names."""

    def __init__(self, norm_nc: int, label_nc: int = 3):
        super().__init__()
        self.param_free_norm = nn.InstanceNorm2d(norm_nc, affine=False)
        self.mlp_shared = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(label_nc, SPADE_HIDDEN, 3), nn.ReLU())
        self.pad = nn.ReflectionPad2d(1)
        self.mlp_gamma = nn.Conv2d(SPADE_HIDDEN, norm_nc, 3)
        self.mlp_beta = nn.Conv2d(SPADE_HIDDEN, norm_nc, 3)

    def forward(self, x, seg):
        actv = self.pad(self.mlp_shared(F.interpolate(seg, size=x.shape[2:], mode="nearest")))
        return self.param_free_norm(x) * (1 + self.mlp_gamma(actv)) + self.mlp_beta(actv)


class _SPADEBlock(nn.Module):
    """``SPADEResnetBlock(fin, fout, opt)`` (cmodules/architecture.py:19-96) with ``pad_type='nozero'``, spectral norm and no SE layer."""

    def __init__(self, fin: int, fout: int):
        super().__init__()
        self.learned_shortcut = fin != fout
        fmid = min(fin, fout)
        self.pad = nn.ReflectionPad2d(1)
        self.conv_0 = nn.utils.spectral_norm(nn.Conv2d(fin, fmid, 3))
        self.conv_1 = nn.utils.spectral_norm(nn.Conv2d(fmid, fout, 3))
        if self.learned_shortcut:
            self.conv_s = nn.utils.spectral_norm(nn.Conv2d(fin, fout, 1, bias=False))
        self.norm_0 = _SPADE(fin)
        self.norm_1 = _SPADE(fmid)
        if self.learned_shortcut:
            self.norm_s = _SPADE(fin)

    def forward(self, x, seg):
        x_s = self.conv_s(self.norm_s(x, seg)) if self.learned_shortcut else x
        dx = self.conv_0(self.pad(F.leaky_relu(self.norm_0(x, seg), 0.2)))
        dx = self.conv_1(self.pad(F.leaky_relu(self.norm_1(dx, seg), 0.2)))
        return x_s + dx


class BlenderFPN(nn.Module):
    """The recolouring network's feature network, ``AdaptiveFeatureGenerator`` (backbone.py:13-79) at the reference's default arguments, with its
    ``state_dict`` keys and shapes (``latest_netG.pth``'s ``referencer.FPN.*`` entries, the prefix taken off, load with ``strict=True``): five
    spectral-normalised convolutions with InstanceNorm and LeakyReLU(0.2) between them, then three SPADE residual blocks conditioned on the image itself.
    ``forward`` is the plain PyTorch composition — what the tests and the timing compare ``blender_fpn`` with; ``blender_fpn(img, module)`` runs the same
    weights on the HIP kernels.  In eval mode spectral norm makes no power iteration: the weight is ``weight_orig / (u . W v)``."""

    def __init__(self):
        super().__init__()
        for name, cin, cout, stride in _FPN_LAYERS:
            setattr(self, name, nn.Sequential(nn.utils.spectral_norm(nn.Conv2d(cin, cout, 3, stride, 1, bias=False)), nn.InstanceNorm2d(cout, affine=False)))
        self.actvn = nn.LeakyReLU(0.2, False)
        for name, fin, fout in _FPN_BLOCKS:
            setattr(self, name, _SPADEBlock(fin, fout))

    def forward(self, img, seg=None):
        seg = img if seg is None else seg
        x = self.layer1(img)
        for name, *_ in _FPN_LAYERS[1:]:
            x = getattr(self, name)(self.actvn(x))
        for name, *_ in _FPN_BLOCKS:
            x = getattr(self, name)(x, seg)
        return x


class SmallFPN(nn.Module):
    """``SmallFPN`` (backbone.py:82-90), the feature network of ``small_FPN``: two 1x1 stride-2 convolutions with bias, 3 -> 256 -> 256."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, FPN_CHANNELS, 1, stride=2, padding=0)
        self.conv2 = nn.Conv2d(FPN_CHANNELS, FPN_CHANNELS, 1, stride=2, padding=0)

    def forward(self, x, y=None):
        return self.conv2(self.conv1(x))


class BlenderNet(nn.Module):
    """A holder with the layout of ``Blender`` (blener.py) and of ``latest_netG.pth``: ``referencer.trainable_tao``, ``referencer.FPN.*``, ``unet.*``.
    It has no forward of its own: ``blender_forward(..., weights=BlenderNet().eval())``."""

    def __init__(self, small_FPN: bool = False):
        super().__init__()
        self.referencer = nn.Module()
        self.referencer.trainable_tao = nn.Parameter(torch.tensor(1.))
        self.referencer.FPN = SmallFPN() if small_FPN else BlenderFPN()
        self.unet = ResUNet(16 if small_FPN else 64)


def fpn_state_dict_shapes(small: bool = False):
    """``{key: shape}`` of ``BlenderFPN().state_dict()`` (``SmallFPN()`` with ``small``), in its order."""
    return dict(_keys_shapes(SmallFPN if small else BlenderFPN))


def _fpn_small(name, sd):
    if "layer1.0.weight_orig" in sd:
        return False
    if "conv1.weight" in sd:
        return True
    raise KeyError(f"{name}: the weights have neither 'layer1.0.weight_orig' (BlenderFPN) nor 'conv1.weight' (SmallFPN): expected the keys of "
                   f"ops.fpn_state_dict_shapes(), bare or prefixed with one of {_FPN_PREFIXES}")


_FPN_NET = _Net("BlenderFPN / SmallFPN", fpn_state_dict_shapes, _FPN_PREFIXES, False, ("layer1.0.weight_orig", "conv1.weight"), _fpn_small,
            "spectral norm's power iteration is not offered", ())


def fpn_weight_tensors(weights, name: str = "blender_fpn"):
    """The tensors of the feature network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _FPN_NET)[2]


def _sigma_folded(sd, prefix):
    """Eval-mode spectral norm: ``weight_orig / sigma`` with ``sigma = u . (W_mat v)`` from the stored vectors, formed in float64, as float32."""
    w = sd[prefix + ".weight_orig"].double()
    sigma = torch.dot(sd[prefix + ".weight_u"].double(), torch.mv(w.reshape(w.shape[0], -1), sd[prefix + ".weight_v"].double()))
    return (w / sigma).float()


class PreparedFPN(PreparedNet):
    """The kernels' copies of a feature network's weights, rebuilt when a tensor changes version or storage.  ``BlenderFPN``: ``layers`` the five
    convolutions with sigma folded in, per block ``conv_0`` / ``conv_1`` (with bias) and ``conv_s`` likewise and per norm the gamma and beta convolutions
    concatenated into one of ``2 C`` outputs, all as three-way split slabs; ``shared`` the first layers of the seven norms stacked ``[7 * 128, 3, 3, 3]``
    with their biases.  ``SmallFPN``: its two convolutions."""

    __slots__ = ()
    _entry, _net = "blender_fpn", _FPN_NET

    def _build(self, sd, small, dev):
        if small:
            return dict(small=True, convs=[prep_fwd(sd[f"{n}.weight"], None, sd[f"{n}.bias"]) for n in ("conv1", "conv2")])
        layers = [dict(conv=prep_fwd(_sigma_folded(sd, name + ".0")), stride=stride) for name, _, _, stride in _FPN_LAYERS]
        norms = _fpn_norms()
        blocks = []
        for name, fin, fout in _FPN_BLOCKS:
            B = dict(conv_0=prep_fwd(_sigma_folded(sd, name + ".conv_0"), None, sd[name + ".conv_0.bias"]),
                     conv_1=prep_fwd(_sigma_folded(sd, name + ".conv_1"), None, sd[name + ".conv_1.bias"]),
                     conv_s=prep_fwd(_sigma_folded(sd, name + ".conv_s")) if fin != fout else None)
            for n in ("norm_0", "norm_1") + (("norm_s",) if fin != fout else ()):
                p = f"{name}.{n}"
                B[n] = (norms.index(p), prep_fwd(torch.cat([sd[p + ".mlp_gamma.weight"], sd[p + ".mlp_beta.weight"]]), None,
                                                 torch.cat([sd[p + ".mlp_gamma.bias"], sd[p + ".mlp_beta.bias"]])))
            blocks.append(B)
        shared = (torch.cat([sd[p + ".mlp_shared.1.weight"] for p in norms]).contiguous(), torch.cat([sd[p + ".mlp_shared.1.bias"] for p in norms]).contiguous())
        return dict(small=False, layers=layers, blocks=blocks, shared=shared, nnorms=len(norms))


def _plane_stats(x):
    bs, c, h, w = x.shape
    mean = torch.empty((bs * c,), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    lib().call("e4s_plane_stats", _p(mean), _p(rstd), None, _p(x), bs * c, h * w, IN_EPS, _stream())
    return mean, rstd


def _modulate(x, stats, gamma_beta, leaky, padded):
    """``e4s_spade_modulate``: act((x - mean) rstd (1 + gamma) + beta), or the plain InstanceNorm without ``gamma_beta``; padded by reflection or not."""
    bs, c, h, w = x.shape
    out = torch.empty((bs, c, h + 2, w + 2) if padded else (bs, c, h, w), dtype=torch.float32, device=x.device)
    lib().call("e4s_spade_modulate", _p(out), _p(x), _p(stats[0]), _p(stats[1]), _p(gamma_beta), bs, c, h, w, 1 if leaky else 0, 1 if padded else 0, _stream())
    return out


def _fpn_forward(P, img):
    if P["small"]:
        return conv_sb(conv_sb(img, *P["convs"][0], k=1, stride=2), *P["convs"][1], k=1, stride=2)
    x = img
    for i, L in enumerate(P["layers"]):                                 # conv -> InstanceNorm -> LeakyReLU; layer5 ends with its InstanceNorm
        y = conv_sb(x, *L["conv"], k=3, stride=L["stride"])
        x = _modulate(y, _plane_stats(y), None, leaky=i + 1 < len(P["layers"]), padded=False)
    bs, _, h, w = x.shape
    # gamma and beta depend on the image alone: the first layers of all seven norms in one launch, each norm's slice a contiguous padded batch
    actv = torch.empty((P["nnorms"], bs, SPADE_HIDDEN, h + 2, w + 2), dtype=torch.float32, device=x.device)
    lib().call("e4s_spade_shared", _p(actv), _p(img), _p(P["shared"][0]), _p(P["shared"][1]), bs, P["nnorms"], img.shape[2], img.shape[3], h, w, _stream())

    def spade(norm, src, stats, leaky, padded):
        idx, gb = norm
        return _modulate(src, stats, conv_sb(actv[idx], *gb, k=3, pad=0), leaky, padded)

    for B in P["blocks"]:
        stats = _plane_stats(x)                                         # norm_0 and norm_s normalise the same x
        dx = conv_sb(spade(B["norm_0"], x, stats, True, True), *B["conv_0"], k=3, pad=0)
        a1 = spade(B["norm_1"], dx, _plane_stats(dx), True, True)
        shortcut = conv_sb(spade(B["norm_s"], x, stats, False, False), *B["conv_s"], k=1) if B["conv_s"] is not None else x
        x = conv_sb(a1, *B["conv_1"], k=3, pad=0, residual=shortcut)
    return x


def fpn_output_size(H: int, W: int):
    """The feature map of an ``H x W`` image: two stride-2 layers (3x3 with padding 1, or SmallFPN's 1x1 without: the same sizes)."""
    return ((H - 1) // 2 + 1 - 1) // 2 + 1 if H >= 1 else 0, ((W - 1) // 2 + 1 - 1) // 2 + 1 if W >= 1 else 0


def _fpn_image_checked(name, nm, img):
    _tensor_checked(name, nm, img, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    if img.shape[1] != 3:
        raise ValueError(f"{name}: {nm}: expected a float32 [bs, 3, H, W] image, got {tuple(img.shape)}")
    h, w = fpn_output_size(img.shape[2], img.shape[3])
    if h < 2 or w < 2:
        raise ValueError(f"{name}: {nm} is {img.shape[2]} x {img.shape[3]}: its feature map would be {h} x {w}, reflection padding needs at least 2 x 2")
    return h, w


def _fpn_checked_all(name, weights, **images):
    """Every check of a feature-network call, once; returns the validated weights for ``_fpn_prepared``."""
    checked = _validated(name, weights, _FPN_NET)
    for nm, img in images.items():
        _fpn_image_checked(name, nm, img)
    shapes = {tuple(img.shape) for img in images.values()}
    if len(shapes) != 1:
        raise ValueError(f"{name}: the images differ in shape: {sorted(shapes)}")
    for nm, img in images.items():
        _devices_checked(name, nm, img, checked[2])
    _cuda_checked(name, **images)
    return checked


def _fpn_run(img, prepared):
    """``prepared``: a callable that gives the prepared weights (not called for an empty batch, which has nothing to launch)."""
    bs, _, H, W = img.shape
    if bs == 0:
        return torch.empty((0, FPN_CHANNELS) + fpn_output_size(H, W), dtype=torch.float32, device=img.device)
    with torch.no_grad():
        return _fpn_forward(prepared(), img.detach().contiguous())


def _features_run(img_a, img_t, weights, checked, flip_target):
    """The two FPN calls on weights validated by the caller and prepared once for both."""
    P = []

    def prepared():
        if not P:
            P.append(prepare(PreparedFPN, weights, checked))
        return P[0]

    feats_a = _fpn_run(img_a, prepared)
    return feats_a, _fpn_run(torch.flip(img_t, dims=[-1]) if flip_choice(flip_target) else img_t, prepared)


def blender_fpn(img: torch.Tensor, weights) -> torch.Tensor:
    """``AdaptiveFeatureGenerator.forward(img, img)`` (backbone.py:60-79, the reference's default arguments) or ``SmallFPN.forward`` in eval mode on the
    device: float32 ``[bs, 256, h, w]`` features of a float32 ``[bs, 3, H, W]`` image, ``h = ceil(ceil(H / 2) / 2)`` (at least 2).  ``weights``: a module
    with a feature network's keys (``BlenderFPN``, ``SmallFPN``, the drop-ins of ``backbone.py``) in eval mode, or a mapping, bare or with the keys of
    ``latest_netG.pth`` (``referencer.FPN.``) or of the referencer (``FPN.``); which of the two networks is read off the keys.  A module's prepared weights
    are cached per parameter version; a mapping is prepared on every call.  Forward only, no gradient.  Every argument is checked before any launch; no
    host synchronisation, the same inputs give the same bits, and after one eager call (which prepares the weights) the call captures in a graph."""
    checked = _fpn_checked_all("blender_fpn", weights, img=img)
    return _fpn_run(img, lambda: prepare(PreparedFPN, weights, checked))


def flip_choice(flip_target=None) -> bool:
    """Whether the target is mirrored before its features are taken.  ``None`` is ``Referencer.forward``'s rule (referencer.py:32-35): one
    ``np.random.rand()``, no flip below 0.5."""
    if flip_target is None:
        import numpy as np
        return not np.random.rand() < 0.5
    if not isinstance(flip_target, bool):
        raise TypeError(f"flip_target is True, False or None, got {type(flip_target).__name__}")
    return flip_target


def blender_features(img_a: torch.Tensor, img_t: torch.Tensor, weights, flip_target=None):
    """The two FPN calls of ``Referencer.forward`` (referencer.py:29-36): ``(feats_a, feats_t)``, each exactly ``blender_fpn`` of ``img_a`` and of ``img_t``
    or, when the target is flipped, of ``flip(img_t, -1)``; the features are not flipped back (the reference's line that would is commented out).
    ``flip_target`` True / False decides; ``None`` draws like the reference (``flip_choice``), after the first call as it does, so a caller who seeds NumPy
    gets the reference's choice."""
    name = "blender_features"
    if flip_target is not None and not isinstance(flip_target, bool):
        raise TypeError(f"{name}: flip_target is True, False or None, got {type(flip_target).__name__}")
    return _features_run(img_a, img_t, weights, _fpn_checked_all(name, weights, img_a=img_a, img_t=img_t), flip_target)


def _blender_weights(name, weights):
    """(FPN weights, tau, Res-U-Net weights) of a module or mapping with ``latest_netG.pth``'s layout."""
    if isinstance(weights, nn.Module):
        if weights.training:
            raise RuntimeError(f"{name}: {type(weights).__name__} is in training mode: call .eval()")
        ref = getattr(weights, "referencer", None)
        if ref is None or not hasattr(ref, "FPN") or not hasattr(ref, "trainable_tao") or not hasattr(weights, "unet"):
            raise TypeError(f"{name}: {type(weights).__name__} has no referencer.FPN, referencer.trainable_tao and unet (the layout of Blender)")
        return ref.FPN, ref.trainable_tao.detach(), weights.unet
    if not hasattr(weights, "keys"):
        raise TypeError(f"{name}: weights must be a module or a mapping with the layout of latest_netG.pth, got {type(weights).__name__}")
    if "referencer.trainable_tao" not in weights:
        raise KeyError(f"{name}: the weights lack 'referencer.trainable_tao': expected the keys of latest_netG.pth (referencer.FPN.*, unet.*)")
    return weights, weights["referencer.trainable_tao"].detach(), weights


def blender_forward(img_a: torch.Tensor, img_t: torch.Tensor, labels_a: torch.Tensor, labels_t: torch.Tensor, weights, flip_target=None):
    """The whole of ``Blender.forward`` (blener.py:13-24) on the device: ``(pred, packages, (inv, inv_target))`` = ``blender_features`` followed by
    ``blender_recolor`` with ``tau = referencer.trainable_tao`` (read by the kernel, never on the host).  ``weights``: a module (``BlenderNet``, the
    reference's ``Blender`` over the drop-ins) in eval mode or a mapping with ``latest_netG.pth``'s layout: ``referencer.FPN.*``,
    ``referencer.trainable_tao``, ``unet.*``.  Images float32 ``[bs, 3, H, W]`` with ``H`` and ``W`` multiples of 8, labels uint8 ``[bs, H, W]``."""
    name = "blender_forward"
    fpn, tau, unet = _blender_weights(name, weights)
    if flip_target is not None and not isinstance(flip_target, bool):
        raise TypeError(f"{name}: flip_target is True, False or None, got {type(flip_target).__name__}")
    unet_checked = _validated(name, unet, _RESUNET_NET)
    for nm, t in (("img_a", img_a), ("img_t", img_t)):
        _fpn_image_checked(name, nm, t)
    if img_t.shape[2] % 8 or img_t.shape[3] % 8:
        raise ValueError(f"{name}: images are {img_t.shape[2]} x {img_t.shape[3]}: both sizes must be multiples of 8")
    _labels_checked(name, labels_a, labels_t)
    checked = _fpn_checked_all(name, fpn, img_a=img_a, img_t=img_t)
    _cuda_checked(name, labels_a=labels_a, labels_t=labels_t)
    if tau.numel() != 1 or tau.dtype != torch.float32 or tau.device != img_t.device:
        raise ValueError(f"{name}: referencer.trainable_tao is one float32 element on the images' device, got {tau.dtype} {tuple(tau.shape)} on {tau.device}")
    feats_a, feats_t = _features_run(img_a, img_t, fpn, checked, flip_target)
    return _recolor(name, img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau.reshape(1), unet, unet_checked)


# ------------------------------------------------------------------------------------------------ row f11: the Real-ESRGAN step
class RRDBNet(GpenSRNet):
    """``RRDBNet(3, 3, num_feat=64, num_block, num_grow_ch=32, scale=4)`` of basicsr's rrdbnet_arch, the only configuration the reference builds, with its
    ``state_dict`` keys and shapes (``RealESRGAN_x4plus.pth``'s ``params_ema``, load with ``strict=True``): 702 tensors at 23 blocks.  ``ops_rrdb``'s mirror
    module at width 64 and scale 4; ``forward`` is the plain PyTorch composition — what the tests and the timing compare ``realesr_forward`` with;
    ``realesr_forward(x, module)`` runs the same weights on the HIP kernels."""

    def __init__(self, num_block: int = 23):
        ops_rrdb._config_checked("RRDBNet", num_block, 64, 4)
        super().__init__(num_block, 64, 4)


def rrdbnet_state_dict_shapes(num_block: int = 23):
    """``{key: shape}`` of ``RRDBNet(num_block).state_dict()``, in its order."""
    return dict(_keys_shapes(RRDBNet, num_block))


# the block count is the whole variant: any other width or scale fails the shapes of ``rrdbnet_state_dict_shapes``
_RRDB_NET = _Net("RRDBNet", rrdbnet_state_dict_shapes, ops_rrdb._PREFIXES, True, ("conv_first.weight",),
                 functools.partial(ops_rrdb._blocks, shapes="rrdbnet_state_dict_shapes"), None, ())


def rrdbnet_weight_tensors(weights, name: str = "realesr_forward"):
    """The tensors of the network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _RRDB_NET)[2]


class PreparedRRDBNet(ops_rrdb._PreparedRRDB):
    """``ops_rrdb._PreparedRRDB`` for the network at width 64 and scale 4."""

    __slots__ = ()
    _entry, _net = "realesr_forward", _RRDB_NET


def _rrdb_run(x, P, want_float, want_u8):
    """``ops_rrdb._run`` with ``e4s_esr_tail`` at its end: (float32 [bs, 3, 4h, 4w] or None, uint8 [bs, 4h, 4w, 3] or None) of ``x [bs, 3, h, w]``."""
    return ops_rrdb._run(x, P, want_float, (4 * x.shape[2], 4 * x.shape[3]) if want_u8 else None, ("e4s_esr_tail", (), ()))


def _rrdb_checked_all(name, x, weights):
    checked = _validated(name, weights, _RRDB_NET)
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, 3, h, w] image")
    if x.shape[1] != 3 or x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError(f"{name}: x: expected a float32 [bs, 3, h, w] image with h, w >= 1, got {tuple(x.shape)}")
    if 4 * x.shape[2] > 16384 or 4 * x.shape[3] > 16384:
        raise ValueError(f"{name}: x is {x.shape[2]} x {x.shape[3]}: the x4 output may be 16384 x 16384 at the most")
    _devices_checked(name, "x", x, checked[2])
    _cuda_checked(name, x=x)
    return checked


def realesr_forward(x: torch.Tensor, weights) -> torch.Tensor:
    """``RRDBNet.forward`` at scale 4 (basicsr's rrdbnet_arch, as ``RealESRBatchInfer`` builds it) in eval mode on the device: float32 ``[bs, 3, 4h, 4w]`` from
    a float32 ``[bs, 3, h, w]`` image, ``h, w >= 1``.  ``weights``: a module with the network's keys (``RRDBNet``) or a mapping, bare or the checkpoint with
    ``params_ema`` / ``params``; the block count is read off the keys.  A module's prepared weights are cached per parameter version; a mapping is prepared
    on every call.  The 351 convolutions run on the three-way split-bf16 kernel except conv_last, which is exact float32 (``e4s_esr_tail``).  The samples of
    a batch run one after another on scratch that does not grow with ``bs``, each exactly as a batch-of-one call.  Forward only, no gradient.  Every argument
    is checked before any launch; no host synchronisation, the same inputs give the same bits, and after one eager call (which prepares the weights) the
    call captures in a graph."""
    name = "realesr_forward"
    checked = _rrdb_checked_all(name, x, weights)
    bs, _, h, w = x.shape
    if bs == 0:
        return torch.empty((0, 3, 4 * h, 4 * w), dtype=torch.float32, device=x.device)
    with torch.no_grad():
        return _rrdb_run(x.detach().contiguous(), prepare(PreparedRRDBNet, weights, checked), True, False)[0]


def realesr_input(img_u8: torch.Tensor, out_hw, name: str = "realesr_input") -> torch.Tensor:
    """The head of ``RealESRBatchInfer.infer_image`` and ``infer_batch`` (image_infer.py:64-65, :73-76) in one pass (``e4s_esr_input``): uint8
    ``[bs, H, W, 3]`` to float32 ``[bs, 3, *out_hw]`` = the ``align_corners=True`` bilinear resize of ``clamp((v / 127.5 - 1) * 0.5 + 0.5, 0, 1)``."""
    _tensor_checked(name, "img_u8", img_u8, torch.uint8, 4, "a uint8 [bs, H, W, 3] image")
    bs, H, W, c3 = img_u8.shape
    if c3 != 3 or H < 1 or W < 1 or H > 16384 or W > 16384:
        raise ValueError(f"{name}: img_u8: expected a uint8 [bs, H, W, 3] image with 1 <= H, W <= 16384, got {tuple(img_u8.shape)}")
    oh, ow = out_hw
    for v in (oh, ow):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 4096:
            raise ValueError(f"{name}: the network's input size is a pair of ints in 1..4096, got {out_hw!r}")
    _cuda_checked(name, img_u8=img_u8)
    x = torch.empty((bs, 3, oh, ow), dtype=torch.float32, device=img_u8.device)
    lib().call("e4s_esr_input", _p(x), _p(img_u8.contiguous()), bs, H, W, oh, ow, _stream())
    return x


def realesr_image(img_u8: torch.Tensor, weights, in_size: int = 256) -> torch.Tensor:
    """``RealESRBatchInfer.infer_image`` (image_infer.py:71-80) for a batch on the device, as three fused steps: ``realesr_input`` (``/ 127.5 - 1``,
    ``* 0.5 + 0.5``, the clamp and the ``align_corners=True`` bilinear resize to ``in_size``), the network, and ``e4s_esr_tail`` (conv_last, ``* 2 - 1``, the
    clamp, ``* 127.5 + 127.5``, the clamp and the truncation).  uint8 ``[bs, H, W, 3]`` to uint8 ``[bs, 4 in_size, 4 in_size, 3]``."""
    name = "realesr_image"
    checked = _validated(name, weights, _RRDB_NET)
    if isinstance(img_u8, torch.Tensor):
        _devices_checked(name, "img_u8", img_u8, checked[2])
    with torch.no_grad():
        x = realesr_input(img_u8, (in_size, in_size), name)
        if x.shape[0] == 0:
            return torch.empty((0, 4 * in_size, 4 * in_size, 3), dtype=torch.uint8, device=x.device)
        return _rrdb_run(x, prepare(PreparedRRDBNet, weights, checked), False, True)[1]


__all__ = ["BLENDER_PARTS", "BLENDER_PART_IDS", "COLORREF_CHANNELS", "COLORREF_MAX_PIXELS", "blender_part_masks", "color_reference", "blender_packages",
           "RESUNET_WIDTHS", "ResUNet", "PreparedResUNet", "resunet_state_dict_shapes", "resunet_weight_tensors", "blender_unet", "blender_recolor",
           "FPN_CHANNELS", "BlenderFPN", "SmallFPN", "BlenderNet", "PreparedFPN", "fpn_state_dict_shapes", "fpn_weight_tensors", "fpn_output_size",
           "flip_choice", "blender_fpn", "blender_features", "blender_forward",
           "RRDBNet", "PreparedRRDBNet", "rrdbnet_state_dict_shapes", "rrdbnet_weight_tensors", "realesr_forward", "realesr_input", "realesr_image"]
