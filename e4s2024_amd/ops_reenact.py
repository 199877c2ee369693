"""Row f17: face-vid2vid reenactment, stage 1 — everything that turns images into the two keypoint sets the generator consumes: ``KPDetector`` and
``HEEstimator`` of swap_face_fine/face_vid2vid/modules/keypoint_detector.py (with the blocks of modules/util.py) in eval mode, and ``keypoint_transformation``
with ``headpose_pred_to_degree`` and ``get_rotation_matrix`` of drive_demo.py:67-180.

    KPDetector     e4s_v2v_antialias_down (pad, 13 x 13 Gaussian and [::4, ::4] in one pass, exact float32)
                   DownBlock2d: conv 3 x 3 + folded BatchNorm + ReLU (the 3-channel first one on the exact e4s_conv2d, the others on e4s_conv2d_sb3), e4s_avgpool2x2
                   the 1 x 1 convolution on e4s_conv2d_sb3; its output [bs, C D, h, w] IS the volume [bs, C, D, h, w]
                   UpBlock3d: e4s_conv3d_sb3 with up_hw = 2 (the nearest (1, 2, 2) upsampling is in the gather), BatchNorm folded in float64, ReLU
                   the kp (and jacobian) heads: e4s_conv3d_sb3 with bias; e4s_v2v_heatmap_kp: softmax(logit / temperature) over the volume and its expectations
    HEEstimator    conv1 7 x 7 stride 2 on the exact e4s_conv2d + folded BatchNorm + ReLU, e4s_maxpool3x3s2, every 1 x 1 / 3 x 3 convolution on e4s_conv2d_sb3 with
                   its bias and BatchNorm folded in float64, ReLU and the residual add fused; e4s_plane_stats as the global average pool; the five linear heads as
                   one e4s_vec_fc (exact float32 products)
    transformation e4s_v2v_kp_transform: degrees, rotation matrix, transformed keypoints and Jacobians in one launch per batch

The reference's oddities are kept: ``yaw = fc_roll(out)`` and ``roll = fc_yaw(out)``, degrees ``sum(p idx) 3 - 99``, radians through 3.14, ``rot = pitch_mat
yaw_mat roll_mat``.  One difference: the reference's ``keypoint_transformation`` reshapes the caller's ``he['t']`` in place to ``[bs, 1, 3]`` (``unsqueeze_``);
here ``he`` is left as it was.

Row f18, stage 2, is the second half of this module: ``DenseMotionNetwork`` of modules/dense_motion.py (``dense_motion_forward``; its own overview stands in front
of it).  Row f19, stage 3, is the third: ``OcclusionAwareSPADEGenerator`` of modules/generator.py in front of its decoder (``appearance_feature``, once per
clip, and ``generator_warp``, per frame; their overview stands in front of them).

Forward only; no host synchronisation; the same inputs give the same bits; after one eager call (which prepares the weights) a call captures in a graph."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lossnet
from ._lib import lib
from .lossnet import conv_exact, conv_sb, fold_conv_bn, prep_exact, prep_fwd
from .ops import _c, _p, _req, _stream
from .netweights import EVAL_ONLY, PreparedNet, _Net, _cuda_checked, _placed_checked, _tensor_checked, _validated, bn_shapes, check_loaded, module_net, prepare

NUM_BINS = 66                                # headpose_pred_to_degree's idx_tensor is range(66) whatever the module's num_bins


# ------------------------------------------------------------------------------------------------ configuration arithmetic
def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def antialias_kernel(scale_factor) -> torch.Tensor:
    """``AntiAliasInterpolation2d(channels, scale).weight[0, 0]``: sigma = (1 / scale - 1) / 2, k = 2 round(4 sigma) + 1, the normalised float32 Gaussian."""
    sigma = (1 / scale_factor - 1) / 2
    k = 2 * round(sigma * 4) + 1
    ax = torch.arange(k, dtype=torch.float32)
    g = torch.exp(-(ax - (k - 1) / 2) ** 2 / (2 * sigma ** 2))
    kernel = g[:, None] * g[None, :]                 # the reference multiplies the two meshgrid factors into 1: rows first
    return kernel / torch.sum(kernel)


def kp_detector_structure(block_expansion=32, num_kp=15, image_channel=3, max_features=1024, reshape_channel=16384, reshape_depth=16, num_blocks=5,
                          estimate_jacobian=False, scale_factor=0.25, single_jacobian_map=False):
    """The constructor arithmetic of ``KPDetector`` / ``KPHourglass`` as ``(image_channel, down widths, reshape_depth, up widths, num_kp, jacobian maps,
    anti-alias kernel size or 0, its stride)``; refuses what the native path does not implement."""
    if not all(_is_int(v) for v in (block_expansion, num_kp, image_channel, max_features, reshape_channel, reshape_depth, num_blocks)):
        raise ValueError("KPDetector: block_expansion, num_kp, image_channel, max_features, reshape_channel, reshape_depth and num_blocks are ints")
    if min(block_expansion, num_kp, max_features, reshape_channel, reshape_depth, num_blocks) < 1:
        raise ValueError("KPDetector: widths, depths and counts are positive")
    if image_channel != 3:
        raise ValueError(f"KPDetector: image_channel {image_channel} is not implemented: the native network takes three colour channels")
    if single_jacobian_map:
        raise ValueError("KPDetector: single_jacobian_map=True is not implemented: the native path keeps one Jacobian map per keypoint")
    inv = 1.0 / float(scale_factor) if scale_factor and scale_factor > 0 else 0.0
    if inv < 1 or abs(inv - round(inv)) > 1e-9:
        raise ValueError(f"KPDetector: scale_factor {scale_factor!r} is not implemented: its inverse must be an integer (1, 0.5, 0.25, ...)")
    width = lambda i: min(max_features, block_expansion * 2 ** i)      # noqa: E731
    if reshape_channel != reshape_depth * width(num_blocks):
        raise ValueError(f"KPDetector: reshape_channel {reshape_channel} breaks reshape_channel == reshape_depth * min(max_features, block_expansion * "
                         f"2 ** num_blocks) = {reshape_depth} * {width(num_blocks)}: the 1 x 1 convolution's output is reshaped to that volume")
    if reshape_depth < 2:
        raise ValueError(f"KPDetector: reshape_depth {reshape_depth}: every extent of the final volume must be at least 2 (the coordinate grid divides by n - 1)")
    down = tuple(width(i + 1) for i in range(num_blocks))
    up = tuple(width(num_blocks - i - 1) for i in range(num_blocks))
    s = int(round(inv))
    k = 0 if s == 1 else 2 * round((s - 1) / 2 * 4) + 1
    return int(image_channel), down, int(reshape_depth), up, int(num_kp), int(num_kp) if estimate_jacobian else 0, int(k), s


def kp_volume_size(structure, H: int, W: int):
    """(D, H', W') of the heatmap volume for an H x W input."""
    _, down, depth, up, _, _, k, s = structure
    if k:
        H, W = -(-H // s), -(-W // s)
    for _ in down:
        H, W = H // 2, W // 2
    return depth, H * 2 ** len(up), W * 2 ** len(up)


# ------------------------------------------------------------------------------------------------ the modules: the reference's keys, a stock-PyTorch forward
class _DownBlock2d(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm = nn.BatchNorm2d(cout, affine=True)

    def forward(self, x):
        return F.avg_pool2d(F.relu(self.norm(self.conv(x))), 2)


class _UpBlock3d(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 3, padding=1)
        self.norm = nn.BatchNorm3d(cout, affine=True)

    def forward(self, x):
        return F.relu(self.norm(self.conv(F.interpolate(x, scale_factor=(1, 2, 2)))))


class _KPHourglass(nn.Module):
    def __init__(self, structure):
        super().__init__()
        cin, down, depth, up, _, _, _, _ = structure
        self.down_blocks = nn.Sequential()
        for i, c in enumerate(down):
            self.down_blocks.add_module(f"down{i}", _DownBlock2d(cin if i == 0 else down[i - 1], c))
        self.conv = nn.Conv2d(down[-1], depth * down[-1], 1)
        self.up_blocks = nn.Sequential()
        for i, c in enumerate(up):
            self.up_blocks.add_module(f"up{i}", _UpBlock3d(down[-1] if i == 0 else up[i - 1], c))
        self.reshape_depth, self.out_filters = depth, up[-1]

    def forward(self, x):
        out = self.conv(self.down_blocks(x))
        bs, c, h, w = out.shape
        return self.up_blocks(out.view(bs, c // self.reshape_depth, self.reshape_depth, h, w))


class _AntiAlias(nn.Module):
    """``AntiAliasInterpolation2d(channels, scale)``: its buffer ``weight [channels, 1, k, k]``."""

    def __init__(self, channels, scale):
        super().__init__()
        kernel = antialias_kernel(scale)
        self.register_buffer("weight", kernel.view(1, 1, *kernel.shape).repeat(channels, 1, 1, 1))
        self.groups, self.stride, self.pad = channels, int(round(1 / scale)), kernel.shape[0] // 2

    def forward(self, x):
        out = F.conv2d(F.pad(x, (self.pad,) * 4), self.weight, groups=self.groups)
        return out[:, :, ::self.stride, ::self.stride]


class _Loadable(nn.Module):
    """Random weights until ``load_state_dict`` has filled the module: the native entries refuse it before."""
    _PROBE = ()

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if all(k in state_dict for k in self._PROBE):
            self._loaded = True
        return out


class KPDetector(_Loadable):
    """``KPDetector(block_expansion, feature_channel, num_kp, image_channel, max_features, reshape_channel, reshape_depth, num_blocks, temperature,
    estimate_jacobian, scale_factor, single_jacobian_map)`` of swap_face_fine/face_vid2vid/modules/keypoint_detector.py with its ``state_dict`` keys, shapes and
    order; the defaults are the upstream ``vox-256.yaml`` (75 tensors, the buffer ``down.weight`` included; ``checkpoint['kp_detector']`` loads with
    ``strict=True``).  ``forward`` is the plain PyTorch composition in eval mode, returning ``{'value'[, 'jacobian']}`` — what the tests compare
    ``kp_detector_forward`` with; ``kp_detector_forward(x, module)`` runs the same weights on the HIP kernels.  Refused with ``ValueError``:
    ``single_jacobian_map=True``, a ``scale_factor`` whose inverse is no integer, a ``reshape_channel`` other than ``reshape_depth * min(max_features,
    block_expansion * 2 ** num_blocks)``, ``reshape_depth < 2``, ``image_channel != 3``."""
    _PROBE = ("predictor.conv.weight", "kp.weight")

    def __init__(self, block_expansion=32, feature_channel=32, num_kp=15, image_channel=3, max_features=1024, reshape_channel=16384, reshape_depth=16,
                 num_blocks=5, temperature=0.1, estimate_jacobian=False, scale_factor=0.25, single_jacobian_map=False):
        super().__init__()
        self.structure = kp_detector_structure(block_expansion, num_kp, image_channel, max_features, reshape_channel, reshape_depth, num_blocks,
                                               estimate_jacobian, scale_factor, single_jacobian_map)
        if not float(temperature) > 0:
            raise ValueError(f"KPDetector: temperature {temperature!r} must be positive")
        self.predictor = _KPHourglass(self.structure)
        self.kp = nn.Conv3d(self.predictor.out_filters, num_kp, 3, padding=1)
        if estimate_jacobian:
            self.num_jacobian_maps = num_kp
            self.jacobian = nn.Conv3d(self.predictor.out_filters, 9 * num_kp, 3, padding=1)
            self.jacobian.weight.data.zero_()
            self.jacobian.bias.data.copy_(torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1] * num_kp, dtype=torch.float))
        else:
            self.jacobian = None
        self.temperature, self.scale_factor = temperature, scale_factor
        if self.structure[6]:
            self.down = _AntiAlias(image_channel, scale_factor)
        self.requires_grad_(False)
        self._loaded = False

    def forward(self, x):
        if self.training:
            raise NotImplementedError("KPDetector: training mode is not implemented; call .eval()")
        with torch.no_grad():
            if self.structure[6]:
                x = self.down(x)
            feature_map = self.predictor(x)
            prediction = self.kp(feature_map)
            bs, K, D, H, W = prediction.shape
            if min(D, H, W) < 2:
                raise ValueError(f"KPDetector: the final volume is {D} x {H} x {W}: every extent must be at least 2")
            heatmap = F.softmax(prediction.view(bs, K, -1) / self.temperature, dim=2).view(bs, K, D, H, W)
            ax = lambda n: 2 * (torch.arange(n).type(heatmap.type()) / (n - 1)) - 1      # noqa: E731
            grid = torch.stack((ax(W).view(1, 1, W).expand(D, H, W), ax(H).view(1, H, 1).expand(D, H, W), ax(D).view(D, 1, 1).expand(D, H, W)), 3)
            out = {"value": (heatmap.unsqueeze(-1) * grid[None, None]).sum(dim=(2, 3, 4))}
            if self.jacobian is not None:
                jm = self.jacobian(feature_map).reshape(bs, K, 9, D, H, W)
                out["jacobian"] = (heatmap.unsqueeze(2) * jm).view(bs, K, 9, -1).sum(dim=-1).view(bs, K, 3, 3)
            return out


class _ResBottleneck(nn.Module):
    def __init__(self, c, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(c, c // 4, 1)
        self.conv2 = nn.Conv2d(c // 4, c // 4, 3, padding=1, stride=stride)
        self.conv3 = nn.Conv2d(c // 4, c, 1)
        self.norm1 = nn.BatchNorm2d(c // 4, affine=True)
        self.norm2 = nn.BatchNorm2d(c // 4, affine=True)
        self.norm3 = nn.BatchNorm2d(c, affine=True)
        self.stride = stride
        if stride != 1:
            self.skip = nn.Conv2d(c, c, 1, stride=stride)
            self.norm4 = nn.BatchNorm2d(c, affine=True)

    def forward(self, x):
        out = F.relu(self.norm1(self.conv1(x)))
        out = F.relu(self.norm2(self.conv2(out)))
        out = self.norm3(self.conv3(out))
        if self.stride != 1:
            x = self.norm4(self.skip(x))
        return F.relu(out + x)


# the stages of HEEstimator in key order: (1 x 1 widening convolution + norm, its width), the strided block, the group of stride-1 blocks (name, letter, count)
_HE_STAGES = ((("conv3", "norm3", 512), "block2", ("block3", "b3_", 3)), (("conv4", "norm4", 1024), "block4", ("block5", "b5_", 5)),
              (("conv5", "norm5", 2048), "block6", ("block7", "b7_", 2)))
_HE_HEADS = ("fc_roll", "fc_pitch", "fc_yaw", "fc_t", "fc_exp")


class HEEstimator(_Loadable):
    """``HEEstimator(block_expansion, feature_channel, num_kp, image_channel, max_features, num_bins, estimate_jacobian)`` of keypoint_detector.py:85-178 with
    its keys (402 tensors at the upstream configuration); the widths 256 .. 2048 are the reference's constants, only ``conv1`` follows ``block_expansion``.
    ``forward`` is the plain PyTorch composition in eval mode, returning ``{'yaw', 'pitch', 'roll', 't', 'exp'}`` with the reference's crossed heads
    (``yaw = fc_roll(out)``, ``roll = fc_yaw(out)``)."""
    _PROBE = ("conv1.weight", "fc_exp.weight")

    def __init__(self, block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048, num_bins=66, estimate_jacobian=False):
        super().__init__()
        if not all(_is_int(v) and v >= 1 for v in (block_expansion, num_kp, image_channel, num_bins)):
            raise ValueError("HEEstimator: block_expansion, num_kp, image_channel and num_bins are positive ints")
        if image_channel != 3:
            raise ValueError(f"HEEstimator: image_channel {image_channel} is not implemented: the native network takes three colour channels")
        self.structure = (int(image_channel), int(block_expansion), int(num_bins), int(num_kp))
        self.conv1 = nn.Conv2d(image_channel, block_expansion, 7, padding=3, stride=2)
        self.norm1 = nn.BatchNorm2d(block_expansion, affine=True)
        self.conv2 = nn.Conv2d(block_expansion, 256, 1)
        self.norm2 = nn.BatchNorm2d(256, affine=True)
        self.block1 = nn.Sequential()
        for i in range(3):
            self.block1.add_module(f"b1_{i}", _ResBottleneck(256, 1))
        for (conv, norm, c), strided, (group, letter, n) in _HE_STAGES:
            setattr(self, conv, nn.Conv2d(c // 2, c, 1))
            setattr(self, norm, nn.BatchNorm2d(c, affine=True))
            setattr(self, strided, _ResBottleneck(c, 2))
            seq = nn.Sequential()
            for i in range(n):
                seq.add_module(f"{letter}{i}", _ResBottleneck(c, 1))
            setattr(self, group, seq)
        self.fc_roll = nn.Linear(2048, num_bins)
        self.fc_pitch = nn.Linear(2048, num_bins)
        self.fc_yaw = nn.Linear(2048, num_bins)
        self.fc_t = nn.Linear(2048, 3)
        self.fc_exp = nn.Linear(2048, 3 * num_kp)
        self.requires_grad_(False)
        self._loaded = False

    def forward(self, x):
        if self.training:
            raise NotImplementedError("HEEstimator: training mode is not implemented; call .eval()")
        with torch.no_grad():
            out = F.max_pool2d(F.relu(self.norm1(self.conv1(x))), 3, 2, 1)
            out = self.block1(F.relu(self.norm2(self.conv2(out))))
            for (conv, norm, _), strided, (group, _, _) in _HE_STAGES:
                out = getattr(self, group)(getattr(self, strided)(F.relu(getattr(self, norm)(getattr(self, conv)(out)))))
            out = F.adaptive_avg_pool2d(out, 1).view(out.shape[0], -1)
            return {"yaw": self.fc_roll(out), "pitch": self.fc_pitch(out), "roll": self.fc_yaw(out), "t": self.fc_t(out), "exp": self.fc_exp(out)}


# ------------------------------------------------------------------------------------------------ weights: keys, shapes, validation
def kp_detector_structure_shapes(structure):
    """``{key: shape}`` of the ``KPDetector`` with ``structure`` (``kp_detector_structure``), in ``state_dict`` order."""
    cin, down, depth, up, K, jmaps, k, _ = structure
    out = {}
    for i, c in enumerate(down):
        p = f"predictor.down_blocks.down{i}"
        out[p + ".conv.weight"], out[p + ".conv.bias"] = (c, cin if i == 0 else down[i - 1], 3, 3), (c,)
        bn_shapes(out, p + ".norm", c)
    out["predictor.conv.weight"], out["predictor.conv.bias"] = (depth * down[-1], down[-1], 1, 1), (depth * down[-1],)
    for i, c in enumerate(up):
        p = f"predictor.up_blocks.up{i}"
        out[p + ".conv.weight"], out[p + ".conv.bias"] = (c, down[-1] if i == 0 else up[i - 1], 3, 3, 3), (c,)
        bn_shapes(out, p + ".norm", c)
    out["kp.weight"], out["kp.bias"] = (K, up[-1], 3, 3, 3), (K,)
    if jmaps:
        out["jacobian.weight"], out["jacobian.bias"] = (9 * jmaps, up[-1], 3, 3, 3), (9 * jmaps,)
    if k:
        out["down.weight"] = (cin, 1, k, k)
    return out


def he_estimator_structure_shapes(structure):
    """``{key: shape}`` of the ``HEEstimator`` with ``structure`` = (image_channel, block_expansion, num_bins, num_kp), in ``state_dict`` order."""
    cin, be, nbins, K = structure
    out = {}

    def conv(p, co, ci, k):
        out[p + ".weight"], out[p + ".bias"] = (co, ci, k, k), (co,)

    def bottleneck(p, c, strided):
        conv(p + ".conv1", c // 4, c, 1), conv(p + ".conv2", c // 4, c // 4, 3), conv(p + ".conv3", c, c // 4, 1)
        bn_shapes(out, p + ".norm1", c // 4), bn_shapes(out, p + ".norm2", c // 4), bn_shapes(out, p + ".norm3", c)
        if strided:
            conv(p + ".skip", c, c, 1), bn_shapes(out, p + ".norm4", c)

    conv("conv1", be, cin, 7), bn_shapes(out, "norm1", be)
    conv("conv2", 256, be, 1), bn_shapes(out, "norm2", 256)
    for i in range(3):
        bottleneck(f"block1.b1_{i}", 256, False)
    for (cv, norm, c), strided, (group, letter, n) in _HE_STAGES:
        conv(cv, c, c // 2, 1), bn_shapes(out, norm, c)
        bottleneck(strided, c, True)
        for i in range(n):
            bottleneck(f"{group}.{letter}{i}", c, False)
    for name, n in zip(_HE_HEADS, (nbins, nbins, nbins, 3, 3 * K)):
        out[name + ".weight"], out[name + ".bias"] = (n, 2048), (n,)
    return out


def kp_detector_state_dict_shapes(**config):
    """``{key: shape}`` of ``KPDetector(**config).state_dict()``, in its order (the upstream configuration by default)."""
    config.pop("feature_channel", None), config.pop("temperature", None)
    return kp_detector_structure_shapes(kp_detector_structure(**config))


def he_estimator_state_dict_shapes(block_expansion=64, num_kp=15, image_channel=3, num_bins=66):
    """``{key: shape}`` of ``HEEstimator(...).state_dict()``, in its order."""
    return he_estimator_structure_shapes((image_channel, block_expansion, num_bins, num_kp))


def _shape_of(name, sd, key, ndim, cls):
    t = sd.get(key)
    if not isinstance(t, torch.Tensor) or t.dim() != ndim:
        raise KeyError(f"{name}: the weights lack '{key}': expected the keys of {cls}")
    return tuple(int(d) for d in t.shape)


def _kp_structure_of_keys(name, sd):
    """The structure read off the keys and shapes of a mapping (a ``KPDetector`` module hands over its own)."""
    down, i = [], 0
    cin = _shape_of(name, sd, "predictor.down_blocks.down0.conv.weight", 4, "KPDetector")[1]
    while f"predictor.down_blocks.down{i}.conv.weight" in sd:
        down.append(_shape_of(name, sd, f"predictor.down_blocks.down{i}.conv.weight", 4, "KPDetector")[0])
        i += 1
    depth = _shape_of(name, sd, "predictor.conv.weight", 4, "KPDetector")[0] // down[-1]
    up, i = [], 0
    while f"predictor.up_blocks.up{i}.conv.weight" in sd:
        up.append(_shape_of(name, sd, f"predictor.up_blocks.up{i}.conv.weight", 5, "KPDetector")[0])
        i += 1
    K = _shape_of(name, sd, "kp.weight", 5, "KPDetector")[0]
    jmaps = _shape_of(name, sd, "jacobian.weight", 5, "KPDetector")[0] // 9 if "jacobian.weight" in sd else 0
    k = _shape_of(name, sd, "down.weight", 4, "KPDetector")[2] if "down.weight" in sd else 0
    s = (k + 3) // 4 if k else 1                                      # k = 2 round(2 (s - 1)) + 1 = 4 s - 3 for an integer s
    if min(depth, len(up)) < 1 or (k and (k != 4 * s - 3)) or (jmaps and jmaps != K):
        raise ValueError(f"{name}: the weights are not a KPDetector the native path implements (depth {depth}, {len(up)} up blocks, anti-alias kernel {k}, "
                         f"{jmaps} Jacobian maps for {K} keypoints)")
    return cin, tuple(down), depth, tuple(up), K, jmaps, k, s


def _he_structure_of_keys(name, sd):
    be, cin = _shape_of(name, sd, "conv1.weight", 4, "HEEstimator")[:2]
    return cin, be, _shape_of(name, sd, "fc_roll.weight", 2, "HEEstimator")[0], _shape_of(name, sd, "fc_exp.weight", 2, "HEEstimator")[0] // 3


_KP_NET = _Net("KPDetector", kp_detector_structure_shapes, ("module.", "kp_detector."), True, ("predictor.conv.weight",), _kp_structure_of_keys, EVAL_ONLY,
               ("num_batches_tracked",))
_HE_NET = _Net("HEEstimator", he_estimator_structure_shapes, ("module.", "he_estimator."), True, ("conv1.weight",), _he_structure_of_keys, EVAL_ONLY,
               ("num_batches_tracked",))


def _net_of(weights, base):
    """The description ``_validated`` checks ``weights`` against (``base``: ``_KP_NET`` or ``_HE_NET``): a mirror module is held to the structure it was built
    with, anything else to the structure its keys and shapes spell."""
    return module_net(base, weights.structure) if isinstance(weights, KPDetector if base is _KP_NET else HEEstimator) else base


def _slabs3d(cout, cin, device):
    return tuple(torch.empty(((cin + 15) // 16, 27, 2, cout, 8), dtype=torch.int16, device=device) for _ in range(3))


def prep_conv3d(w, scale=None, shift=None):
    """(three-way split slabs of the Conv3d weight ``w [cout, cin, 3, 3, 3]`` times ``scale[co]``, the shift as fp32 bias or None) for ``conv3d_sb3``."""
    cout, cin = w.shape[:2]
    if tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError(f"prep_conv3d: expected a [cout, cin, 3, 3, 3] weight, got {tuple(w.shape)}")
    if scale is not None:
        w = (w.double() * scale[:, None, None, None, None]).float()
    w = _c(w, "weight")
    s3 = _slabs3d(cout, cin, w.device)
    lib().call("e4s_conv3d_prep_weights_sb3", _p(s3[0]), _p(s3[1]), _p(s3[2]), None, _p(w), None, None, None, None, 0.0, None, cout, cin, _stream())
    return s3, (shift.float().contiguous() if shift is not None else None)


def _batch_slice(t):
    """Whether ``t`` is a tensor the strided kernels take in place: every sample dense (a channel slice ``buf[:, a:b]`` of a dense buffer is)."""
    return t.dim() >= 2 and (t.shape[0] == 0 or t[0].is_contiguous())


def conv3d_sb3(x, slabs, bias=None, *, relu: bool = False, residual=None, up_hw: int = 1, out=None):
    """``act(conv3d(up(x), W, stride 1, zero pad 1) + bias + residual)`` of csrc/conv3d.hip on prepared ``slabs`` (``prep_conv3d``): ``x [bs, cin, D, h, w]``
    float32, ``up`` the nearest (1, ``up_hw``, ``up_hw``) upsampling folded into the gather; returns ``[bs, cout, D, up_hw h, up_hw w]``.  A channel slice of a
    dense buffer is read in place, and ``out``, a tensor or such a slice of the output's shape, is written in place (``e4s_conv3d_sb3_strided``): a
    concatenation along the channels is never copied."""
    x = _req(x, "x") if isinstance(x, torch.Tensor) and _batch_slice(x) else _c(x, "x")
    if x.dim() != 5 or up_hw not in (1, 2) or x.shape[1] > 16 * slabs[0].shape[0] or x.shape[1] <= 16 * (slabs[0].shape[0] - 1):
        raise ValueError(f"conv3d_sb3: x is {tuple(x.shape)} with up_hw {up_hw}: expected [bs, cin, D, h, w] matching the slabs and up_hw 1 or 2")
    bs, cin, D, h, w = x.shape
    cout = slabs[0].shape[3]
    shape = (bs, cout, D, up_hw * h, up_hw * w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(_req(out, "out").shape) != shape or not _batch_slice(out):
        raise ValueError(f"conv3d_sb3: out is {tuple(out.shape)}, strides {out.stride()}: expected {shape} with every sample dense")
    if residual is not None:
        residual = _c(residual, "residual")
        if residual.shape != out.shape:
            raise ValueError(f"conv3d_sb3: residual shape {tuple(residual.shape)} != output {tuple(out.shape)}")
    if x.is_contiguous() and out.is_contiguous():
        lib().call("e4s_conv3d_sb3", _p(out), _p(x), *[_p(s) for s in slabs], _p(bias), _p(residual), 1 if relu else 0, up_hw, bs, cin, cout, D, up_hw * h,
                   up_hw * w, _stream())
    else:
        lib().call("e4s_conv3d_sb3_strided", _p(out), _p(x), *[_p(s) for s in slabs], _p(bias), _p(residual), 1 if relu else 0, up_hw, bs, cin, cout, D,
                   up_hw * h, up_hw * w, _bstride(x), _bstride(out), cout * D * up_hw * h * up_hw * w, _stream())
    return out


def _bstride(t):
    """The element stride between the samples of ``t`` (a batch of one has none to speak of: its own size)."""
    return int(t.stride(0)) if t.shape[0] > 1 else int(t[0].numel())


def _conv_any(x, prepared, k, stride=1, relu=False, residual=None):
    """A 2-D convolution on whichever kernel its weights were prepared for: the exact one (a K-major tensor: fewer than 16 input channels) or sb3 (slabs)."""
    w, bias = prepared
    conv = conv_sb if isinstance(w, tuple) else conv_exact
    return conv(x, w, bias, k=k, stride=stride, relu=relu, residual=residual)


def _prep2d(sd, conv, norm=None):
    w = sd[conv + ".weight"]
    scale, shift = fold_conv_bn(sd, conv, norm) if norm is not None else (torch.ones(w.shape[0], dtype=torch.float64, device=w.device), sd[conv + ".bias"].double())
    return (prep_exact if w.shape[1] < 16 else prep_fwd)(w, scale, shift)


class PreparedKPDetector(PreparedNet):
    """The kernels' copies of a ``KPDetector``'s weights, rebuilt when a tensor changes version or storage: per DownBlock2d the convolution with its bias and
    BatchNorm folded in float64 (K-major fp32 under 16 input channels, three-way split slabs otherwise), the 1 x 1 convolution's slabs, per UpBlock3d and for
    the heads the 27-tap slabs, and the anti-alias kernel."""

    __slots__ = ()
    _entry = "kp_detector_forward"

    def _net(self, weights):
        return _net_of(weights, _KP_NET)

    def _build(self, sd, structure, dev):
        _, down, _, up, _, jmaps, k, _ = structure
        return dict(down=[_prep2d(sd, f"predictor.down_blocks.down{i}.conv", f"predictor.down_blocks.down{i}.norm") for i in range(len(down))],
                    conv=_prep2d(sd, "predictor.conv"),
                    up=[prep_conv3d(sd[f"predictor.up_blocks.up{i}.conv.weight"], *fold_conv_bn(sd, f"predictor.up_blocks.up{i}.conv", f"predictor.up_blocks.up{i}.norm"))
                        for i in range(len(up))],
                    kp=prep_conv3d(sd["kp.weight"], None, sd["kp.bias"].double()),
                    jac=prep_conv3d(sd["jacobian.weight"], None, sd["jacobian.bias"].double()) if jmaps else None,
                    taps=sd["down.weight"][0, 0].contiguous() if k else None)


class PreparedHEEstimator(PreparedNet):
    """The kernels' copies of an ``HEEstimator``'s weights: ``conv1`` K-major fp32 with ``norm1`` folded, every other convolution as three-way split slabs with
    its bias and BatchNorm folded in float64, and the five heads as one ``[3 num_bins + 3 + 3 num_kp, 2048]`` matrix in key order with its bias."""

    __slots__ = ()
    _entry = "he_estimator_forward"

    def _net(self, weights):
        return _net_of(weights, _HE_NET)

    def _build(self, sd, structure, dev):
        def bottleneck(p, strided):
            return dict(c1=_prep2d(sd, p + ".conv1", p + ".norm1"), c2=_prep2d(sd, p + ".conv2", p + ".norm2"), c3=_prep2d(sd, p + ".conv3", p + ".norm3"),
                        skip=_prep2d(sd, p + ".skip", p + ".norm4") if strided else None)

        stages = [dict(widen=_prep2d(sd, "conv2", "norm2"), blocks=[bottleneck(f"block1.b1_{i}", False) for i in range(3)])]
        for (cv, norm, _), strided, (group, letter, n) in _HE_STAGES:
            stages.append(dict(widen=_prep2d(sd, cv, norm), blocks=[bottleneck(strided, True)] + [bottleneck(f"{group}.{letter}{i}", False) for i in range(n)]))
        n = sum(sd[h + ".bias"].shape[0] for h in _HE_HEADS)
        return dict(stem=prep_exact(sd["conv1.weight"], *fold_conv_bn(sd, "conv1", "norm1")), stages=stages,
                    fc_w=torch.cat([sd[h + ".weight"] for h in _HE_HEADS]).contiguous(), fc_b=torch.cat([sd[h + ".bias"] for h in _HE_HEADS]).contiguous(),
                    ones=torch.ones(n, dtype=torch.float32, device=dev), zeros=torch.zeros(n, dtype=torch.float32, device=dev))


# ------------------------------------------------------------------------------------------------ the forward passes
def _checked_image(name, x, weights, base):
    """Everything that can be refused, before any launch; returns the checked weights."""
    check_loaded(name, weights, "the weights")
    checked = _validated(name, weights, _net_of(weights, base))
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    if x.shape[1] != 3:
        raise ValueError(f"{name}: x is {tuple(x.shape)}: expected three colour channels")
    if min(x.shape[2:]) < 1 or max(x.shape[2:]) > 16384:
        raise ValueError(f"{name}: x is {tuple(x.shape)}: sides of 1 .. 16384")
    return checked


def heatmap_keypoints(logits, jac_planes=None, temperature=0.1, want_heatmap=False):
    """``e4s_v2v_heatmap_kp``: the softmax of ``logits [bs, K, D, H, W] / temperature`` over each volume and its expectation on the (x, y, z) grid in [-1, 1]:
    ``value [bs, K, 3]``; with ``jac_planes [bs, 9 K, D, H, W]`` also ``jacobian [bs, K, 3, 3]``; the normalised ``heatmap`` when wanted.  Returns the three
    (None where not asked for)."""
    logits = _c(logits, "logits")
    if logits.dim() != 5 or min(logits.shape[2:]) < 2:
        raise ValueError(f"heatmap_keypoints: logits are {tuple(logits.shape)}: expected [bs, K, D, H, W] with every extent of the volume at least 2")
    bs, K, D, H, W = logits.shape
    if jac_planes is not None:
        jac_planes = _c(jac_planes, "jac_planes")
        if tuple(jac_planes.shape) != (bs, 9 * K, D, H, W):
            raise ValueError(f"heatmap_keypoints: jac_planes are {tuple(jac_planes.shape)}, expected {(bs, 9 * K, D, H, W)}")
    value = torch.empty((bs, K, 3), dtype=torch.float32, device=logits.device)
    jac = torch.empty((bs, K, 3, 3), dtype=torch.float32, device=logits.device) if jac_planes is not None else None
    heat = torch.empty_like(logits) if want_heatmap else None
    lib().call("e4s_v2v_heatmap_kp", _p(value), _p(jac), _p(heat), _p(logits), _p(jac_planes), float(temperature), bs, K, D, H, W, _stream())
    return value, jac, heat


def antialias_down(x, taps, stride: int):
    """``AntiAliasInterpolation2d.forward`` on ``x [bs, C, H, W]`` with the ``k x k`` kernel ``taps``: only the kept outputs are evaluated."""
    x, taps = _c(x, "x"), _c(taps, "taps")
    bs, c, h, w = x.shape
    out = torch.empty((bs, c, -(-h // stride), -(-w // stride)), dtype=torch.float32, device=x.device)
    lib().call("e4s_v2v_antialias_down", _p(out), _p(x), _p(taps), bs * c, h, w, taps.shape[0], int(stride), _stream())
    return out


def avgpool2x2(x, out=None):
    """``nn.AvgPool2d(2)`` on ``[bs, C, H, W]`` (an odd last row or column is dropped).  ``out``: a ``[bs, C, H // 2, W // 2]`` tensor or channel slice of a
    dense buffer to write into (``e4s_avgpool2x2_strided``)."""
    x = _c(x, "x")
    bs, c, h, w = x.shape
    if min(h, w) < 2:
        raise ValueError(f"avgpool2x2: x is {tuple(x.shape)}: the planes must be at least 2 x 2")
    if out is None:
        out = torch.empty((bs, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
        lib().call("e4s_avgpool2x2", _p(out), _p(x), bs * c, h, w, _stream())
        return out
    if tuple(_req(out, "out").shape) != (bs, c, h // 2, w // 2) or not _batch_slice(out):
        raise ValueError(f"avgpool2x2: out is {tuple(out.shape)}, strides {out.stride()}: expected {(bs, c, h // 2, w // 2)} with every sample dense")
    lib().call("e4s_avgpool2x2_strided", _p(out), _p(x), bs, c, h, w, _bstride(out), _stream())
    return out


def kp_detector_forward(x: torch.Tensor, weights, temperature=None, want_heatmap: bool = False):
    """``KPDetector.forward(x)`` (keypoint_detector.py:56-82) in eval mode on the device: ``{'value' [bs, num_kp, 3][, 'jacobian' [bs, num_kp, 3, 3]]}`` from a
    float32 ``x [bs, 3, H, W]``; with ``want_heatmap`` also ``'prediction'`` (the logits) and ``'heatmap'``.  ``weights``: a module with the network's keys
    (``KPDetector``, the drop-in) or the mapping ``torch.load`` returns (``checkpoint['kp_detector']`` or the checkpoint itself); a mapping's structure is read off
    its keys and shapes, and its ``temperature`` — which no key holds — is the argument (default: the module's, 0.1 for a mapping).  A module's prepared weights
    are cached per parameter version.  Refused before any launch: a CPU tensor, another dtype, other than three channels, a module in training mode or never
    loaded, an input that leaves an extent of the final volume below 2."""
    name = "kp_detector_forward"
    checked = _checked_image(name, x, weights, _KP_NET)
    structure = checked[1]
    if temperature is None:
        temperature = getattr(weights, "temperature", 0.1)
    if not float(temperature) > 0:
        raise ValueError(f"{name}: temperature {temperature!r} must be positive")
    D, H, W = kp_volume_size(structure, int(x.shape[2]), int(x.shape[3]))
    if min(D, H, W) < 2:
        raise ValueError(f"{name}: x is {tuple(x.shape)}: the final volume would be {D} x {H} x {W}, every extent must be at least 2")
    _placed_checked(name, "x", x, checked[2])
    K, jmaps = structure[4], structure[5]
    bs = x.shape[0]
    if bs == 0:
        out = {"value": x.new_empty((0, K, 3))}
        if jmaps:
            out["jacobian"] = x.new_empty((0, K, 3, 3))
        return out
    with torch.no_grad():
        P = prepare(PreparedKPDetector, weights, checked)
        cur = x.detach().contiguous()
        if P["taps"] is not None:
            cur = antialias_down(cur, P["taps"], structure[7])
        for L in P["down"]:
            cur = avgpool2x2(_conv_any(cur, L, 3, relu=True))
        cur = _conv_any(cur, P["conv"], 1)
        cur = cur.view(bs, cur.shape[1] // D, D, cur.shape[2], cur.shape[3])
        for L in P["up"]:
            cur = conv3d_sb3(cur, *L, relu=True, up_hw=2)
        logits = conv3d_sb3(cur, *P["kp"])
        planes = conv3d_sb3(cur, *P["jac"]) if jmaps else None
        value, jac, heat = heatmap_keypoints(logits, planes, temperature, want_heatmap)
    out = {"value": value}
    if jmaps:
        out["jacobian"] = jac
    if want_heatmap:
        out["prediction"], out["heatmap"] = logits, heat
    return out


def he_estimator_forward(x: torch.Tensor, weights):
    """``HEEstimator.forward(x)`` (keypoint_detector.py:136-178) in eval mode on the device: ``{'yaw', 'pitch', 'roll' [bs, num_bins], 't' [bs, 3], 'exp' [bs, 3
    num_kp]}`` from a float32 ``x [bs, 3, H, W]``, the head names crossed as the reference crosses them (``yaw`` comes from ``fc_roll``, ``roll`` from
    ``fc_yaw``).  The five outputs are views of one ``[bs, 3 num_bins + 3 + 3 num_kp]`` tensor.  ``weights`` and the refusals: see ``kp_detector_forward``."""
    name = "he_estimator_forward"
    checked = _checked_image(name, x, weights, _HE_NET)
    _, _, nbins, K = checked[1]
    _placed_checked(name, "x", x, checked[2])
    bs, _, H, W = x.shape
    n = 3 * nbins + 3 + 3 * K
    y = torch.empty((bs, n), dtype=torch.float32, device=x.device)
    if bs:
        with torch.no_grad():
            P = prepare(PreparedHEEstimator, weights, checked)
            cur = _conv_any(x.detach().contiguous(), P["stem"], 7, stride=2, relu=True)
            pooled = torch.empty((bs, cur.shape[1], (cur.shape[2] - 1) // 2 + 1, (cur.shape[3] - 1) // 2 + 1), dtype=torch.float32, device=x.device)
            lib().call("e4s_maxpool3x3s2", _p(pooled), _p(cur), bs * cur.shape[1], cur.shape[2], cur.shape[3], _stream())
            cur = pooled
            for S in P["stages"]:
                cur = _conv_any(cur, S["widen"], 1, relu=True)
                for L in S["blocks"]:
                    stride = 2 if L["skip"] is not None else 1
                    o = _conv_any(cur, L["c1"], 1, relu=True)
                    o = _conv_any(o, L["c2"], 3, stride=stride, relu=True)
                    idn = _conv_any(cur, L["skip"], 1, stride=stride) if L["skip"] is not None else cur
                    cur = _conv_any(o, L["c3"], 1, relu=True, residual=idn)
            feat = torch.empty((bs, cur.shape[1]), dtype=torch.float32, device=x.device)
            lib().call("e4s_plane_stats", _p(feat), None, None, _p(cur), bs * cur.shape[1], cur.shape[2] * cur.shape[3], 0.0, _stream())
            # the bias rides on e4s_vec_fc's BatchNorm slot: (a - 0) * (1 / sqrt(1 + 0)) + bias
            lib().call("e4s_vec_fc", _p(y), _p(feat), _p(P["fc_w"]), _p(P["ones"]), _p(P["fc_b"]), _p(P["zeros"]), _p(P["ones"]), 0.0, 0, bs, cur.shape[1], n,
                       _stream())
    roll_head, pitch_head, yaw_head, t, exp = torch.split(y, (nbins, nbins, nbins, 3, 3 * K), dim=1)
    return {"yaw": roll_head, "pitch": pitch_head, "roll": yaw_head, "t": t, "exp": exp}


# ------------------------------------------------------------------------------------------------ keypoint_transformation
def _angles(name, he, yaw, pitch, roll, free_view):
    """(the three logit rows or None, deg_in [bs, 3] or None) of drive_demo.py:137-157: without ``free_view`` the logits; with it a fixed angle where one is
    given (a number, for every sample) and the logits' degrees where it is None."""
    rows = [he["yaw"], he["pitch"], he["roll"]]
    for nm, r in zip(("yaw", "pitch", "roll"), rows):
        _tensor_checked(name, f"he['{nm}']", r, torch.float32, 2, "float32 [bs, 66] logits")
        if r.shape != rows[0].shape or r.shape[1] != NUM_BINS:
            raise ValueError(f"{name}: he['{nm}'] is {tuple(r.shape)}: expected [bs, {NUM_BINS}] (headpose_pred_to_degree weighs 66 bins)")
    if not free_view:
        return rows, None
    fixed = (yaw, pitch, roll)
    return [None if f is not None else r for f, r in zip(fixed, rows)], fixed


def _transform(name, kp_canonical, he, estimate_jacobian, free_view, yaw, pitch, roll):
    if not hasattr(kp_canonical, "keys") or "value" not in kp_canonical or not hasattr(he, "keys"):
        raise TypeError(f"{name}: kp_canonical is KPDetector's output dict and he HEEstimator's")
    kp, t, exp = kp_canonical["value"], he["t"], he["exp"]
    _tensor_checked(name, "kp_canonical['value']", kp, torch.float32, 3, "float32 [bs, num_kp, 3]")
    rows, fixed = _angles(name, he, yaw, pitch, roll, free_view)
    bs, K = he["yaw"].shape[0], kp.shape[1]
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != bs * 3 or t.dim() not in (2, 3):
        raise ValueError(f"{name}: he['t'] is {tuple(getattr(t, 'shape', ()))}: expected float32 [bs, 3] (or the [bs, 1, 3] the reference leaves behind)")
    _tensor_checked(name, "he['exp']", exp, torch.float32, 2, "float32 [bs, 3 num_kp]")
    if kp.shape[2] != 3 or kp.shape[0] not in (bs, 1) or tuple(exp.shape) != (bs, 3 * K):
        raise ValueError(f"{name}: kp_canonical['value'] is {tuple(kp.shape)} and he['exp'] {tuple(exp.shape)} for a batch of {bs}: expected [bs or 1, K, 3] and [bs, 3 K]")
    jac = None
    if estimate_jacobian:
        jac = kp_canonical.get("jacobian")
        _tensor_checked(name, "kp_canonical['jacobian']", jac, torch.float32, 4, "float32 [bs, num_kp, 3, 3]")
        if tuple(jac.shape) != (kp.shape[0], K, 3, 3):
            raise ValueError(f"{name}: kp_canonical['jacobian'] is {tuple(jac.shape)}, expected {(kp.shape[0], K, 3, 3)}")
    ts = {"kp_canonical['value']": kp, "he['yaw']": he["yaw"], "he['pitch']": he["pitch"], "he['roll']": he["roll"], "he['t']": t, "he['exp']": exp}
    if jac is not None:
        ts["kp_canonical['jacobian']"] = jac
    for nm, v in ts.items():
        if not v.is_cuda:
            raise RuntimeError(f"{name}: {nm} must be a CUDA tensor")
    dev = kp.device
    if any(v.device != dev for v in ts.values()):
        raise RuntimeError(f"{name}: device mismatch among the tensors")
    deg_in = None
    if fixed is not None:
        deg_in = torch.tensor([[0.0 if f is None else float(f) for f in fixed]] * max(bs, 1), dtype=torch.float32).to(dev)[:bs].contiguous()
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)      # noqa: E731
    value, jout, deg, rot = new(bs, K, 3), (new(bs, K, 3, 3) if jac is not None else None), new(bs, 3), new(bs, 3, 3)
    with torch.no_grad():
        # contiguous copies (the heads are column slices of one tensor) stay alive in these names until the launch is queued
        rows_c = [None if r is None else r.detach().contiguous() for r in rows]
        t_c, exp_c, kp_c = t.detach().contiguous(), exp.detach().contiguous(), kp.detach().contiguous()
        jac_c = None if jac is None else jac.detach().contiguous()
        lib().call("e4s_v2v_kp_transform", _p(value), _p(jout), _p(deg), _p(rot), *[_p(r) for r in rows_c], _p(deg_in), _p(t_c), _p(exp_c), _p(kp_c), _p(jac_c),
                   bs, kp.shape[0], K, NUM_BINS, _stream())
    return value, jout, deg, rot


def keypoint_transformation(kp_canonical, he, estimate_jacobian=True, free_view=False, yaw=0, pitch=0, roll=0):
    """``keypoint_transformation`` of drive_demo.py:135-180 on the device in one launch: ``{'value': rot kp + t + exp, 'jacobian': rot jacobian or None}`` with
    ``rot = pitch_mat yaw_mat roll_mat`` from the degrees of the three logit rows (radians through 3.14).  ``kp_canonical['value']`` may hold one sample for every
    frame of ``he``.  With ``free_view`` an angle that is a number replaces that row's degrees for every sample, ``None`` keeps the row's.  Unlike the reference,
    ``he['t']`` is not reshaped in place: the caller's dict is left as it was (a ``[bs, 1, 3]`` tensor the reference left behind is accepted)."""
    value, jac, _, _ = _transform("keypoint_transformation", kp_canonical, he, estimate_jacobian, free_view, yaw, pitch, roll)
    return {"value": value, "jacobian": jac}


def headpose_degrees(he):
    """``headpose_pred_to_degree`` of the three rows of ``he``: float32 ``[bs, 3]`` of (yaw, pitch, roll) degrees, ``sum(softmax(row) idx) 3 - 99``."""
    return _pose("headpose_degrees", he)[0]


def rotation_matrix(he):
    """``get_rotation_matrix`` of those degrees: float32 ``[bs, 3, 3]``."""
    return _pose("rotation_matrix", he)[1]


def _pose(name, he):
    if not hasattr(he, "keys"):
        raise TypeError(f"{name}: he is HEEstimator's output dict")
    bs = he["yaw"].shape[0] if isinstance(he["yaw"], torch.Tensor) and he["yaw"].dim() == 2 else 0
    dev = he["yaw"].device if isinstance(he["yaw"], torch.Tensor) else "cpu"
    zero = {"value": torch.zeros((1, 1, 3), dtype=torch.float32, device=dev)}
    stub = dict(he, t=torch.zeros((bs, 3), dtype=torch.float32, device=dev), exp=torch.zeros((bs, 3), dtype=torch.float32, device=dev))
    _, _, deg, rot = _transform(name, zero, stub, False, False, 0, 0, 0)
    return deg, rot


# ------------------------------------------------------------------------------------------------ the clip-level function
def reenact_keypoints(source, driving, kp_detector, he_estimator, estimate_jacobian=None):
    """What ``make_animation`` (drive_demo.py:182-) computes in front of the generator: ``kp_canonical = kp_detector(source)``, once per clip, and the transformed
    keypoints of the source and of every driving frame.  ``source [1, 3, H, W]`` and ``driving [n, 3, H, W]`` are float32 in [0, 1] on the device.  ONE
    ``HEEstimator`` pass runs over the n + 1 images.  Returns ``(kp_canonical, kp_source, kp_driving)``, ``kp_driving`` batched over the n frames.
    ``estimate_jacobian``: default, whether the detector has a Jacobian head."""
    name = "reenact_keypoints"
    for nm, t in (("source", source), ("driving", driving)):
        _tensor_checked(name, nm, t, torch.float32, 4, "a float32 [n, 3, H, W] image batch")
    if source.shape[0] != 1 or driving.shape[1:] != source.shape[1:]:
        raise ValueError(f"{name}: source is {tuple(source.shape)} and driving {tuple(driving.shape)}: expected [1, 3, H, W] and [n, 3, H, W] of one size")
    _cuda_checked(name, source=source, driving=driving)
    kp_canonical = kp_detector_forward(source, kp_detector)
    if estimate_jacobian is None:
        estimate_jacobian = "jacobian" in kp_canonical
    he = he_estimator_forward(torch.cat((source, driving)), he_estimator)
    part = lambda a, b: {k: v[a:b] for k, v in he.items()}      # noqa: E731
    kp_source = keypoint_transformation(kp_canonical, part(0, 1), estimate_jacobian)
    kp_driving = keypoint_transformation(kp_canonical, part(1, None), estimate_jacobian)
    return kp_canonical, kp_source, kp_driving


# ================================================================================================ row f18: stage 2, the dense-motion network
# ``DenseMotionNetwork`` of swap_face_fine/face_vid2vid/modules/dense_motion.py:9-128 with ``Hourglass`` / ``Encoder`` / ``Decoder`` / ``DownBlock3d`` /
# ``UpBlock3d``, ``kp2gaussian`` and ``make_coordinate_grid`` of modules/util.py, in eval mode:
#
#     compress       1 x 1 x 1 + BatchNorm + ReLU as a 1 x 1 on [bs, C, D H, W] (e4s_conv2d_sb3; the exact e4s_conv2d under 16 channels)
#     input          e4s_v2v_motion_input: heatmaps and deformed features of the K + 1 motions in one pass, written where the last skip is read
#     hourglass      e4s_conv3d_sb3(_strided) with BatchNorm folded in float64 and ReLU fused; every torch.cat([out, skip], dim=1) of the decoder is one buffer:
#                    UpBlock3d (up_hw = 2) writes its first channels, e4s_avgpool2x2_strided pools the encoder's output into its last
#     mask           e4s_conv3d_k7_sb3 (7 x 7 x 7), then e4s_v2v_motion_combine: softmax over the K + 1 channels and the deformation
#     occlusion      e4s_conv3d_k7_sb3 with kd 1 on prediction.view(bs, C D, H, W), sigmoid in the epilogue
#
# The reference builds the sampling grid with the align_corners=True formula and samples with F.grid_sample's default (False): kept as it is.
def dense_motion_structure(block_expansion=32, num_blocks=5, max_features=1024, num_kp=15, feature_channel=32, reshape_depth=16, compress=4,
                           estimate_occlusion_map=True):
    """The constructor arithmetic of ``DenseMotionNetwork`` / ``Hourglass`` as ``(num_kp, feature_channel, compress, encoder widths, decoder widths, depth of
    the occlusion head or 0)``; refuses what the native path does not implement."""
    if not all(_is_int(v) for v in (block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress)):
        raise ValueError("DenseMotionNetwork: block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth and compress are ints")
    if min(block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress) < 1:
        raise ValueError("DenseMotionNetwork: widths, depths and counts are positive")
    if num_kp + 1 > 32:
        raise ValueError(f"DenseMotionNetwork: num_kp {num_kp} is not implemented: the mask head has num_kp + 1 outputs and the native kernel takes at most 32")
    if block_expansion > max_features:
        raise ValueError(f"DenseMotionNetwork: block_expansion {block_expansion} above max_features {max_features}: the reference's own decoder does not fit")
    width = lambda i: min(max_features, block_expansion * 2 ** i)      # noqa: E731
    down = tuple(width(i + 1) for i in range(num_blocks))
    up = tuple(width(num_blocks - i - 1) for i in range(num_blocks))
    return int(num_kp), int(feature_channel), int(compress), down, up, int(reshape_depth) if estimate_occlusion_map else 0


def _dm_widths(structure):
    """(hourglass input channels, its output channels, the encoder's output channels per level, level 0 the input)."""
    K, _, c, down, up, _ = structure
    infe = (K + 1) * (c + 1)
    return infe, up[-1] + infe, (infe,) + tuple(down)


class _DownBlock3d(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 3, padding=1)
        self.norm = nn.BatchNorm3d(cout, affine=True)

    def forward(self, x):
        return F.avg_pool3d(F.relu(self.norm(self.conv(x))), (1, 2, 2))


class _Encoder3d(nn.Module):
    def __init__(self, levels):
        super().__init__()
        self.down_blocks = nn.ModuleList([_DownBlock3d(levels[i], levels[i + 1]) for i in range(len(levels) - 1)])

    def forward(self, x):
        outs = [x]
        for block in self.down_blocks:
            outs.append(block(outs[-1]))
        return outs


class _Decoder3d(nn.Module):
    def __init__(self, levels, up, out_filters):
        super().__init__()
        nb = len(up)
        self.up_blocks = nn.ModuleList([_UpBlock3d(levels[nb] if j == 0 else up[j - 1] + levels[nb - j], up[j]) for j in range(nb)])
        self.conv = nn.Conv3d(out_filters, out_filters, 3, padding=1)
        self.norm = nn.BatchNorm3d(out_filters, affine=True)

    def forward(self, outs):
        outs = list(outs)
        out = outs.pop()
        for block in self.up_blocks:
            out = torch.cat([block(out), outs.pop()], dim=1)
        return F.relu(self.norm(self.conv(out)))


class _Hourglass3d(nn.Module):
    def __init__(self, structure):
        super().__init__()
        _, self.out_filters, levels = _dm_widths(structure)
        self.encoder = _Encoder3d(levels)
        self.decoder = _Decoder3d(levels, structure[4], self.out_filters)

    def forward(self, x):
        return self.decoder(self.encoder(x))


def _grid_xyz(d, h, w, like):
    ax = lambda n: 2 * (torch.arange(n, dtype=like.dtype, device=like.device) / (n - 1)) - 1      # noqa: E731
    return torch.stack((ax(w).view(1, 1, w).expand(d, h, w), ax(h).view(1, h, 1).expand(d, h, w), ax(d).view(d, 1, 1).expand(d, h, w)), 3)


def _has_jacobian(kp):
    return "jacobian" in kp and kp["jacobian"] is not None


class DenseMotionNetwork(_Loadable):
    """``DenseMotionNetwork(block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress, estimate_occlusion_map)`` of
    swap_face_fine/face_vid2vid/modules/dense_motion.py with its ``state_dict`` keys, shapes and order; the defaults are the upstream ``vox-256.yaml`` with the
    occlusion head (88 tensors, 43 545 549 parameters; the generator checkpoint's ``dense_motion_network.`` keys load with ``strict=True``).
    ``forward(feature, kp_driving, kp_source)`` is the plain PyTorch composition in eval mode, returning ``{'mask', 'deformation'[, 'occlusion_map']}`` — what
    the tests compare ``dense_motion_forward`` with; ``dense_motion_forward(feature, kp_driving, kp_source, module)`` runs the same weights on the HIP kernels."""
    _PROBE = ("mask.weight", "compress.weight")

    def __init__(self, block_expansion=32, num_blocks=5, max_features=1024, num_kp=15, feature_channel=32, reshape_depth=16, compress=4,
                 estimate_occlusion_map=True):
        super().__init__()
        self.structure = dense_motion_structure(block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress,
                                                estimate_occlusion_map)
        self.hourglass = _Hourglass3d(self.structure)
        self.mask = nn.Conv3d(self.hourglass.out_filters, num_kp + 1, kernel_size=7, padding=3)
        self.compress = nn.Conv3d(feature_channel, compress, kernel_size=1)
        self.norm = nn.BatchNorm3d(compress, affine=True)
        self.occlusion = nn.Conv2d(self.hourglass.out_filters * reshape_depth, 1, kernel_size=7, padding=3) if estimate_occlusion_map else None
        self.num_kp = num_kp
        self.requires_grad_(False)
        self._loaded = False

    def forward(self, feature, kp_driving, kp_source):
        if self.training:
            raise NotImplementedError("DenseMotionNetwork: training mode is not implemented; call .eval()")
        with torch.no_grad():
            bs, _, d, h, w = feature.shape
            K = self.num_kp
            f = F.relu(self.norm(self.compress(feature)))
            grid = _grid_xyz(d, h, w, f)
            kd, ks = kp_driving["value"].view(bs, K, 1, 1, 1, 3), kp_source["value"].view(bs, K, 1, 1, 1, 3)
            motion = grid.view(1, 1, d, h, w, 3) - kd
            if _has_jacobian(kp_driving):
                jac = torch.matmul(kp_source["jacobian"], torch.inverse(kp_driving["jacobian"]))
                motion = torch.matmul(jac.view(bs, K, 1, 1, 1, 3, 3), motion.unsqueeze(-1)).squeeze(-1)
            sparse = torch.cat([grid.view(1, 1, d, h, w, 3).expand(bs, -1, -1, -1, -1, -1), motion + ks], dim=1)
            c = f.shape[1]
            deformed = F.grid_sample(f.unsqueeze(1).expand(-1, K + 1, -1, -1, -1, -1).reshape(bs * (K + 1), c, d, h, w), sparse.reshape(bs * (K + 1), d, h, w, 3),
                                     align_corners=False).view(bs, K + 1, c, d, h, w)
            gauss = lambda kp: torch.exp(-0.5 * ((grid.view(1, 1, d, h, w, 3) - kp) ** 2).sum(-1) / 0.01)      # noqa: E731
            heat = torch.cat([torch.zeros_like(f[:, :1]), gauss(kd) - gauss(ks)], dim=1).unsqueeze(2)
            prediction = self.hourglass(torch.cat([heat, deformed], dim=2).view(bs, -1, d, h, w))
            mask = F.softmax(self.mask(prediction), dim=1)
            out = {"mask": mask, "deformation": (sparse.permute(0, 1, 5, 2, 3, 4) * mask.unsqueeze(2)).sum(dim=1).permute(0, 2, 3, 4, 1)}
            if self.occlusion is not None:
                out["occlusion_map"] = torch.sigmoid(self.occlusion(prediction.reshape(bs, -1, h, w)))
            return out


def dense_motion_structure_shapes(structure):
    """``{key: shape}`` of the ``DenseMotionNetwork`` with ``structure`` (``dense_motion_structure``), in ``state_dict`` order."""
    K, C, c, down, up, occ = structure
    infe, outf, levels = _dm_widths(structure)
    nb = len(down)
    out = {}

    def block(p, co, ci):
        out[p + ".conv.weight"], out[p + ".conv.bias"] = (co, ci, 3, 3, 3), (co,)
        bn_shapes(out, p + ".norm", co)

    for i in range(nb):
        block(f"hourglass.encoder.down_blocks.{i}", levels[i + 1], levels[i])
    for j in range(nb):
        block(f"hourglass.decoder.up_blocks.{j}", up[j], levels[nb] if j == 0 else up[j - 1] + levels[nb - j])
    out["hourglass.decoder.conv.weight"], out["hourglass.decoder.conv.bias"] = (outf, outf, 3, 3, 3), (outf,)
    bn_shapes(out, "hourglass.decoder.norm", outf)
    out["mask.weight"], out["mask.bias"] = (K + 1, outf, 7, 7, 7), (K + 1,)
    out["compress.weight"], out["compress.bias"] = (c, C, 1, 1, 1), (c,)
    bn_shapes(out, "norm", c)
    if occ:
        out["occlusion.weight"], out["occlusion.bias"] = (1, outf * occ, 7, 7), (1,)
    return out


def dense_motion_state_dict_shapes(**config):
    """``{key: shape}`` of ``DenseMotionNetwork(**config).state_dict()``, in its order (the upstream configuration with the occlusion head by default)."""
    return dense_motion_structure_shapes(dense_motion_structure(**config))


def _dm_structure_of_keys(name, sd):
    """The structure read off the keys and shapes of a mapping (a ``DenseMotionNetwork`` module hands over its own)."""
    cls = "DenseMotionNetwork"
    K = _shape_of(name, sd, "mask.weight", 5, cls)[0] - 1
    c, C = _shape_of(name, sd, "compress.weight", 5, cls)[:2]
    down, up, i = [], [], 0
    while f"hourglass.encoder.down_blocks.{i}.conv.weight" in sd:
        down.append(_shape_of(name, sd, f"hourglass.encoder.down_blocks.{i}.conv.weight", 5, cls)[0])
        i += 1
    i = 0
    while f"hourglass.decoder.up_blocks.{i}.conv.weight" in sd:
        up.append(_shape_of(name, sd, f"hourglass.decoder.up_blocks.{i}.conv.weight", 5, cls)[0])
        i += 1
    outf = _shape_of(name, sd, "hourglass.decoder.conv.weight", 5, cls)[0]
    occ = _shape_of(name, sd, "occlusion.weight", 4, cls)[1] // outf if "occlusion.weight" in sd else 0
    if not down or len(down) != len(up) or not 1 <= K <= 31 or outf != up[-1] + (K + 1) * (c + 1):
        raise ValueError(f"{name}: the weights are not a DenseMotionNetwork the native path implements ({len(down)} down and {len(up)} up blocks, num_kp {K}, "
                         f"{outf} hourglass outputs)")
    return K, C, c, tuple(down), tuple(up), occ


_DM_NET = _Net("DenseMotionNetwork", dense_motion_structure_shapes, ("dense_motion_network.", "module.dense_motion_network.", "module."), False,
               ("mask.weight",), _dm_structure_of_keys, EVAL_ONLY, ("num_batches_tracked",))


def _dm_net_of(weights):
    """A mirror module is held to the structure it was built with, anything else to the structure its keys and shapes spell."""
    return module_net(_DM_NET, weights.structure) if isinstance(weights, DenseMotionNetwork) else _DM_NET


def _pool_into(full, dst):
    """DownBlock3d's ``AvgPool3d((1, 2, 2))`` of the dense ``full [bs, C, D, h, w]`` into ``dst [bs, C, D, h // 2, w // 2]``, a tensor or a channel slice."""
    bs, C, D, h, w = full.shape
    lib().call("e4s_avgpool2x2_strided", _p(dst), _p(full), bs, C * D, h, w, _bstride(dst), _stream())


def prep_conv3d_k7(w):
    """The three-way split slabs ``[ceil(cin / 16), 49 kd, 2, cout, 8]`` of a 7-tap weight for ``conv3d_k7``: a Conv3d's ``[cout, cin, 7, 7, 7]`` (kd 7) or
    ``[cout, cin, 1, 7, 7]``, or a Conv2d's ``[cout, cin, 7, 7]`` (kd 1); ``cout`` at most 32."""
    shape = tuple(w.shape)
    if len(shape) == 4:
        shape = shape[:2] + (1,) + shape[2:]
    if len(shape) != 5 or shape[2] not in (1, 7) or shape[3:] != (7, 7) or not 1 <= shape[0] <= 32:
        raise ValueError(f"prep_conv3d_k7: expected a [cout <= 32, cin, 7 or 1, 7, 7] or [cout <= 32, cin, 7, 7] weight, got {tuple(w.shape)}")
    cout, cin, kd = shape[:3]
    w = _c(w, "weight")
    slabs = tuple(torch.empty(((cin + 15) // 16, 49 * kd, 2, cout, 8), dtype=torch.int16, device=w.device) for _ in range(3))
    lib().call("e4s_conv3d_k7_prep_weights_sb3", _p(slabs[0]), _p(slabs[1]), _p(slabs[2]), _p(w), cout, cin, kd, _stream())
    return slabs


def conv3d_k7(x, slabs, bias=None, *, sigmoid: bool = False):
    """``act(conv(x, W, stride 1, zero pad (kd // 2, 3, 3)) + bias)`` of csrc/conv3d_k7.hip on prepared ``slabs`` (``prep_conv3d_k7``): ``x [bs, cin, D, H, W]``
    float32 to ``[bs, cout, D, H, W]``; with kd 1 slabs also ``x [bs, cin, H, W]`` to ``[bs, cout, H, W]`` (a 7 x 7 Conv2d).  ``act``: none, or the sigmoid."""
    x = _c(x, "x")
    kd = slabs[0].shape[1] // 49
    if x.dim() not in ((4, 5) if kd == 1 else (5,)) or x.shape[1] > 16 * slabs[0].shape[0] or x.shape[1] <= 16 * (slabs[0].shape[0] - 1):
        raise ValueError(f"conv3d_k7: x is {tuple(x.shape)}: expected [bs, cin, D, H, W]{' or [bs, cin, H, W]' if kd == 1 else ''} matching the slabs")
    bs, cin = x.shape[:2]
    D, H, W = (1,) * (5 - x.dim()) + tuple(x.shape[2:])
    cout = slabs[0].shape[3]
    out = torch.empty((bs, cout) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    lib().call("e4s_conv3d_k7_sb3", _p(out), _p(x), *[_p(s) for s in slabs], _p(bias), 3 if sigmoid else 0, kd, bs, cin, cout, D, H, W, _stream())
    return out


def _keypoints_checked(name, kp_driving, kp_source, bs=None, K=None):
    """(kp_d, kp_s, jac_d, jac_s) of the two keypoint dicts, which are left as they are: float32 ``value [bs, K, 3]`` and, in both or in neither, ``jacobian
    [bs, K, 3, 3]`` (a ``None`` entry counts as absent, as the reference reads it)."""
    for nm, kp in (("kp_driving", kp_driving), ("kp_source", kp_source)):
        if not hasattr(kp, "keys") or "value" not in kp:
            raise TypeError(f"{name}: {nm} is a keypoint dict with a 'value' entry")
        _tensor_checked(name, f"{nm}['value']", kp["value"], torch.float32, 3, "float32 [bs, num_kp, 3]")
    vd, vs = kp_driving["value"], kp_source["value"]
    bs = vd.shape[0] if bs is None else bs
    K = vd.shape[1] if K is None else K
    for nm, v in (("kp_driving", vd), ("kp_source", vs)):
        if tuple(v.shape) != (bs, K, 3):
            raise ValueError(f"{name}: {nm}['value'] is {tuple(v.shape)}, expected {(bs, K, 3)}: the keypoint shapes do not fit")
    if not 1 <= K <= 31:
        raise ValueError(f"{name}: num_kp {K}: the native kernels take num_kp + 1 <= 32 motions")
    if _has_jacobian(kp_driving) != _has_jacobian(kp_source):
        raise ValueError(f"{name}: a jacobian in only one of kp_driving and kp_source: give both or neither")
    jd = js = None
    if _has_jacobian(kp_driving):
        jd, js = kp_driving["jacobian"], kp_source["jacobian"]
        for nm, j in (("kp_driving", jd), ("kp_source", js)):
            _tensor_checked(name, f"{nm}['jacobian']", j, torch.float32, 4, "float32 [bs, num_kp, 3, 3]")
            if tuple(j.shape) != (bs, K, 3, 3):
                raise ValueError(f"{name}: {nm}['jacobian'] is {tuple(j.shape)}, expected {(bs, K, 3, 3)}: the keypoint shapes do not fit")
    return vd, vs, jd, js


def _keypoints_placed(name, x, kps):
    ts = {nm: t for nm, t in zip(("kp_driving['value']", "kp_source['value']", "kp_driving['jacobian']", "kp_source['jacobian']"), kps) if t is not None}
    _cuda_checked(name, **ts)
    if any(t.device != x.device for t in ts.values()):
        raise RuntimeError(f"{name}: device mismatch among the tensors")
    return [None if t is None else t.detach().contiguous() for t in kps]


def _volume_checked(name, nm, t):
    _tensor_checked(name, nm, t, torch.float32, 5, "a float32 [bs, C, D, H, W] volume")
    if min(t.shape[2:]) < 2:
        raise ValueError(f"{name}: {nm} is {tuple(t.shape)}: every extent of the volume must be at least 2 (the coordinate grid divides by n - 1)")


def motion_input(feature, kp_driving, kp_source, out=None):
    """``e4s_v2v_motion_input``: the hourglass input ``[bs, (K + 1)(c + 1), D, H, W]`` of the compressed ``feature [bs, c, D, H, W]`` and the two keypoint
    dicts: per motion k (0 the background, the identity grid) the heatmap channel ``k (c + 1)`` and the ``c`` features sampled at the sparse motion behind it.
    ``out``: a tensor or channel slice of a dense buffer to write into."""
    name = "motion_input"
    _volume_checked(name, "feature", feature)
    kps = _keypoints_checked(name, kp_driving, kp_source, feature.shape[0])
    _cuda_checked(name, feature=feature)
    kd, ks, jd, js = _keypoints_placed(name, feature, kps)
    feature = feature.detach().contiguous()
    bs, c, D, H, W = feature.shape
    K = kd.shape[1]
    shape = (bs, (K + 1) * (c + 1), D, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=feature.device)
    elif tuple(_req(out, "out").shape) != shape or not _batch_slice(out):
        raise ValueError(f"{name}: out is {tuple(out.shape)}, strides {out.stride()}: expected {shape} with every sample dense")
    lib().call("e4s_v2v_motion_input", _p(out), _p(feature), _p(kd), _p(ks), _p(jd), _p(js), bs, K, c, D, H, W, _bstride(out), _stream())
    return out


def motion_combine(logits, kp_driving, kp_source):
    """``e4s_v2v_motion_combine``: ``(mask [bs, K + 1, D, H, W], deformation [bs, D, H, W, 3])`` of the mask head's ``logits [bs, K + 1, D, H, W]``: the softmax
    over the K + 1 motions and the sparse motions (the bits ``motion_input`` sampled at) weighted with it."""
    name = "motion_combine"
    _volume_checked(name, "logits", logits)
    kps = _keypoints_checked(name, kp_driving, kp_source, logits.shape[0], logits.shape[1] - 1)
    _cuda_checked(name, logits=logits)
    kd, ks, jd, js = _keypoints_placed(name, logits, kps)
    logits = logits.detach().contiguous()
    bs, K1, D, H, W = logits.shape
    mask = torch.empty_like(logits)
    deformation = torch.empty((bs, D, H, W, 3), dtype=torch.float32, device=logits.device)
    lib().call("e4s_v2v_motion_combine", _p(mask), _p(deformation), _p(logits), _p(kd), _p(ks), _p(jd), _p(js), bs, K1 - 1, D, H, W, _stream())
    return mask, deformation


class PreparedDenseMotion(PreparedNet):
    """The kernels' copies of a ``DenseMotionNetwork``'s weights, rebuilt when a tensor changes version or storage: ``compress`` with its bias and ``norm``
    folded in float64 as a 1 x 1 convolution, per DownBlock3d / UpBlock3d and for the decoder's last convolution the 27-tap slabs with the BatchNorm folded, and
    the 7-tap slabs of the ``mask`` and ``occlusion`` heads with their biases."""

    __slots__ = ()
    _entry = "dense_motion_forward"

    def _net(self, weights):
        return _dm_net_of(weights)

    def _build(self, sd, structure, dev):
        _, C, c, down, up, occ = structure
        block = lambda p: prep_conv3d(sd[p + ".conv.weight"], *fold_conv_bn(sd, p + ".conv", p + ".norm"))      # noqa: E731
        return dict(compress=(prep_exact if C < 16 else prep_fwd)(sd["compress.weight"].view(c, C, 1, 1), *fold_conv_bn(sd, "compress", "norm")),
                    enc=[block(f"hourglass.encoder.down_blocks.{i}") for i in range(len(down))],
                    dec=[block(f"hourglass.decoder.up_blocks.{j}") for j in range(len(up))],
                    dec_conv=prep_conv3d(sd["hourglass.decoder.conv.weight"], *fold_conv_bn(sd, "hourglass.decoder.conv", "hourglass.decoder.norm")),
                    mask=(prep_conv3d_k7(sd["mask.weight"]), sd["mask.bias"].contiguous()),
                    occlusion=(prep_conv3d_k7(sd["occlusion.weight"]), sd["occlusion.bias"].contiguous()) if occ else None)


def dense_motion_forward(feature, kp_driving, kp_source, weights):
    """``DenseMotionNetwork.forward(feature, kp_driving, kp_source)`` (dense_motion.py:92-128) in eval mode on the device: ``{'mask' [bs, K + 1, D, H, W],
    'deformation' [bs, D, H, W, 3][, 'occlusion_map' [bs, 1, H, W]]}`` from a float32 ``feature [bs, C, D, H, W]`` and the keypoint dicts (``'value' [bs, K,
    3]`` and, in both or in neither, ``'jacobian' [bs, K, 3, 3]``), which are not modified.  ``weights``: a module with the network's keys
    (``DenseMotionNetwork``, the drop-in), a mapping with them, a generator checkpoint whose keys lie under ``dense_motion_network.``, or the dict ``torch.load``
    returns with a ``generator`` entry; a mapping's structure is read off its keys and shapes.  A module's prepared weights are cached per parameter version.
    Refused with ``ValueError`` before any launch: ``H`` or ``W`` no multiple of ``2 ** num_blocks`` (the reference's own ``torch.cat`` fails there), an extent
    below 2, a depth other than the occlusion head's ``reshape_depth``, ``num_kp + 1 > 32``, keypoint shapes that do not fit, a Jacobian in only one dict,
    anything that is not float32; then a CPU tensor (``RuntimeError``)."""
    name = "dense_motion_forward"
    check_loaded(name, weights, "the weights")
    if not isinstance(weights, nn.Module) and hasattr(weights, "keys") and isinstance(weights.get("generator"), dict):
        weights = weights["generator"]                      # the checkpoint file as torch.load gives it
    checked = _validated(name, weights, _dm_net_of(weights))
    structure = checked[1]
    K, C, c, down, up, occ = structure
    nb = len(down)
    _volume_checked(name, "feature", feature)
    bs, _, D, H, W = feature.shape
    if feature.shape[1] != C:
        raise ValueError(f"{name}: feature is {tuple(feature.shape)}: expected {C} channels (feature_channel)")
    if H % 2 ** nb or W % 2 ** nb:
        raise ValueError(f"{name}: feature is {tuple(feature.shape)}: H and W must be multiples of 2 ** num_blocks = {2 ** nb} (the decoder concatenates each "
                         "upsampled level with the encoder's)")
    if occ and D != occ:
        raise ValueError(f"{name}: feature is {tuple(feature.shape)}: the occlusion head was built for reshape_depth {occ}")
    kps = _keypoints_checked(name, kp_driving, kp_source, bs, K)
    _placed_checked(name, "feature", feature, checked[2])
    kd, ks, jd, js = _keypoints_placed(name, feature, kps)
    infe, outf, levels = _dm_widths(structure)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=feature.device)      # noqa: E731
    if bs == 0:
        out = {"mask": new(0, K + 1, D, H, W), "deformation": new(0, D, H, W, 3)}
        if occ:
            out["occlusion_map"] = new(0, 1, H, W)
        return out
    with torch.no_grad():
        P = prepare(PreparedDenseMotion, weights, checked)
        x = feature.detach().contiguous()
        comp = _conv_any(x.view(bs, C, D * H, W), P["compress"], 1, relu=True).view(bs, c, D, H, W)
        # bufs[j]: torch.cat([up_blocks[j](out), skip], dim=1) at level nb - 1 - j, formed in place
        bufs = [new(bs, up[j] + levels[nb - 1 - j], D, H >> (nb - 1 - j), W >> (nb - 1 - j)) for j in range(nb)]
        src = bufs[-1][:, up[-1]:]                            # the hourglass input: the encoder's first input and the last skip
        lib().call("e4s_v2v_motion_input", _p(src), _p(comp), _p(kd), _p(ks), _p(jd), _p(js), bs, K, c, D, H, W, _bstride(src), _stream())
        for i in range(nb):
            full = conv3d_sb3(src, *P["enc"][i], relu=True)
            if i + 1 < nb:
                j = nb - 2 - i
                dst = bufs[j][:, up[j]:]
            else:
                dst = new(bs, down[i], D, H >> (i + 1), W >> (i + 1))
            _pool_into(full, dst)
            src = dst
        cur = src
        for j in range(nb):
            conv3d_sb3(cur, *P["dec"][j], relu=True, up_hw=2, out=bufs[j][:, :up[j]])
            cur = bufs[j]
        prediction = conv3d_sb3(cur, *P["dec_conv"], relu=True)
        logits = conv3d_k7(prediction, *P["mask"])
        mask = torch.empty_like(logits)
        deformation = new(bs, D, H, W, 3)
        lib().call("e4s_v2v_motion_combine", _p(mask), _p(deformation), _p(logits), _p(kd), _p(ks), _p(jd), _p(js), bs, K, D, H, W, _stream())
        out = {"mask": mask, "deformation": deformation}
        if occ:
            out["occlusion_map"] = conv3d_k7(prediction.view(bs, outf * D, H, W), *P["occlusion"], sigmoid=True)
    return out


# ================================================================================================ row f19: stage 3, the generator's feature warp
# ``OcclusionAwareSPADEGenerator.forward`` of swap_face_fine/face_vid2vid/modules/generator.py:210-244 up to the input of ``self.decoder``, in eval mode:
#
#     per clip       first (3 channels: the exact e4s_conv2d) and down_blocks (e4s_conv2d_sb3, e4s_avgpool2x2), BatchNorm folded in float64, ReLU fused; second,
#                    the 1 x 1 with its bias, whose output [bs, C D, h, w] IS the volume [bs, C, D, h, w]; per ResBlock3d three launches: e4s_v2v_bn_relu (norm1
#                    and the ReLU stand in front of conv1's zero padding: no fold), e4s_conv3d_sb3 with norm2 folded and ReLU, e4s_conv3d_sb3 with the block's
#                    input as residual (the Cout <= 32 tile at the upstream width)
#     per frame      dense_motion_forward (row f18); e4s_v2v_deform, whose output [n, C D, h, w] is the reference's view; third on e4s_conv2d_sb3 with the
#                    BatchNorm folded and nn.LeakyReLU()'s default slope 0.01 through the PReLU epilogue; fourth, a 1 x 1; e4s_v2v_occlude in place
#
# ``make_animation`` calls the generator once per driving frame and so recomputes the per-clip part every frame; here ``appearance_feature`` is computed once and
# ``generator_warp`` takes it, a batch-1 volume shared by every frame of a call (the gather reads it through a batch stride of 0).  Two branches of the reference
# cannot be reached with this DenseMotionNetwork, which returns a deformation and an occlusion map at the feature's own size: the trilinear resize of the
# deformation and the bilinear resize of the occlusion map.  Neither is built; a size mismatch is refused.  The ``SPADEDecoder`` is stage 4: the mirror module
# holds its keys and a stock-PyTorch forward, the native path ends at its input.
LEAKY_SLOPE = 0.01                           # nn.LeakyReLU()'s default, SameBlock2d(lrelu=True)
DENSE_MOTION_PARAMS = dict(block_expansion=32, max_features=1024, num_blocks=5, reshape_depth=16, compress=4)      # vox-256.yaml: dense_motion_params
_UPSTREAM = object()                         # the default of ``dense_motion_params``: the upstream dict; None is the reference's "no dense-motion network"


def generator_structure(image_channel=3, feature_channel=32, num_kp=15, block_expansion=64, max_features=512, num_down_blocks=2, reshape_channel=32,
                        reshape_depth=16, num_resblocks=6, estimate_occlusion_map=True, dense_motion_params=_UPSTREAM, estimate_jacobian=False):
    """The constructor arithmetic of ``OcclusionAwareSPADEGenerator`` as ``(image_channel, kernel size of first (3), block_expansion, down widths, max_features,
    reshape_channel, reshape_depth, num_resblocks, width of third and fourth, the dense-motion structure or None)``; refuses what the reference's own forward
    cannot run."""
    if not all(_is_int(v) for v in (image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel, reshape_depth,
                                    num_resblocks)):
        raise ValueError("OcclusionAwareSPADEGenerator: image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel, "
                         "reshape_depth and num_resblocks are ints")
    if min(image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel, reshape_depth) < 1 or num_resblocks < 0:
        raise ValueError("OcclusionAwareSPADEGenerator: widths, depths and counts are positive (num_down_blocks at least 1: the reference's `second` takes the "
                         "last down block's width)")
    if image_channel != 3:
        raise ValueError(f"OcclusionAwareSPADEGenerator: image_channel {image_channel} is not implemented: the native network takes three colour channels")
    if max_features != reshape_channel * reshape_depth:
        raise ValueError(f"OcclusionAwareSPADEGenerator: max_features {max_features} != reshape_channel * reshape_depth = {reshape_channel} * {reshape_depth}: "
                         "the output of `second` is viewed as that volume")
    if block_expansion > max_features:
        raise ValueError(f"OcclusionAwareSPADEGenerator: block_expansion {block_expansion} above max_features {max_features}: the reference's first down block "
                         "takes min(max_features, block_expansion) channels from `first`'s block_expansion, its own forward does not fit")
    dm = None
    if dense_motion_params is not None:
        params = dict(DENSE_MOTION_PARAMS if dense_motion_params is _UPSTREAM else dense_motion_params)
        dm = dense_motion_structure(num_kp=num_kp, feature_channel=feature_channel, estimate_occlusion_map=estimate_occlusion_map, **params)
        if feature_channel != reshape_channel:
            raise ValueError(f"OcclusionAwareSPADEGenerator: feature_channel {feature_channel} != reshape_channel {reshape_channel}: the dense-motion network's "
                             "`compress` takes the feature volume")
        if dm[5] and dm[5] != reshape_depth:
            raise ValueError(f"OcclusionAwareSPADEGenerator: the dense-motion network's reshape_depth {dm[5]} != reshape_depth {reshape_depth}: its occlusion head "
                             "views the volume's depth into channels")
    down = tuple(min(max_features, block_expansion * 2 ** (i + 1)) for i in range(num_down_blocks))
    return (int(image_channel), 3, int(block_expansion), down, int(max_features), int(reshape_channel), int(reshape_depth), int(num_resblocks),
            int(block_expansion * 2 ** num_down_blocks), dm)


class _SameBlock2d(nn.Module):
    def __init__(self, cin, cout, k, lrelu=False):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2)
        self.norm = nn.BatchNorm2d(cout, affine=True)
        self.ac = nn.LeakyReLU() if lrelu else nn.ReLU()

    def forward(self, x):
        return self.ac(self.norm(self.conv(x)))


class _ResBlock3d(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1 = nn.Conv3d(c, c, 3, padding=1)
        self.conv2 = nn.Conv3d(c, c, 3, padding=1)
        self.norm1 = nn.BatchNorm3d(c, affine=True)
        self.norm2 = nn.BatchNorm3d(c, affine=True)

    def forward(self, x):
        out = self.conv1(F.relu(self.norm1(x)))
        return self.conv2(F.relu(self.norm2(out))) + x


class _SPADE(nn.Module):
    def __init__(self, norm_nc, label_nc):
        super().__init__()
        self.param_free_norm = nn.InstanceNorm2d(norm_nc, affine=False)
        self.mlp_shared = nn.Sequential(nn.Conv2d(label_nc, 128, 3, padding=1), nn.ReLU())
        self.mlp_gamma = nn.Conv2d(128, norm_nc, 3, padding=1)
        self.mlp_beta = nn.Conv2d(128, norm_nc, 3, padding=1)

    def forward(self, x, segmap):
        actv = self.mlp_shared(F.interpolate(segmap, size=x.shape[2:], mode="nearest"))
        return self.param_free_norm(x) * (1 + self.mlp_gamma(actv)) + self.mlp_beta(actv)


class _SPADEResnetBlock(nn.Module):
    """``SPADEResnetBlock(fin, fout, 'spadespectralinstance', label_nc)`` of modules/util.py:444-481."""

    def __init__(self, fin, fout, label_nc):
        super().__init__()
        self.learned_shortcut = fin != fout
        fmiddle = min(fin, fout)
        sn = torch.nn.utils.spectral_norm
        self.conv_0 = sn(nn.Conv2d(fin, fmiddle, 3, padding=1))
        self.conv_1 = sn(nn.Conv2d(fmiddle, fout, 3, padding=1))
        if self.learned_shortcut:
            self.conv_s = sn(nn.Conv2d(fin, fout, 1, bias=False))
        self.norm_0 = _SPADE(fin, label_nc)
        self.norm_1 = _SPADE(fmiddle, label_nc)
        if self.learned_shortcut:
            self.norm_s = _SPADE(fin, label_nc)

    def forward(self, x, seg):
        x_s = self.conv_s(self.norm_s(x, seg)) if self.learned_shortcut else x
        dx = self.conv_0(F.leaky_relu(self.norm_0(x, seg), 2e-1))
        dx = self.conv_1(F.leaky_relu(self.norm_1(dx, seg), 2e-1))
        return x_s + dx


class SPADEDecoder(nn.Module):
    """``SPADEDecoder()`` of modules/generator.py:120-158 with its keys (``torch.nn.utils.spectral_norm``'s ``weight_orig`` / ``weight_u`` / ``weight_v``
    included): 256 input channels, fixed.  ``forward`` is the plain PyTorch composition in eval mode; the native decoder is stage 4."""

    def __init__(self):
        super().__init__()
        ic, oc, label_nc = 256, 64, 256
        self.fc = nn.Conv2d(ic, 2 * ic, 3, padding=1)
        for i in range(6):
            setattr(self, f"G_middle_{i}", _SPADEResnetBlock(2 * ic, 2 * ic, label_nc))
        self.up_0 = _SPADEResnetBlock(2 * ic, ic, label_nc)
        self.up_1 = _SPADEResnetBlock(ic, oc, label_nc)
        self.conv_img = nn.Conv2d(oc, 3, 3, padding=1)
        self.up = nn.Upsample(scale_factor=2)

    def forward(self, feature):
        if self.training:
            raise NotImplementedError("SPADEDecoder: training mode is not implemented (spectral norm's power iteration); call .eval()")
        x = self.fc(feature)
        for i in range(6):
            x = getattr(self, f"G_middle_{i}")(x, feature)
        x = self.up_0(self.up(x), feature)
        x = self.up_1(self.up(x), feature)
        return torch.sigmoid(self.conv_img(F.leaky_relu(x, 2e-1)))


class OcclusionAwareSPADEGenerator(_Loadable):
    """``OcclusionAwareSPADEGenerator(image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel, reshape_depth,
    num_resblocks, estimate_occlusion_map, dense_motion_params, estimate_jacobian)`` of swap_face_fine/face_vid2vid/modules/generator.py:161-251 with its
    ``state_dict`` keys, shapes and order; the defaults are the upstream ``vox-256.yaml`` with the occlusion head (``checkpoint['generator']`` loads with
    ``strict=True``).  ``forward(source_image, kp_driving, kp_source)`` is the plain PyTorch composition of the whole generator in eval mode, decoder included,
    returning ``{'mask'[, 'occlusion_map'], 'prediction'}``; ``front`` is its part up to the decoder's input, what the tests compare ``generator_front_forward``
    with.  ``dense_motion_params=None`` builds, as the reference does, a generator without a dense-motion network, which no forward here runs."""
    _PROBE = ("second.weight", "third.conv.weight")

    def __init__(self, image_channel=3, feature_channel=32, num_kp=15, block_expansion=64, max_features=512, num_down_blocks=2, reshape_channel=32,
                 reshape_depth=16, num_resblocks=6, estimate_occlusion_map=True, dense_motion_params=_UPSTREAM, estimate_jacobian=False):
        super().__init__()
        self.structure = generator_structure(image_channel, feature_channel, num_kp, block_expansion, max_features, num_down_blocks, reshape_channel,
                                             reshape_depth, num_resblocks, estimate_occlusion_map, dense_motion_params, estimate_jacobian)
        _, k, bexp, down, _, _, _, _, outf, dm = self.structure
        if dm is not None:
            params = dict(DENSE_MOTION_PARAMS if dense_motion_params is _UPSTREAM else dense_motion_params)
            self.dense_motion_network = DenseMotionNetwork(num_kp=num_kp, feature_channel=feature_channel, estimate_occlusion_map=estimate_occlusion_map, **params)
        else:
            self.dense_motion_network = None
        self.first = _SameBlock2d(image_channel, bexp, k)
        self.down_blocks = nn.ModuleList([_DownBlock2d(bexp if i == 0 else down[i - 1], c) for i, c in enumerate(down)])
        self.second = nn.Conv2d(down[-1], max_features, 1)
        self.reshape_channel, self.reshape_depth = reshape_channel, reshape_depth
        self.resblocks_3d = nn.Sequential()
        for i in range(num_resblocks):
            self.resblocks_3d.add_module(f"3dr{i}", _ResBlock3d(reshape_channel))
        self.third = _SameBlock2d(max_features, outf, 3, lrelu=True)
        self.fourth = nn.Conv2d(outf, outf, 1)
        self.estimate_occlusion_map, self.image_channel = estimate_occlusion_map, image_channel
        self.decoder = SPADEDecoder()
        self.requires_grad_(False)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        dm = self.dense_motion_network                        # filled through this module's keys, not through its own load_state_dict
        if dm is not None and all("dense_motion_network." + k in state_dict for k in dm._PROBE):
            dm._loaded = True
        return out

    def source_feature(self, source_image):
        out = self.first(source_image)
        for block in self.down_blocks:
            out = block(out)
        out = self.second(out)
        bs, _, h, w = out.shape
        return self.resblocks_3d(out.view(bs, self.reshape_channel, self.reshape_depth, h, w))

    def warp(self, feature_3d, kp_driving, kp_source):
        if self.dense_motion_network is None:
            raise ValueError("OcclusionAwareSPADEGenerator: built with dense_motion_params=None: the reference's forward has no input for its decoder then")
        n = kp_driving["value"].shape[0]
        if feature_3d.shape[0] == 1 and n != 1:                  # one source for n driving frames: what n calls of the reference compute
            feature_3d = feature_3d.expand(n, -1, -1, -1, -1)
        dense_motion = self.dense_motion_network(feature_3d, kp_driving, kp_source)
        out = {"mask": dense_motion["mask"], "deformation": dense_motion["deformation"]}
        warped = F.grid_sample(feature_3d, dense_motion["deformation"], align_corners=False)
        bs, c, d, h, w = warped.shape
        feature = self.fourth(self.third(warped.view(bs, c * d, h, w)))
        if "occlusion_map" in dense_motion:
            out["occlusion_map"] = dense_motion["occlusion_map"]
            feature = feature * dense_motion["occlusion_map"]
        out["feature"] = feature
        return out

    def front(self, source_image, kp_driving, kp_source):
        """``{'mask', 'deformation'[, 'occlusion_map'], 'feature'}``: ``forward`` up to the input of ``self.decoder``."""
        if self.training:
            raise NotImplementedError("OcclusionAwareSPADEGenerator: training mode is not implemented; call .eval()")
        with torch.no_grad():
            return self.warp(self.source_feature(source_image), kp_driving, kp_source)

    def forward(self, source_image, kp_driving, kp_source):
        out = self.front(source_image, kp_driving, kp_source)
        with torch.no_grad():
            out["prediction"] = self.decoder(out.pop("feature"))
        del out["deformation"]                                # the reference's output_dict holds the mask, the occlusion map and the prediction
        return out


def _spade_shapes(out, p, norm_nc, label_nc):
    out[p + ".mlp_shared.0.weight"], out[p + ".mlp_shared.0.bias"] = (128, label_nc, 3, 3), (128,)
    for nm in ("mlp_gamma", "mlp_beta"):
        out[f"{p}.{nm}.weight"], out[f"{p}.{nm}.bias"] = (norm_nc, 128, 3, 3), (norm_nc,)


def spade_decoder_state_dict_shapes():
    """``{key: shape}`` of ``SPADEDecoder().state_dict()``, in its order."""
    out = {"fc.weight": (512, 256, 3, 3), "fc.bias": (512,)}

    def sn(p, co, ci, k, bias=True):
        if bias:
            out[p + ".bias"] = (co,)
        out[p + ".weight_orig"], out[p + ".weight_u"], out[p + ".weight_v"] = (co, ci, k, k), (co,), (ci * k * k,)

    for p, fin, fout in [(f"G_middle_{i}", 512, 512) for i in range(6)] + [("up_0", 512, 256), ("up_1", 256, 64)]:
        mid = min(fin, fout)
        sn(p + ".conv_0", mid, fin, 3), sn(p + ".conv_1", fout, mid, 3)
        if fin != fout:
            sn(p + ".conv_s", fout, fin, 1, bias=False)
        _spade_shapes(out, p + ".norm_0", fin, 256), _spade_shapes(out, p + ".norm_1", mid, 256)
        if fin != fout:
            _spade_shapes(out, p + ".norm_s", fin, 256)
    out["conv_img.weight"], out["conv_img.bias"] = (3, 64, 3, 3), (3,)
    return out


def generator_structure_shapes(structure, decoder: bool = True):
    """``{key: shape}`` of the ``OcclusionAwareSPADEGenerator`` with ``structure`` (``generator_structure``), in ``state_dict`` order; without ``decoder`` the
    keys of the front alone: everything the native path reads."""
    cin, k, bexp, down, maxf, rc, _, nres, outf, dm = structure
    out = {}
    if dm is not None:
        out.update({"dense_motion_network." + key: v for key, v in dense_motion_structure_shapes(dm).items()})

    def conv(p, co, ci, kk):
        out[p + ".weight"], out[p + ".bias"] = (co, ci, kk, kk), (co,)

    conv("first.conv", bexp, cin, k), bn_shapes(out, "first.norm", bexp)
    for i, c in enumerate(down):
        conv(f"down_blocks.{i}.conv", c, bexp if i == 0 else down[i - 1], 3), bn_shapes(out, f"down_blocks.{i}.norm", c)
    conv("second", maxf, down[-1], 1)
    for i in range(nres):
        p = f"resblocks_3d.3dr{i}"
        for nm in ("conv1", "conv2"):
            out[f"{p}.{nm}.weight"], out[f"{p}.{nm}.bias"] = (rc, rc, 3, 3, 3), (rc,)
        bn_shapes(out, p + ".norm1", rc), bn_shapes(out, p + ".norm2", rc)
    conv("third.conv", outf, maxf, 3), bn_shapes(out, "third.norm", outf)
    conv("fourth", outf, outf, 1)
    if decoder:
        out.update({"decoder." + key: v for key, v in spade_decoder_state_dict_shapes().items()})
    return out


def generator_front_structure_shapes(structure):
    """``generator_structure_shapes`` without the ``decoder.`` keys: what ``PreparedGeneratorFront`` validates a mapping against."""
    return generator_structure_shapes(structure, decoder=False)


def generator_state_dict_shapes(**config):
    """``{key: shape}`` of ``OcclusionAwareSPADEGenerator(**config).state_dict()``, in its order (the upstream configuration by default)."""
    return generator_structure_shapes(generator_structure(**config))


def generator_structure_of_keys(sd, name="generator_structure_of_keys"):
    """The structure (``generator_structure``) read off the keys and shapes of a mapping with the generator's bare keys; the ``decoder.`` keys are not needed."""
    cls = "OcclusionAwareSPADEGenerator"
    first = _shape_of(name, sd, "first.conv.weight", 4, cls)
    if first[2:] != (3, 3):
        raise ValueError(f"{name}: 'first.conv.weight' is {first}: the SPADE generator's `first` is a 3 x 3 convolution (7 x 7 is OcclusionAwareGenerator's, which "
                         "is not implemented)")
    bexp, cin, k = first[:3]
    down, i = [], 0
    while f"down_blocks.{i}.conv.weight" in sd:
        down.append(_shape_of(name, sd, f"down_blocks.{i}.conv.weight", 4, cls)[0])
        i += 1
    maxf = _shape_of(name, sd, "second.weight", 4, cls)[0]
    nres = 0
    while f"resblocks_3d.3dr{nres}.conv1.weight" in sd:
        nres += 1
    outf = _shape_of(name, sd, "third.conv.weight", 4, cls)[0]
    dm = None
    if any(key.startswith("dense_motion_network.") for key in sd.keys()):
        dm = _dm_structure_of_keys(name, {key[len("dense_motion_network."):]: v for key, v in sd.items() if key.startswith("dense_motion_network.")})
    # a generator without a ResBlock3d does not say how `second`'s channels split into (channel, depth): the dense-motion network does
    rc = _shape_of(name, sd, "resblocks_3d.3dr0.conv1.weight", 5, cls)[0] if nres else (dm[1] if dm is not None else 0)
    if not down or rc < 1 or maxf % rc:
        raise ValueError(f"{name}: the weights are not an OcclusionAwareSPADEGenerator the native path implements ({len(down)} down blocks, {maxf} channels of "
                         f"`second` for a reshape_channel of {rc})")
    return cin, k, bexp, tuple(down), maxf, rc, maxf // rc, nres, outf, dm


_GEN_NET = _Net("OcclusionAwareSPADEGenerator", generator_front_structure_shapes, ("generator.", "module.generator.", "module."), True, ("second.weight",),
                lambda name, sd: generator_structure_of_keys(sd, name), EVAL_ONLY, ("num_batches_tracked",))


def _gen_net_of(weights):
    return module_net(_GEN_NET, weights.structure) if isinstance(weights, OcclusionAwareSPADEGenerator) else _GEN_NET


class PreparedGeneratorFront(PreparedNet):
    """The kernels' copies of the weights of an ``OcclusionAwareSPADEGenerator`` in front of its decoder, rebuilt when a tensor changes version or storage:
    ``first``, the down blocks and ``third`` with their bias and BatchNorm folded in float64 (K-major fp32 under 16 input channels, three-way split slabs
    otherwise), ``second`` and ``fourth`` with their bias, per ResBlock3d ``norm1`` as float32 (scale, shift), ``conv1`` with ``norm2`` folded and ``conv2`` with
    its bias as 27-tap slabs, and ``third``'s slope vector.  Takes a module, the mapping ``torch.load`` returns (``checkpoint['generator']`` or the whole
    checkpoint) or a mapping without any ``decoder.`` key: the front reads none of them.  The dense-motion network's weights are ``PreparedDenseMotion``'s."""

    __slots__ = ()
    _entry = "generator_front_forward"

    def _net(self, weights):
        return _gen_net_of(weights)

    def _build(self, sd, structure, dev):
        _, _, _, down, _, _, _, nres, outf, _ = structure
        res = []
        for i in range(nres):
            p = f"resblocks_3d.3dr{i}"
            scale, shift = lossnet.bn_fold(sd, p + ".norm1")
            res.append(dict(scale=scale.float().contiguous(), shift=shift.float().contiguous(),
                            c1=prep_conv3d(sd[p + ".conv1.weight"], *fold_conv_bn(sd, p + ".conv1", p + ".norm2")),
                            c2=prep_conv3d(sd[p + ".conv2.weight"], None, sd[p + ".conv2.bias"].double())))
        return dict(first=_prep2d(sd, "first.conv", "first.norm"), down=[_prep2d(sd, f"down_blocks.{i}.conv", f"down_blocks.{i}.norm") for i in range(len(down))],
                    second=_prep2d(sd, "second"), res=res, third=_prep2d(sd, "third.conv", "third.norm"), fourth=_prep2d(sd, "fourth"),
                    slope=torch.full((outf,), LEAKY_SLOPE, dtype=torch.float32, device=dev))


def bn_relu(x, scale, shift, out=None):
    """``e4s_v2v_bn_relu``: ``relu(x * scale[c] + shift[c])`` over a float32 ``x [bs, C, ...]`` with float32 ``scale``, ``shift [C]`` (an eval-mode BatchNorm as
    ``lossnet.bn_fold`` gives it, rounded to float32); ``out``: a dense tensor of x's shape, x itself allowed."""
    name = "bn_relu"
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError(f"{name}: x: expected a float32 [bs, C, ...] tensor, got {getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    C = x.shape[1]
    for nm, t in (("scale", scale), ("shift", shift)):
        _tensor_checked(name, nm, t, torch.float32, 1, f"float32 [{C}]")
        if t.shape[0] != C:
            raise ValueError(f"{name}: {nm} is {tuple(t.shape)} for x {tuple(x.shape)}: expected [{C}]")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous()):
        raise ValueError(f"{name}: out: expected a dense float32 tensor of x's shape {tuple(x.shape)}")
    _cuda_checked(name, x=x, scale=scale, shift=shift, **({"out": out} if out is not None else {}))
    x, scale, shift = x.detach().contiguous(), scale.detach().contiguous(), shift.detach().contiguous()
    if out is None:
        out = torch.empty_like(x)
    n = x[0, 0].numel() if x.numel() else 1
    lib().call("e4s_v2v_bn_relu", _p(out), _p(x), _p(scale), _p(shift), x.shape[0], C, max(n, 1), _stream())
    return out


def occlude(x, occlusion_map, out=None):
    """``e4s_v2v_occlude``: ``x [bs, C, h, w] * occlusion_map [bs, 1, h, w]``, float32; ``out``: a dense tensor of x's shape, x itself allowed (in place).  The
    reference resizes an occlusion map of another size bilinearly; the dense-motion network never returns one, and a size mismatch is refused."""
    name = "occlude"
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, C, h, w] tensor")
    _tensor_checked(name, "occlusion_map", occlusion_map, torch.float32, 4, "a float32 [bs, 1, h, w] map")
    bs, C, h, w = x.shape
    if tuple(occlusion_map.shape) != (bs, 1, h, w):
        raise ValueError(f"{name}: occlusion_map is {tuple(occlusion_map.shape)} for x {tuple(x.shape)}: expected {(bs, 1, h, w)} (the bilinear resize of a map of "
                         "another size is not implemented: the dense-motion network returns the feature's size)")
    if C < 1 or h * w < 1:
        raise ValueError(f"{name}: x is {tuple(x.shape)}: no empty channel or plane")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous()):
        raise ValueError(f"{name}: out: expected a dense float32 tensor of x's shape {tuple(x.shape)}")
    _cuda_checked(name, x=x, occlusion_map=occlusion_map, **({"out": out} if out is not None else {}))
    if out is not None and out.data_ptr() == x.data_ptr() and not x.is_contiguous():
        raise ValueError(f"{name}: in place needs a dense x")
    x, occ = x.detach().contiguous(), occlusion_map.detach().contiguous()
    if out is None:
        out = torch.empty_like(x)
    lib().call("e4s_v2v_occlude", _p(out), _p(x), _p(occ), bs, C, h * w, _stream())
    return out


def _deform_checked(name, feature_3d, deformation):
    _tensor_checked(name, "feature_3d", feature_3d, torch.float32, 5, "a float32 [bs, C, D, h, w] volume")
    _tensor_checked(name, "deformation", deformation, torch.float32, 5, "a float32 [n, D, h, w, 3] sampling grid")
    fb, C, D, H, W = feature_3d.shape
    n = deformation.shape[0]
    if tuple(deformation.shape[1:]) != (D, H, W, 3):
        raise ValueError(f"{name}: deformation is {tuple(deformation.shape)} for feature_3d {tuple(feature_3d.shape)}: expected [n, {D}, {H}, {W}, 3] (the trilinear "
                         "resize of a deformation of another size is not implemented: the dense-motion network returns the feature's size)")
    if fb != n and fb != 1:
        raise ValueError(f"{name}: feature_3d is {tuple(feature_3d.shape)} for a deformation of batch {n}: expected a batch of {n}, or 1 (shared by every sample)")
    if min(C, D, H, W) < 1:
        raise ValueError(f"{name}: feature_3d is {tuple(feature_3d.shape)}: no empty extent")
    return n, C, D, H, W


def deform_feature(feature_3d, deformation, out=None):
    """``e4s_v2v_deform``: the reference's ``deform_input`` and the ``view`` behind it: ``F.grid_sample(feature_3d [bs, C, D, h, w], deformation [n, D, h, w,
    3])`` at its defaults (trilinear, zero padding, ``align_corners=False``) as ``[n, C D, h, w]``.  A ``feature_3d`` of batch 1 against a deformation of batch n
    is read through a batch stride of 0: one source feature for every driving frame, without a copy (so is a batch-1 volume ``expand``ed to n).  ``out``: a
    ``[n, C D, h, w]`` tensor or channel slice of a dense buffer to write into."""
    name = "deform_feature"
    n, C, D, H, W = _deform_checked(name, feature_3d, deformation)
    shape = (n, C * D, H, W)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape or not _batch_slice(out)):
        raise ValueError(f"{name}: out: expected float32 {shape} with every sample dense, got {getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))}")
    _cuda_checked(name, feature_3d=feature_3d, deformation=deformation, **({"out": out} if out is not None else {}))
    if deformation.device != feature_3d.device or (out is not None and out.device != feature_3d.device):
        raise RuntimeError(f"{name}: device mismatch among the tensors")
    feature_3d = feature_3d.detach()
    shared = feature_3d.shape[0] == 1 or (n > 1 and feature_3d.stride(0) == 0)
    if shared:
        feature_3d = feature_3d[:1]
    x = feature_3d if _batch_slice(feature_3d) else feature_3d.contiguous()
    deformation = deformation.detach().contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if n:
        lib().call("e4s_v2v_deform", _p(out), _p(x), _p(deformation), n, C, D, H, W, 0 if shared else _bstride(x), _bstride(out), _stream())
    return out


def _generator_checked(name, weights):
    """(weights without the checkpoint's wrapping, what ``_validated`` returns, the structure); a generator without a dense-motion network is refused."""
    check_loaded(name, weights, "the weights")
    if not isinstance(weights, nn.Module) and hasattr(weights, "keys") and isinstance(weights.get("generator"), dict):
        weights = weights["generator"]                      # the checkpoint file as torch.load gives it
    if isinstance(weights, OcclusionAwareSPADEGenerator) and weights.structure[9] is None:
        raise ValueError(f"{name}: the generator was built with dense_motion_params=None: without a dense-motion network there is no deformation to warp by")
    checked = _validated(name, weights, _gen_net_of(weights))
    if checked[1][9] is None:
        raise ValueError(f"{name}: the weights hold no dense_motion_network. keys (dense_motion_params=None): without a dense-motion network there is no "
                         "deformation to warp by")
    return weights, checked, checked[1]


def _feature_size_checked(name, nm, shape, structure, h, w):
    """The feature plane ``h x w`` must be one the dense-motion network takes: multiples of 2 ** num_blocks, at least 2."""
    nb = len(structure[9][3])
    if min(h, w) < 2 or structure[6] < 2:
        raise ValueError(f"{name}: {nm} is {tuple(shape)}: the feature volume would be {structure[6]} x {h} x {w}, every extent must be at least 2 (the "
                         "dense-motion network's coordinate grid divides by n - 1)")
    if h % 2 ** nb or w % 2 ** nb:
        raise ValueError(f"{name}: {nm} is {tuple(shape)}: the feature plane {h} x {w} must be multiples of 2 ** num_blocks = {2 ** nb} of the dense-motion network")


def appearance_feature(source, weights):
    """The source-only part of ``OcclusionAwareSPADEGenerator.forward`` (generator.py:212-219) in eval mode on the device: ``first``, the down blocks, ``second``,
    the view and ``resblocks_3d``: ``feature_3d [bs, reshape_channel, reshape_depth, H / 2 ** num_down_blocks, W / 2 ** num_down_blocks]`` from a float32
    ``source [bs, 3, H, W]``.  It does not depend on the driving frame: compute it once per clip and hand it to ``generator_warp``.  ``weights``: an
    ``OcclusionAwareSPADEGenerator``, the mapping ``torch.load`` returns (``checkpoint['generator']`` or the checkpoint itself) or a mapping without the
    ``decoder.`` keys.  Refused with ``ValueError`` before any launch: anything not float32, other than three channels, a size that ``2 ** num_down_blocks`` does
    not divide or that leaves the dense-motion network an extent it refuses, a generator without a dense-motion network; then a CPU tensor (``RuntimeError``)."""
    name = "appearance_feature"
    weights, checked, structure = _generator_checked(name, weights)
    _tensor_checked(name, "source", source, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    _, k, _, down, maxf, rc, depth, _, _, _ = structure
    bs, ch, H, W = source.shape
    if ch != 3:
        raise ValueError(f"{name}: source is {tuple(source.shape)}: expected three colour channels")
    f = 2 ** len(down)
    if H % f or W % f or min(H, W) < f or max(H, W) > 16384:
        raise ValueError(f"{name}: source is {tuple(source.shape)}: H and W must be multiples of 2 ** num_down_blocks = {f} (the reference's pools would drop a row "
                         "or column), up to 16384")
    h, w = H // f, W // f
    _feature_size_checked(name, "source", source.shape, structure, h, w)
    _placed_checked(name, "source", source, checked[2])
    if bs == 0:
        return source.new_empty((0, rc, depth, h, w))
    with torch.no_grad():
        P = prepare(PreparedGeneratorFront, weights, checked)
        cur = _conv_any(source.detach().contiguous(), P["first"], k, relu=True)
        for L in P["down"]:
            cur = avgpool2x2(_conv_any(cur, L, 3, relu=True))
        cur = _conv_any(cur, P["second"], 1).view(bs, rc, depth, h, w)
        for R in P["res"]:
            t = torch.empty_like(cur)
            lib().call("e4s_v2v_bn_relu", _p(t), _p(cur), _p(R["scale"]), _p(R["shift"]), bs, rc, depth * h * w, _stream())
            t = conv3d_sb3(t, *R["c1"], relu=True)
            cur = conv3d_sb3(t, *R["c2"], residual=cur)
    return cur


def generator_warp(feature_3d, kp_driving, kp_source, weights):
    """The per-frame part of ``OcclusionAwareSPADEGenerator.forward`` (generator.py:221-244) in eval mode on the device: the dense-motion network, ``deform_input``,
    ``third``, ``fourth`` and the product with the occlusion map: ``{'mask' [n, K + 1, D, h, w], 'deformation' [n, D, h, w, 3][, 'occlusion_map' [n, 1, h, w]],
    'feature' [n, block_expansion 2 ** num_down_blocks, h, w]}``, ``feature`` the decoder's input.  The batch n is that of the keypoint dicts; a ``feature_3d``
    (``appearance_feature``) of batch 1 is shared by all n frames.  ``weights`` and the refusals as ``appearance_feature``'s, and ``dense_motion_forward``'s for
    the keypoints."""
    name = "generator_warp"
    weights, checked, structure = _generator_checked(name, weights)
    _, _, _, _, maxf, rc, depth, _, outf, dm = structure
    _tensor_checked(name, "feature_3d", feature_3d, torch.float32, 5, "a float32 [bs, C, D, h, w] volume")
    fb, _, _, h, w = feature_3d.shape
    if tuple(feature_3d.shape[1:3]) != (rc, depth):
        raise ValueError(f"{name}: feature_3d is {tuple(feature_3d.shape)}: expected [bs, {rc}, {depth}, h, w] (reshape_channel, reshape_depth)")
    _feature_size_checked(name, "feature_3d", feature_3d.shape, structure, h, w)
    kps = _keypoints_checked(name, kp_driving, kp_source, None, dm[0])
    n = kps[0].shape[0]
    if fb != n and fb != 1:
        raise ValueError(f"{name}: feature_3d is {tuple(feature_3d.shape)} for keypoints of batch {n}: expected a batch of {n}, or 1 (shared by every frame)")
    _placed_checked(name, "feature_3d", feature_3d, checked[2])
    _keypoints_placed(name, feature_3d, kps)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=feature_3d.device)      # noqa: E731
    if n == 0:
        out = {"mask": new(0, dm[0] + 1, depth, h, w), "deformation": new(0, depth, h, w, 3)}
        if dm[5]:
            out["occlusion_map"] = new(0, 1, h, w)
        out["feature"] = new(0, outf, h, w)
        return out
    with torch.no_grad():
        P = prepare(PreparedGeneratorFront, weights, checked)
        feature_3d = feature_3d.detach()
        # dense_motion_forward takes a dense batch: the shared volume is copied n times here (8 MB per frame at the upstream size), the gather reads it in place
        # a mapping goes on as the validated bare keys (a `generator.` prefix or the file's nesting is gone): its dense_motion_network. keys are what
        # dense_motion_forward understands
        dmw = weights.dense_motion_network if isinstance(weights, nn.Module) else checked[0]
        out = dense_motion_forward(feature_3d.expand(n, -1, -1, -1, -1) if fb != n else feature_3d, kp_driving, kp_source, dmw)
        warped = deform_feature(feature_3d, out["deformation"])
        w3, b3 = P["third"]
        conv = conv_sb if isinstance(w3, tuple) else conv_exact
        feature = _conv_any(conv(warped, w3, b3, k=3, slope=P["slope"]), P["fourth"], 1)
        if "occlusion_map" in out:
            lib().call("e4s_v2v_occlude", _p(feature), _p(feature), _p(out["occlusion_map"]), n, outf, h * w, _stream())
        out["feature"] = feature
    return out


def generator_front_forward(source, kp_driving, kp_source, weights):
    """``OcclusionAwareSPADEGenerator.forward(source, kp_driving, kp_source)`` up to the input of its decoder: ``generator_warp(appearance_feature(source,
    weights), kp_driving, kp_source, weights)``.  ``source`` holds one image, or one per keypoint set."""
    name = "generator_front_forward"
    _generator_checked(name, weights)
    _tensor_checked(name, "source", source, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    kps = _keypoints_checked(name, kp_driving, kp_source)
    if source.shape[0] not in (1, kps[0].shape[0]):
        raise ValueError(f"{name}: source is {tuple(source.shape)} for keypoints of batch {kps[0].shape[0]}: expected that batch, or 1")
    return generator_warp(appearance_feature(source, weights), kp_driving, kp_source, weights)


__all__ = ["KPDetector", "HEEstimator", "PreparedKPDetector", "PreparedHEEstimator", "NUM_BINS", "antialias_kernel", "kp_detector_structure", "kp_volume_size",
           "kp_detector_structure_shapes", "he_estimator_structure_shapes", "kp_detector_state_dict_shapes", "he_estimator_state_dict_shapes", "prep_conv3d",
           "conv3d_sb3", "heatmap_keypoints", "antialias_down", "avgpool2x2", "kp_detector_forward", "he_estimator_forward", "keypoint_transformation",
           "headpose_degrees", "rotation_matrix", "reenact_keypoints", "DenseMotionNetwork", "PreparedDenseMotion", "dense_motion_structure",
           "dense_motion_structure_shapes", "dense_motion_state_dict_shapes", "prep_conv3d_k7", "conv3d_k7", "motion_input", "motion_combine",
           "dense_motion_forward", "OcclusionAwareSPADEGenerator", "SPADEDecoder", "PreparedGeneratorFront", "LEAKY_SLOPE", "DENSE_MOTION_PARAMS",
           "generator_structure", "generator_structure_shapes", "generator_front_structure_shapes", "generator_state_dict_shapes",
           "spade_decoder_state_dict_shapes", "generator_structure_of_keys", "bn_relu", "occlude", "deform_feature", "appearance_feature", "generator_warp",
           "generator_front_forward"]
