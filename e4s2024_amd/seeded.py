"""Deterministic weights / inputs for parity work.

No checkpoint of the reference exists in this environment (reference
``.gitignore:2-4`` excludes ``pretrained/``), so every parity test, the bench and
the golden fixtures are driven by *seeds*: the same ``(seed, key, shape)`` gives
the same fp32 tensor in the container that generated the fixtures and on the GPU
box.  ``numpy.random.RandomState`` (the legacy MT19937 stream) is frozen across
numpy versions, which is why it is used instead of ``torch.manual_seed``.

The distributions follow the reference constructors where they matter
(``models/stylegan2/model.py:103-105, 141, 227-231, 342`` use ``randn``;
modulation bias is initialised to 1, ``:231``) and are otherwise chosen to look
like a trained network (non-zero biases, positive BatchNorm variances) so that no
code path is silently multiplied by zero.
"""
from __future__ import annotations

import re
import zlib
from typing import Dict, Iterable, Mapping, Tuple

import numpy as np
import torch

__all__ = [
    "seeded_array",
    "seeded_lpips_state_dict",
    "seeded_irse50_state_dict",
    "seeded_unet_state_dict",
    "seeded_resunet_state_dict",
    "seeded_fpn_state_dict",
    "seeded_small_fpn_state_dict",
    "seeded_rrdbnet_state_dict",
    "seeded_gpen_sr_state_dict",
    "seeded_gpen_state_dict",
    "seeded_parsenet_state_dict",
    "seeded_retinaface_state_dict",
    "seeded_kp_detector_state_dict",
    "seeded_he_estimator_state_dict",
    "seeded_dense_motion_state_dict",
    "seeded_generator_state_dict",
    "seeded_codeformer_state_dict",
    "seeded_inpaint_state_dict",
    "seeded_state_dict",
    "apply_seeded",
    "blocky_labels",
    "iid_labels",
    "labels_to_onehot",
    "seeded_codes",
    "seeded_latent_avg",
    "seeded_image",
]


def _rs(seed: int, key: str) -> np.random.RandomState:
    return np.random.RandomState((zlib.crc32(key.encode("utf-8")) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)


_SQRT3 = float(np.sqrt(3.0))


def seeded_array(seed: int, key: str, shape, mean: float = 0.0, std: float = 1.0, dist: str = "uniform") -> np.ndarray:
    """fp32 array with the given mean/std that depends only on (seed, key, shape).

    ``dist="uniform"`` (default, used for weights: 164 M of them must be regenerated on
    the GPU box in well under a second per 10 M) draws uint32 words from the legacy
    stream and maps them to U(-sqrt3, sqrt3)·std + mean; ``dist="normal"`` uses the
    legacy ``standard_normal`` (used for inputs: codes, noise maps, images)."""
    n = int(np.prod(shape)) if len(shape) else 1
    rs = _rs(seed, key)
    if dist == "normal":
        a = rs.standard_normal(n).astype(np.float32)
    else:
        u = rs.randint(0, 2 ** 32, size=n, dtype=np.uint32)
        a = u.astype(np.float32)
        a *= np.float32(2.0 * _SQRT3 / 4294967296.0)
        a -= np.float32(_SQRT3)
    if std != 1.0:
        a *= np.float32(std)
    if mean != 0.0:
        a += np.float32(mean)
    return a.reshape(tuple(shape))


# (regex, rule) — first match wins.  rule = (mean, std) | callable(seed, key, shape)
def _fan_in_std(gain: float):
    def rule(seed, key, shape):
        fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else int(shape[0])
        return seeded_array(seed, key, shape, 0.0, gain / np.sqrt(max(fan_in, 1)))
    return rule


def _positive(mean: float, std: float):
    def rule(seed, key, shape):
        return np.abs(seeded_array(seed, key, shape, 0.0, std)) + np.float32(mean)
    return rule


def _const_kernel(seed, key, shape):
    # Blur / Upsample FIR buffers are constants of the architecture
    # (models/stylegan2/model.py:23-31, 39, 82-87): outer([1,3,3,1]) / 64 * 4.
    k = np.array([1.0, 3.0, 3.0, 1.0], dtype=np.float32)
    k2 = np.outer(k, k)
    k2 = k2 / k2.sum() * 4.0
    assert tuple(shape) == (4, 4), shape
    return k2.astype(np.float32)


_RULES_NET3 = [
    (r"\.blur\.kernel$|\.upsample\.kernel$", _const_kernel),
    (r"^G\.noises\.", (0.0, 1.0, "normal")),
    (r"^G\.input\.input$", (0.0, 1.0)),
    (r"\.modulation\.weight$", (0.0, 1.0)),
    (r"\.modulation\.bias$", (1.0, 0.1)),
    (r"\.noise\.weight$", (0.0, 0.1)),
    (r"\.activate\.bias$", (0.0, 0.1)),
    (r"^G\.to_rgb.*\.bias$", (0.0, 0.1)),
    (r"^G\.style\.\d+\.weight$", (0.0, 100.0)),   # randn / lr_mul, lr_mul = 0.01 (model.py:141)
    (r"^G\.style\.\d+\.bias$", (0.0, 0.1)),
    (r"^G\..*conv\.weight$", (0.0, 1.0)),
    (r"^MLPs\.\d+\.mlp\.\d+\.weight$", (0.0, 1.0)),
    (r"^MLPs\.\d+\.mlp\.\d+\.bias$", (0.0, 0.1)),
    # encoder: PReLU slopes (res_layer.2 / input_layer.2) are 1-D, convs are 4-D
    (r"^encoder\..*\.weight$", None),  # resolved by ndim below
]

_RULES_BISENET = [
    (r"num_batches_tracked$", "zero_long"),
    (r"running_var$", _positive(0.5, 0.5)),
    (r"running_mean$", (0.0, 0.2)),
    (r"\.bn\d*\.weight$|\.bn\.weight$|bn_atten\.weight$|downsample\.1\.weight$", _positive(0.8, 0.3)),
    (r"\.bn\d*\.bias$|\.bn\.bias$|bn_atten\.bias$|downsample\.1\.bias$", (0.0, 0.2)),
    (r"\.weight$", _fan_in_std(1.4)),
]


# LPIPS-AlexNet (criteria/lpips): He-scaled convolutions, small positive biases (most units stay alive), non-negative lin weights like the trained
# ones; mean / std are the reference's fixed buffers (networks.py:47-51)
_RULES_LPIPS = [
    (r"^net\.mean$", lambda seed, key, shape: np.array([-.030, -.088, -.188], dtype=np.float32).reshape(shape)),
    (r"^net\.std$", lambda seed, key, shape: np.array([.458, .448, .450], dtype=np.float32).reshape(shape)),
    (r"^net\.layers\.\d+\.weight$", _fan_in_std(1.4)),
    (r"^net\.layers\.\d+\.bias$", (0.05, 0.05)),
    (r"^lin\.\d+\.1\.weight$", _positive(0.0, 0.2)),
]


def seeded_lpips_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for the drop-in ``criteria.lpips.LPIPS`` (its 17-key state_dict)."""
    shapes = {"net.mean": (1, 3, 1, 1), "net.std": (1, 3, 1, 1)}
    chans = [3, 64, 192, 384, 256, 256]
    for i, (li, k) in enumerate(zip((0, 3, 6, 8, 10), (11, 5, 3, 3, 3))):
        shapes[f"net.layers.{li}.weight"] = (chans[i + 1], chans[i], k, k)
        shapes[f"net.layers.{li}.bias"] = (chans[i + 1],)
    for i in range(5):
        shapes[f"lin.{i}.1.weight"] = (1, chans[i + 1], 1, 1)
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in shapes.items()}, seed, "lpips")


# ArcFace IR-SE50 (models/encoders/model_irse.py::Backbone(112, 50, 'ir_se')): fan-in scaled convolutions / linear, the residual branch's last
# convolution at a smaller gain so that 24 residual additions keep the activations O(1); eval BatchNorm statistics around the identity
_RULES_IRSE50 = [
    (r"num_batches_tracked$", "zero_long"),
    (r"running_var$", (1.0, 1.0 / np.sqrt(12.0))),                    # U(0.5, 1.5)
    (r"running_mean$", (0.0, 0.1)),
    (r"(input_layer\.1|output_layer\.[04]|res_layer\.[04]|shortcut_layer\.1)\.weight$", (1.0, 0.1)),
    (r"(input_layer\.1|output_layer\.[034]|res_layer\.[04]|shortcut_layer\.1)\.bias$", (0.0, 0.1)),
    (r"(input_layer\.2|res_layer\.2)\.weight$", (0.25, 0.05)),          # PReLU slopes
    (r"res_layer\.3\.weight$", _fan_in_std(0.5)),
    (r"\.fc[12]\.weight$", _fan_in_std(1.0)),
    (r"\.weight$", _fan_in_std(1.0)),
]


def seeded_irse50_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``Backbone(112, 50, 'ir_se')`` (the ArcFace net of criteria/id_loss.py; its 397-key state_dict)."""
    from .ops_id import state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in state_dict_shapes().items()}, seed, "irse50")


# face-parsing unet (criteria/face_parsing/unet.py::unet(feature_scale=4)): He-scaled convolutions (ReLU keeps about half of each layer alive, so
# the tap RMS stays O(1) through the ten conv + BN + ReLU layers), small conv biases, eval BatchNorm statistics around the identity
_RULES_UNET = [
    (r"num_batches_tracked$", "zero_long"),
    (r"running_var$", (1.0, 1.0 / np.sqrt(12.0))),                    # U(0.5, 1.5)
    (r"running_mean$", (0.0, 0.1)),
    (r"\.conv[12]\.1\.weight$", (1.0, 0.1)),                         # BatchNorm gamma
    (r"\.conv[12]\.1\.bias$", (0.0, 0.1)),                           # BatchNorm beta
    (r"\.bias$", (0.0, 0.05)),                                        # convolution / transposed convolution biases
    (r"\.weight$", _fan_in_std(1.4)),
]


def seeded_unet_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``unet(feature_scale=4)`` (the face-parsing net of criteria/face_parsing/face_parsing_loss.py; its 136-key state_dict)."""
    from .ops_fp import state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in state_dict_shapes().items()}, seed, "unet")


# Res-U-Net of the recolouring network (swap_face_fine/Blender/model_center/res_u_net.py): fan-in scaled convolutions; eval BatchNorm values chosen to
# catch a wrong fold — gamma over +-1.5 with one channel per layer exactly 0 and about half negative (a pre-activation written as (x - m) * s divides by
# zero there), beta and running_mean over +-0.5, running_var over [0.5, 2]; the head convolution at a gain that spreads the sigmoid's output over (0, 1)
# (at the default initialisation every output sits at 0.5 +- 0.04)
RESUNET_HEAD_GAIN = 2.0


def _gamma_with_a_zero(seed, key, shape):
    a = seeded_array(seed, key, shape, 0.0, 1.5 / _SQRT3)
    a[_rs(seed, key + "#zero").randint(shape[0])] = 0.0
    return a


_RULES_RESUNET = [
    (r"num_batches_tracked$", "zero_long"),
    (r"running_var$", (1.25, 0.75 / _SQRT3)),                         # U(0.5, 2)
    (r"running_mean$", (0.0, 0.5 / _SQRT3)),                          # U(-0.5, 0.5)
    (r"\.bn[12]\.weight$", _gamma_with_a_zero),
    (r"\.bn[12]\.bias$", (0.0, 0.5 / _SQRT3)),
    (r"\.bias$", (0.0, 0.1)),                                         # convolution biases
    (r"^output_decoder_layer\.0\.weight$", _fan_in_std(RESUNET_HEAD_GAIN)),
    (r"\.weight$", _fan_in_std(1.0)),
]


def seeded_resunet_state_dict(seed: int, width: int = 64) -> Dict[str, torch.Tensor]:
    """Seed-only weights for the recolouring ``ResUNet`` (``ops.ResUNet(width)``: the reference's keys; width 64, or 16 for ``small_FPN``)."""
    from .ops_recolor import resunet_state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in resunet_state_dict_shapes(width).items()}, seed, "resunet")


# Feature network of the recolouring network (swap_face_fine/Blender/model_center/backbone.py).  A spectral-normalised convolution stores weight_orig and the
# vectors u, v of the power iteration; in eval mode the weight is weight_orig / sigma with sigma = u . W v.  u and v are unit vectors; for random u, v and a
# random W that product is a small number of either sign, so weight_orig is a fan-in scaled matrix W0 moved along u v^T until u . W v is FPN_SIGMA exactly
# (in float64): what a trained layer looks like, a leading singular component of that size on top of the bulk.  FPN_SIGMA is not 1, so that a sigma left out
# shows.  The SPADE first layers get He scale (a ReLU follows), biases are large enough to matter.
FPN_SIGMA = 1.25


def _unit_vector(seed, key, shape):
    a = seeded_array(seed, key, shape, dist="normal").astype(np.float64)
    return (a / np.linalg.norm(a)).astype(np.float32)


def _spectral_weight(seed, key, shape):
    base = key[:-len("_orig")]
    w0 = _fan_in_std(1.0)(seed, key, shape).astype(np.float64).reshape(shape[0], -1)
    u = _unit_vector(seed, base + "_u", (w0.shape[0],)).astype(np.float64)
    v = _unit_vector(seed, base + "_v", (w0.shape[1],)).astype(np.float64)
    w = w0 + (FPN_SIGMA - u @ w0 @ v) / ((u @ u) * (v @ v)) * np.outer(u, v)
    return w.reshape(shape).astype(np.float32)


_RULES_FPN = [
    (r"\.weight_orig$", _spectral_weight),
    (r"\.weight_[uv]$", _unit_vector),
    (r"\.mlp_shared\.1\.weight$", _fan_in_std(1.4)),
    (r"\.bias$", (0.0, 0.2)),
    (r"\.weight$", _fan_in_std(1.0)),
]


def seeded_fpn_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for the recolouring feature network (``ops.BlenderFPN()``: the reference's ``AdaptiveFeatureGenerator`` keys at its default
    arguments); every spectral-normalised convolution has unit ``weight_u`` / ``weight_v`` and ``sigma = FPN_SIGMA``."""
    from .ops_recolor import fpn_state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in fpn_state_dict_shapes(False).items()}, seed, "fpn")


def seeded_small_fpn_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``ops.SmallFPN()`` (the reference's ``SmallFPN`` keys)."""
    from .ops_recolor import fpn_state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in fpn_state_dict_shapes(True).items()}, seed, "fpn")


# RRDBNet of the Real-ESRGAN step (basicsr's rrdbnet_arch, 351 convolutions): normal weights at a gain of 0.7 over the fan-in and biases over +-0.1.  With 23
# blocks that keeps the body's activations below about a hundred and the output alive: at a gain of 1 nearly every output pixel saturates behind the
# wrappers' clamps, and basicsr's own 0.1-scaled initialisation gives a flat image.  A test rescales conv_last to its case (tests/rrdb_model.py).
RRDB_GAIN = 0.7


def _rrdb_weight(seed, key, shape):
    return seeded_array(seed, key, shape, 0.0, RRDB_GAIN / np.sqrt(int(np.prod(shape[1:]))), dist="normal")


_RULES_RRDB = [
    (r"\.bias$", (0.0, 0.1 / _SQRT3)),                                # U(-0.1, 0.1)
    (r"\.weight$", _rrdb_weight),
]


def seeded_rrdbnet_state_dict(seed: int, num_block: int = 23) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``ops.RRDBNet(num_block)`` (the keys of ``RealESRGAN_x4plus.pth``'s ``params_ema``)."""
    from .ops_recolor import rrdbnet_state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in rrdbnet_state_dict_shapes(num_block).items()}, seed, "rrdb")


def seeded_gpen_sr_state_dict(seed: int, num_block: int = 23, num_feat: int = 32, scale: int = 2) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``ops.GpenSRNet(num_block, num_feat, scale)`` (the keys of a ``realesrnet_x2.pth``'s ``params_ema``), in
    ``seeded_rrdbnet_state_dict``'s distribution."""
    from .ops_gpen_sr import gpen_sr_state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in gpen_sr_state_dict_shapes(num_block, num_feat, scale).items()}, seed, "rrdb")


# GPEN's generator (swap_face_fine/gpen/face_model/gpen_model.py FullGenerator): the equalised-lr layers scale themselves, so weights are unit-variance (the
# style MLP's are randn / lr_mul with lr_mul = 0.01).  noise.weight, every activation bias and every ToRGB bias are zero in the reference's initialisation; here
# they are NOT: a zero noise weight hides the whole concatenated half of every StyledConv.  GPEN_RGB_GAIN scales the ToRGB weights so that the sum of the skip
# chain stays in the image range (output standard deviation 0.3 - 0.5, at most 5 % of the values outside (-1, 1), on the tests' cases).
GPEN_RGB_GAIN = 0.35


def _fir_kernel(gain):
    def rule(seed, key, shape):
        assert tuple(shape) == (4, 4), shape
        k = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0])
        return (k / k.sum() * gain).astype(np.float32)
    return rule


def _gpen_noise_weight(seed, key, shape):
    a = seeded_array(seed, key, shape, 0.0, 0.3)
    return np.where(a < 0, a - np.float32(0.3), a + np.float32(0.3))          # magnitude in [0.3, 0.82), either sign


_RULES_GPEN = [
    (r"^ecd\d+\.0\.0\.kernel$", _fir_kernel(1.0)),
    (r"\.blur\.kernel$|\.upsample\.kernel$", _fir_kernel(4.0)),
    (r"\.noise\.weight$", _gpen_noise_weight),
    (r"\.activate\.bias$|^ecd\d+\.0\.\d\.bias$|^final_linear\.0\.bias$", (0.0, 0.1)),
    (r"\.modulation\.bias$", (1.0, 0.1)),
    (r"\.modulation\.weight$", (0.0, 1.0)),
    (r"^generator\.style\.\d+\.weight$", (0.0, 100.0)),
    (r"^generator\.style\.\d+\.bias$", (0.0, 10.0)),                          # times lr_mul: +-0.17
    (r"^generator\.to_rgb.*\.conv\.weight$", (0.0, GPEN_RGB_GAIN)),
    (r"^generator\.to_rgb.*\.bias$", (0.0, 0.05)),
    (r"\.weight$|^generator\.input\.input$", (0.0, 1.0)),
]


def seeded_gpen_state_dict(seed: int, size: int = 512, style_dim: int = 512, n_mlp: int = 8, channel_multiplier: int = 2, narrow: float = 1) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``ops.GPEN(size, style_dim, n_mlp, channel_multiplier, narrow)`` (the keys of ``GPEN-BFR-512.pth`` at the default)."""
    from .ops_gpen import gpen_state_dict_shapes
    shapes = gpen_state_dict_shapes(size, style_dim, n_mlp, channel_multiplier, narrow)
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in shapes.items()}, seed, "gpen")


# GPEN's ParseNet (swap_face_fine/gpen/face_parse/parse_model.py): fan-in-scaled convolutions; BatchNorm scales over +-1.5, about half of them negative
# and one per layer exactly zero (a fold that took |gamma|, or divided by it, shows), running statistics and biases away from the identity.  A residual
# block's second convolution has the smaller gain PARSENET_RES_GAIN, so that the sum over the blocks keeps the activations O(1) through the depth, and
# PARSENET_MASK_GAIN puts the standard deviation of the 19 logits between 1 and 10 on the tests' cases (tests/parsenet_model.py checks both): logits in the
# hundreds would widen every bar.
PARSENET_RES_GAIN = 0.7
PARSENET_MASK_GAIN = 2.0


def _parsenet_bn_scale(seed, key, shape):
    a = seeded_array(seed, key, shape, 0.0, 1.5 / _SQRT3)                       # U(-1.5, 1.5)
    a[zlib.crc32(key.encode("utf-8")) % a.size] = 0.0
    return a


_RULES_PARSENET = [
    (r"num_batches_tracked$", "zero_long"),
    (r"running_var$", (1.0, 0.5 / _SQRT3)),                                     # U(0.5, 1.5)
    (r"running_mean$", (0.0, 0.2)),
    (r"\.norm\.norm\.weight$", _parsenet_bn_scale),
    (r"\.norm\.norm\.bias$", (0.0, 0.2)),
    (r"\.conv2d\.bias$", (0.0, 0.1)),
    (r"\.conv2\.conv2d\.weight$", _fan_in_std(PARSENET_RES_GAIN)),
    (r"^out_mask_conv\.conv2d\.weight$", _fan_in_std(PARSENET_MASK_GAIN)),
    (r"\.conv2d\.weight$", _fan_in_std(1.0)),
]


def seeded_parsenet_state_dict(template: Mapping[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for a network with the keys of GPEN's ``ParseNet``: ``template`` is its ``state_dict()`` (meta tensors will do; ``ops.ParseNet(...)``
    or the reference's class give the same keys), ``num_batches_tracked`` included."""
    return seeded_state_dict(template, seed, "parsenet")


# GPEN's RetinaFace detector (swap_face_fine/gpen/face_detect/facemodels/retinaface.py, cfg_re50): He-scaled convolutions (gain sqrt 2 in front of the ReLUs;
# body.conv1 a hundred times smaller, its input being pixels minus a mean); BatchNorm scales of magnitude 0.5 .. 1.5 and either sign — none near zero, so every
# channel and every Bottleneck's residual branch stays alive — running variances over 0.5 .. 1.5 and running means and biases away from zero, so that a fold that
# drops the mean, the bias or the square root shows.  A Bottleneck's last BatchNorm has half that magnitude, which keeps the sum over a stage's blocks O(1).
# The head gains put 5 % .. 40 % of the anchors above the 0.9 score, spread the candidates' scores, and make neighbouring boxes overlap enough for NMS to
# remove at least a fifth of them (tests/golden/make_golden_retinaface.py asserts the conditions on the tests' cases).
RETINA_CONV1_GAIN = 0.014
RETINA_CLASS_GAIN = 0.07
RETINA_BBOX_GAIN = 0.03
RETINA_LANDMARK_GAIN = 0.05


def _retina_bn_scale(mag):
    def rule(seed, key, shape):
        a = seeded_array(seed, key, shape, 0.0, 1.0 / _SQRT3)                   # U(-1, 1)
        return (np.sign(a) + (a == 0)) * (np.float32(0.5) + np.abs(a)) * np.float32(mag)
    return rule


_RULES_RETINAFACE = [
    (r"num_batches_tracked$", "zero_long"),
    (r"running_var$", (1.0, 0.5 / _SQRT3)),                                     # U(0.5, 1.5)
    (r"running_mean$", (0.0, 0.2)),
    (r"\.bn3\.weight$", _retina_bn_scale(0.5)),
    (r"\.bn\d\.weight$|\.downsample\.1\.weight$|^(fpn|ssh\d)\.\w+\.1\.weight$", _retina_bn_scale(1.0)),
    (r"\.bn\d\.bias$|\.downsample\.1\.bias$|^(fpn|ssh\d)\.\w+\.1\.bias$", (0.0, 0.2)),
    (r"conv1x1\.bias$", (0.0, 0.1)),
    (r"^body\.conv1\.weight$", _fan_in_std(RETINA_CONV1_GAIN)),
    (r"^ClassHead\.\d\.conv1x1\.weight$", _fan_in_std(RETINA_CLASS_GAIN)),
    (r"^BboxHead\.\d\.conv1x1\.weight$", _fan_in_std(RETINA_BBOX_GAIN)),
    (r"^LandmarkHead\.\d\.conv1x1\.weight$", _fan_in_std(RETINA_LANDMARK_GAIN)),
    (r"\.weight$", _fan_in_std(1.4)),
]


def seeded_retinaface_state_dict(seed: int, out_channel: int = 256) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``ops.RetinaFace`` at ``cfg_re50`` with that ``out_channel`` (the keys of ``RetinaFace-R50.pth`` at the default)."""
    from .ops_retinaface import retinaface_state_dict_shapes
    shapes = retinaface_state_dict_shapes(out_channel)
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in shapes.items()}, seed, "retinaface")


# face-vid2vid's KPDetector and HEEstimator (swap_face_fine/face_vid2vid/modules/keypoint_detector.py): He-scaled convolutions in front of the ReLUs; BatchNorm
# scales over -1.5 .. 1.5 with one exact zero per layer (a dead channel), running variances over 0.5 .. 1.5, and running means and biases away from zero, so that
# a fold that drops the mean, a bias or the square root shows.  A ResBottleneck's last BatchNorm has half that magnitude, which keeps the sum over a stage's blocks
# O(1).  ``down.weight`` is the architecture's constant Gaussian.  The ``kp`` head's gain is chosen so that every heatmap of the tests' cases has an effective
# support 1 / sum p^2 between 8 positions and a quarter of its volume, neither a one-hot nor uniform (the logits are far from Gaussian: divided by the temperature
# 0.1 a keypoint's have a standard deviation of 2 to 10, most of it in a few broad bumps).  The pose heads' gain spreads each 66-bin softmax over a handful of bins and the degrees over tens of degrees (tests/golden/make_golden_vid2vid_kp.py asserts the
# conditions on the tests' cases).
V2V_KP_HEAD_GAIN = 1.5
V2V_JACOBIAN_GAIN = 1.0
V2V_POSE_GAIN = 1.2


def _v2v_bn_scale(mag):
    def rule(seed, key, shape):
        a = seeded_array(seed, key, shape, 0.0, 1.5 * mag / _SQRT3)             # U(-1.5, 1.5) * mag
        a[zlib.crc32(key.encode("utf-8")) % a.size] = 0.0
        return a
    return rule


def _v2v_antialias(seed, key, shape):
    from .ops_reenact import antialias_kernel
    s = (shape[-1] + 3) // 4                                                    # k = 4 s - 3 (AntiAliasInterpolation2d at scale 1 / s)
    k = antialias_kernel(1.0 / s).numpy()
    assert k.shape == tuple(shape[2:]), (k.shape, shape)
    return np.broadcast_to(k, shape).copy()


_RULES_V2V_KP = [
    (r"num_batches_tracked$", "zero_long"),
    (r"^down\.weight$", _v2v_antialias),
    (r"running_var$", (1.0, 0.5 / _SQRT3)),                                     # U(0.5, 1.5)
    (r"running_mean$", (0.0, 0.2)),
    (r"\.norm3\.weight$", _v2v_bn_scale(0.5)),
    (r"(^|\.)norm\d?\.weight$", _v2v_bn_scale(1.0)),
    (r"(^|\.)norm\d?\.bias$", (0.0, 0.2)),
    (r"\.bias$", (0.0, 0.1)),
    (r"^kp\.weight$", _fan_in_std(V2V_KP_HEAD_GAIN)),
    (r"^jacobian\.weight$", _fan_in_std(V2V_JACOBIAN_GAIN)),
    (r"^fc_(roll|pitch|yaw)\.weight$", _fan_in_std(V2V_POSE_GAIN)),
    (r"^fc_(t|exp)\.weight$", _fan_in_std(1.0)),
    (r"\.weight$", _fan_in_std(1.4)),
]


def seeded_kp_detector_state_dict(template: Mapping[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for a network with the keys of face-vid2vid's ``KPDetector``: ``template`` is its ``state_dict()`` (meta tensors will do;
    ``ops.KPDetector(...)`` or the reference's class give the same keys), ``num_batches_tracked`` and the buffer ``down.weight`` included."""
    return seeded_state_dict(template, seed, "v2v_kp")


def seeded_he_estimator_state_dict(template: Mapping[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for a network with the keys of face-vid2vid's ``HEEstimator`` (``template`` as above)."""
    return seeded_state_dict(template, seed, "v2v_kp")


# face-vid2vid's DenseMotionNetwork (modules/dense_motion.py): the rules above for the hourglass, ``compress`` and the BatchNorms.  The ``mask`` head's gain is
# chosen so that the softmax over the num_kp + 1 motions is neither one-hot nor uniform on the tests' cases (the mean effective count 1 / sum_k mask_k^2 between
# 1.5 and (num_kp + 1) / 2), the ``occlusion`` head's so that its sigmoid spans at least 0.2 .. 0.8 (tests/golden/make_golden_vid2vid_motion.py asserts both).
V2V_MASK_HEAD_GAIN = 18.0
V2V_OCCLUSION_GAIN = 12.0

_RULES_V2V_DM = [
    (r"^mask\.weight$", _fan_in_std(V2V_MASK_HEAD_GAIN)),
    (r"^occlusion\.weight$", _fan_in_std(V2V_OCCLUSION_GAIN)),
] + _RULES_V2V_KP


def seeded_dense_motion_state_dict(template: Mapping[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for a network with the keys of face-vid2vid's ``DenseMotionNetwork``: ``template`` is its ``state_dict()`` (meta tensors will do;
    ``ops.DenseMotionNetwork(...)`` or the reference's class give the same keys)."""
    return seeded_state_dict(template, seed, "v2v_dm")


# face-vid2vid's OcclusionAwareSPADEGenerator (modules/generator.py).  The front (first, down_blocks, second, resblocks_3d, third, fourth) follows the rules above:
# BatchNorm scales of either sign with one exact zero per layer, statistics off the identity, biases away from zero.  The decoder's SPADE blocks follow the
# recolouring feature network's rules (a fan-in scaled bulk plus a leading component of size FPN_SIGMA along weight_v), except that ``weight_u`` is not drawn but
# set to normalize(W v): then sigma = u . W v = |W v| is a norm, about FPN_SIGMA, and never near zero.
_RULES_V2V_GEN = [
    (r"^decoder\..*\.weight_orig$", _spectral_weight),
    (r"^decoder\..*\.weight_[uv]$", _unit_vector),
    (r"^decoder\..*\.mlp_shared\.0\.weight$", _fan_in_std(1.4)),
    (r"^decoder\..*\.bias$", (0.0, 0.2)),
    (r"^decoder\..*\.weight$", _fan_in_std(1.0)),
    (r"^fourth\.weight$", _fan_in_std(1.0)),
] + _RULES_V2V_KP


def seeded_generator_state_dict(template: Mapping[str, torch.Tensor], seed: int) -> Dict[str, torch.Tensor]:
    """Seed-only weights for a network with the keys of face-vid2vid's ``OcclusionAwareSPADEGenerator``, or any part of them (``template``: its
    ``state_dict()``, meta tensors will do; the ``decoder.`` keys may be left out).  The ``dense_motion_network.`` keys get what
    ``seeded_dense_motion_state_dict`` gives the bare keys with the same seed."""
    dm = "dense_motion_network."
    inner = seeded_dense_motion_state_dict({k[len(dm):]: v for k, v in template.items() if k.startswith(dm)}, seed)
    rest = seeded_state_dict({k: v for k, v in template.items() if not k.startswith(dm)}, seed, "v2v_gen")
    out = {k: (inner[k[len(dm):]] if k.startswith(dm) else rest[k]) for k in template}
    for k in out:
        if k.endswith(".weight_u"):
            w, v = out[k[:-2] + "_orig"].double(), out[k[:-2] + "_v"].double()
            u = w.reshape(w.shape[0], -1) @ v
            out[k] = (u / u.norm()).float()
    return out


# CodeFormer (swap_face_fine/archs/codeformer_arch.py, vqgan_arch.py): every convolution and linear fan-in scaled in front of a GroupNorm or on a pre-LayerNorm
# residual stream, so activations stay O(1) through the encoder's 32 GroupNorms and the 9 transformer layers; norm gains around 1, biases away from zero.  ``position_emb`` is
# large enough to matter beside norm1's unit-variance output.  The reference's own initialisation of ``idx_pred_layer.1.weight`` (0.02) and of the codebook
# (1 / 1024) would leave every logit and every code vector near zero: the head's gain spreads a token's logits over several units, so that top-1 and top-2 lie
# more than 64 float32 errors apart on all but a few tokens, and the codebook has unit variance, so that the AdaIN has something to normalise
# (tests/golden/make_golden_codeformer.py asserts both conditions on the codes).  A fuse block's ``scale`` is linear in the decoder stream (through
# ``encode_enc.conv_out``), so ``dec * scale`` is quadratic in it: under the generic rules the stream's deviation went 3, 10, 109, 2e4, 8e8 through the four
# blocks.  The last convolutions of ``scale`` and ``shift`` alone are drawn at a tenth of the generic gain: the stream then grows by at most 1.3 per block while
# the fused term stays a quarter to four fifths of it (tests/golden/make_golden_codeformer_gen.py asserts both).  No other key's bytes change.
CF_SFT_GAIN = 0.1
CF_HEAD_GAIN = 4.0
CF_CODEBOOK_STD = 1.0
CF_POS_STD = 0.5


def _cf_weight(gain: float):
    def rule(seed, key, shape):
        if len(shape) == 1:                                     # a GroupNorm / LayerNorm gain
            return seeded_array(seed, key, shape, 1.0, 0.2)
        return _fan_in_std(gain)(seed, key, shape)
    return rule


_RULES_CODEFORMER = [
    (r"^fuse_convs_dict\.\d+\.(scale|shift)\.2\.weight$", _fan_in_std(1.2 * CF_SFT_GAIN)),
    (r"^fuse_convs_dict\.\d+\.(scale|shift)\.2\.bias$", (0.0, 0.1 * CF_SFT_GAIN)),
    (r"^position_emb$", (0.0, CF_POS_STD)),
    (r"^quantize\.embedding\.weight$", (0.0, CF_CODEBOOK_STD)),
    (r"^idx_pred_layer\.1\.weight$", _fan_in_std(CF_HEAD_GAIN)),
    (r"in_proj_weight$", _fan_in_std(1.0)),
    (r"bias$", (0.0, 0.1)),
    (r"weight$", _cf_weight(1.2)),
]


def seeded_codeformer_state_dict(seed: int, dim_embd: int = 512, n_head: int = 8, n_layers: int = 9, codebook_size: int = 1024, latent_size: int = 256,
                                 connect_list=("32", "64", "128", "256")) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``CodeFormer`` (``ops.CodeFormer`` and the reference's class have the same keys) at the given configuration."""
    from .ops_codeformer import codeformer_state_dict_shapes
    shapes = codeformer_state_dict_shapes(dim_embd, n_head, n_layers, codebook_size, latent_size, tuple(connect_list))
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in shapes.items()}, seed, "codeformer")


# The GCFSR inpainting generator (swap_face_fine/gcfsr_arch.py FaceInpaintingArch; ``ops.FaceInpainting`` has its keys): equalised-lr layers, so unit-variance
# weights.  The reference initialises the noise-injection weights, every bias and the shift convolutions' biases to zero and the condition linears' biases to one;
# here the noise weights, both condition linears (weight: magnitude 0.3 - 0.82, either sign; bias: 0.24 - 0.76) and the shift convolutions' biases (magnitude 0.3 -
# 0.82) are set well away from 0 and 1: a dropped noise term, a swapped scale or a missing bias then shows in the output.  The stored ``noises.noise{i}`` buffers
# (never read by either side) are normal draws.  The ToRGB biases sum to about 0.5 along the skip chain and INPAINT_RGB_GAIN scales the ToRGB weights so that
# the output straddles [0, 1]: at least half of the values inside a hole lie strictly inside (0, 1) on the tests' cases (tests/golden/make_golden_inpaint.py
# asserts it and records the shares), so that the caller's clamp does not hide the network.
INPAINT_RGB_GAIN = 0.12

_RULES_INPAINT = [
    (r"^noises\.noise\d+$", (0.0, 1.0, "normal")),
    (r"^style_conv(1|s\.\d+)\.weight$", _gpen_noise_weight),
    (r"^condition_scale[12]\.\d+\.weight$", _gpen_noise_weight),
    (r"^condition_scale[12]\.\d+\.bias$", (0.5, 0.15)),
    (r"^condition_shift\.\d+\.0\.bias$", _gpen_noise_weight),
    (r"\.modulation\.bias$", (1.0, 0.1)),
    (r"\.modulation\.weight$", (0.0, 1.0)),
    (r"^to_rgb.*\.modulated_conv\.weight$", (0.0, INPAINT_RGB_GAIN)),
    (r"^to_rgb1\.bias$", (0.5, 0.05)),
    (r"^to_rgbs\.\d+\.bias$", (0.0, 0.05)),
    (r"\.bias$", (0.0, 0.1)),
    (r"\.weight$", (0.0, 1.0)),
]


def seeded_inpaint_state_dict(seed: int, out_size: int = 256) -> Dict[str, torch.Tensor]:
    """Seed-only weights for ``ops.FaceInpainting(out_size)`` (the keys of ``net_g_50000.pth``'s ``params_ema`` at 256)."""
    from .ops_inpaint import inpaint_state_dict_shapes
    return seeded_state_dict({k: torch.empty(v, device="meta") for k, v in inpaint_state_dict_shapes(out_size).items()}, seed, "inpaint")


def _resolve(family: str, seed: int, key: str, shape, dtype) -> torch.Tensor:
    rules = {"net3": _RULES_NET3, "lpips": _RULES_LPIPS, "irse50": _RULES_IRSE50, "unet": _RULES_UNET, "resunet": _RULES_RESUNET,
             "fpn": _RULES_FPN, "rrdb": _RULES_RRDB, "gpen": _RULES_GPEN, "parsenet": _RULES_PARSENET,
             "retinaface": _RULES_RETINAFACE, "v2v_kp": _RULES_V2V_KP, "v2v_dm": _RULES_V2V_DM, "v2v_gen": _RULES_V2V_GEN, "codeformer": _RULES_CODEFORMER,
             "inpaint": _RULES_INPAINT}.get(family, _RULES_BISENET)
    for pat, rule in rules:
        if re.search(pat, key):
            break
    else:
        raise KeyError(f"no seeded rule for {family} key {key!r} shape {tuple(shape)}")
    if rule == "zero_long":
        return torch.zeros(tuple(shape), dtype=torch.long)
    if rule is None:  # encoder weights
        if len(shape) == 1:
            arr = seeded_array(seed, key, shape, 0.25, 0.05)       # PReLU slopes
        else:
            arr = _fan_in_std(1.4)(seed, key, shape)                # conv kernels
    elif callable(rule):
        arr = rule(seed, key, shape)
    else:
        arr = seeded_array(seed, key, shape, *rule)
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(dtype)


def seeded_state_dict(template: Mapping[str, torch.Tensor], seed: int, family: str) -> Dict[str, torch.Tensor]:
    """Build a state_dict with the template's keys/shapes/dtypes and seeded values.

    ``family`` is ``"net3"`` (keys of ``models.networks.Net3`` or any sub-tree of it
    when the caller prefixes keys accordingly) or ``"bisenet"``.
    """
    out = {}
    for key, t in template.items():
        out[key] = _resolve(family, seed, key, tuple(t.shape), t.dtype)
    return out


def apply_seeded(module: torch.nn.Module, seed: int, family: str, prefix: str = "") -> torch.nn.Module:
    """Load seeded values into ``module`` in place.  ``prefix`` is prepended to the
    module's own keys before the rule lookup (e.g. ``"G."`` for a bare Generator)."""
    sd = module.state_dict()
    tmpl = {prefix + k: v for k, v in sd.items()}
    vals = seeded_state_dict(tmpl, seed, family)
    module.load_state_dict({k[len(prefix):]: v for k, v in vals.items()})
    return module


# --------------------------------------------------------------------------- inputs
def blocky_labels(seed: int, bs: int, n_cls: int = 12, size: int = 512, cells: int = 16) -> np.ndarray:
    """uint8 [bs, size, size] label maps made of ``cells``×``cells`` constant blocks
    (the benign case — most GEMM tiles see one region)."""
    small = np.random.RandomState(seed).randint(0, n_cls, (bs, cells, cells)).astype(np.uint8)
    rep = size // cells
    return np.repeat(np.repeat(small, rep, axis=1), rep, axis=2)


def facelike_labels(seed: int, bs: int, size: int = 512) -> np.ndarray:
    """uint8 [bs, size, size] region maps shaped like a parsed portrait (12 classes as in CelebAMask-HQ's merged set: 0 background, 1 lips,
    2 eyebrows, 3 eyes, 4 hair, 5 nose, 6 skin, 7 ears, 8 neck, 9 mouth, 10 eye glasses unused, 11 ear rings): ellipses with a few pixels of
    per-sample jitter — large coherent regions with curved borders, the kind of map the face parser produces on real photographs."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size

    def ell(cx, cy, rx, ry):
        return ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0

    out = np.zeros((bs, size, size), dtype=np.uint8)
    for b in range(bs):
        j = lambda s=0.015: float(rs.uniform(-s, s))          # noqa: E731
        cx, cy = 0.5 + j(), 0.5 + j()
        m = out[b]
        m[ell(cx, cy + 0.42, 0.34, 0.22)] = 8                                   # neck / shoulders
        m[ell(cx, cy - 0.06, 0.36 + j(), 0.44 + j())] = 4                       # hair
        m[ell(cx - 0.30, cy + 0.02, 0.035, 0.07)] = 7; m[ell(cx + 0.30, cy + 0.02, 0.035, 0.07)] = 7   # ears
        m[ell(cx - 0.30, cy + 0.10, 0.012, 0.02)] = 11                          # ear ring
        m[ell(cx, cy + 0.04, 0.27 + j(), 0.36 + j())] = 6                       # skin
        m[ell(cx - 0.11, cy - 0.07, 0.06, 0.012)] = 2; m[ell(cx + 0.11, cy - 0.07, 0.06, 0.012)] = 2   # eyebrows
        m[ell(cx - 0.11, cy - 0.02, 0.045, 0.02)] = 3; m[ell(cx + 0.11, cy - 0.02, 0.045, 0.02)] = 3   # eyes
        m[ell(cx, cy + 0.08, 0.04, 0.07)] = 5                                   # nose
        m[ell(cx, cy + 0.21, 0.085, 0.035)] = 1                                 # lips
        m[ell(cx, cy + 0.21, 0.055, 0.012)] = 9                                 # mouth
    return out


def iid_labels(seed: int, bs: int, n_cls: int = 12, size: int = 512) -> np.ndarray:
    """uint8 [bs, size, size] i.i.d. per-pixel labels — the adversarial case where
    every tile sees all regions."""
    return np.random.RandomState(seed).randint(0, n_cls, (bs, size, size)).astype(np.uint8)


def labels_to_onehot(labels: np.ndarray, n_cls: int = 12) -> torch.Tensor:
    """Same result as the reference's ``labelMap2OneHot`` (utils/torch_utils.py:207-213)
    on a [bs,H,W] uint8 label array: float32 [bs, n_cls, H, W]."""
    lab = torch.from_numpy(labels.astype(np.int64))
    oh = torch.zeros(lab.shape[0], n_cls, lab.shape[1], lab.shape[2], dtype=torch.float32)
    return oh.scatter_(1, lab[:, None], 1.0)


def seeded_latent_avg(seed: int = 2, n_styles: int = 18) -> torch.Tensor:
    return torch.from_numpy(seeded_array(seed, "latent_avg", (n_styles, 512), 0.0, 0.1, "normal"))


def seeded_codes(seed: int, bs: int, n_cls: int = 12, n_styles: int = 18, latent_avg: torch.Tensor | None = None) -> torch.Tensor:
    """W+ codes [bs, n_cls, n_styles, 512] = latent_avg + 0.5·N(0,1)."""
    if latent_avg is None:
        latent_avg = seeded_latent_avg(2, n_styles)
    c = torch.from_numpy(seeded_array(seed, "codes", (bs, n_cls, n_styles, 512), 0.0, 0.5, "normal"))
    return c + latent_avg[None, None]


def seeded_image(seed: int, bs: int, size: int = 1024) -> torch.Tensor:
    """[-1,1] images [bs,3,size,size]: tanh of smooth-ish noise."""
    a = seeded_array(seed, "image", (bs, 3, size, size), 0.0, 1.0, "normal")
    return torch.tanh(torch.from_numpy(a))
