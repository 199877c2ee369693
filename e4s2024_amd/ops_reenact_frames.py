"""Row f20: face-vid2vid reenactment, stage 4 — the ``SPADEDecoder`` of swap_face_fine/face_vid2vid/modules/generator.py:120-158 (``SPADE`` and
``SPADEResnetBlock`` of modules/util.py:421-481) in eval mode on the device, and with it whole frames: ``OcclusionAwareSPADEGenerator.forward`` and
``make_animation`` of drive_demo.py:182-211.  Rows f17 - f19 (``ops_reenact``) end at the decoder's input; this module is the rest.

    label maps     the decoder's input ``feature [n, 256, h, w]`` is also the label map of every SPADE norm: at the base size as it is, for up_0 and up_1 its
                   nearest x2 and x4 (x2 twice) picks on e4s_esr_up2
    fc             3 x 3 with its bias on e4s_conv2d_sb3, as every convolution here (three-way bf16 split, fp32-class)
    mlp_shared     3 x 3 + ReLU; with one sample the 12 / 3 / 3 norms that read one label map run as ONE convolution of 128 N outputs (a channel slice of a batch-1
                   tensor is dense, so the convolution behind it reads it in place); with more samples one launch per norm
    gamma | beta   per norm ONE convolution of 2 C outputs: the layout e4s_v2v_spade_norm reads
    a block        e4s_plane_stats of the block's input, shared by norm_0 and norm_s; e4s_v2v_spade_norm: both modulations from one read of x, the leaky 0.2 of
                   norm_0's consumer applied, the nearest x2 in front of up_0 / up_1 folded into the read (the upsampled x is never formed: a nearest x2 plane has
                   exactly the statistics of the plane it repeats); conv_0; statistics and the modulation of norm_1; conv_1 with the shortcut (x, or conv_s of
                   norm_s) as its residual.  Spectral norm is folded in float64 (``weight_orig / (u . (W_mat v))``, no power iteration)
    image          e4s_v2v_image_head: leaky 0.2, conv_img (exact float32, 64 -> 3) and the sigmoid in one pass

``spade_decoder_forward`` is the decoder alone, ``generator_frames`` the per-frame part of the generator (``generator_warp`` and the decoder),
``generator_forward`` the whole forward, ``NativeSPADEGenerator`` a module around a loaded generator that the reference's own ``make_animation`` drives natively,
and ``make_animation`` that function for device tensors, batched over the frames.  The module ``swap_face_fine.face_vid2vid.modules.generator`` is not redirected
(INTEGRATION.md §4l): the wrapper is the way in.

Forward only; eval mode only; no host synchronisation; no atomics; the same inputs give the same bits; after one eager call (which prepares the weights) a call
captures in a graph."""
from __future__ import annotations

import torch
import torch.nn as nn

from ._lib import lib
from .lossnet import conv_sb, prep_fwd
from .netweights import PreparedNet, _Net, _cuda_checked, _placed_checked, _tensor_checked, _validated, check_loaded, prepare, weights_key
from .ops import _p, _stream
from .ops_recolor import _plane_stats, _sigma_folded
from .ops_reenact import (_generator_checked, _keypoints_checked, appearance_feature, generator_warp, he_estimator_forward, keypoint_transformation,
                          kp_detector_forward, spade_decoder_state_dict_shapes)

DECODER_CHANNELS = 256                       # SPADEDecoder's input and label width, fixed in the reference
SPADE_HIDDEN = 128                           # SPADE's nhidden
MAX_SIDE = 16384
# (block, fin, fout, the nearest x2 in front of it)
_BLOCKS = tuple((f"G_middle_{i}", 512, 512, 1) for i in range(6)) + (("up_0", 512, 256, 2), ("up_1", 256, 64, 2))


def _block_norms(p, fin, fout):
    return (p + ".norm_0", p + ".norm_1") + ((p + ".norm_s",) if fin != fout else ())


# the norms that read the label map at one resolution: 12 at the base size, 3 at x2, 3 at x4
_LEVELS = (tuple(n for p, fin, fout, _ in _BLOCKS[:6] for n in _block_norms(p, fin, fout)), _block_norms(*_BLOCKS[6][:3]), _block_norms(*_BLOCKS[7][:3]))


# ------------------------------------------------------------------------------------------------ weights
_DEC_NET = _Net("SPADEDecoder", spade_decoder_state_dict_shapes, ("generator.decoder.", "module.generator.decoder.", "module.decoder.", "decoder.", "module."),
                False, ("fc.weight",), None, None, ())


def _decoder_checked(name, weights):
    """(weights without the checkpoint's wrapping, what ``_validated`` returns of the decoder's keys).  A module in training mode is refused here: spectral
    norm's power iteration and nothing else of training is offered."""
    check_loaded(name, weights, "the weights")
    if isinstance(weights, nn.Module) and weights.training:
        raise NotImplementedError(f"{name}: {type(weights).__name__} is in training mode; the native decoder is the eval-mode forward (spectral norm without "
                                  "its power iteration): call .eval()")
    if not isinstance(weights, nn.Module) and hasattr(weights, "keys") and isinstance(weights.get("generator"), dict):
        weights = weights["generator"]                      # the checkpoint file as torch.load gives it
    return weights, _validated(name, weights, _DEC_NET)


class PreparedSPADEDecoder(PreparedNet):
    """The kernels' copies of a ``SPADEDecoder``'s weights, rebuilt when a tensor changes version or storage, all as three-way split slabs but ``conv_img``:
    ``fc`` with its bias; per block ``conv_0`` / ``conv_1`` (with bias) and ``conv_s`` with eval-mode spectral norm folded in float64; per norm ``mlp_gamma``
    and ``mlp_beta`` concatenated into one convolution of ``2 C`` outputs and ``mlp_shared`` on its own; per resolution the ``mlp_shared`` convolutions of its
    norms stacked into one of ``128 N`` outputs (what a single sample runs); ``conv_img`` as it is, for ``e4s_v2v_image_head``."""

    __slots__ = ()
    _entry, _net = "spade_decoder_forward", _DEC_NET

    def _build(self, sd, variant, dev):
        blocks, norms = [], {}
        for p, fin, fout, up in _BLOCKS:
            blocks.append(dict(name=p, up=up, conv_0=prep_fwd(_sigma_folded(sd, p + ".conv_0"), None, sd[p + ".conv_0.bias"]),
                               conv_1=prep_fwd(_sigma_folded(sd, p + ".conv_1"), None, sd[p + ".conv_1.bias"]),
                               conv_s=prep_fwd(_sigma_folded(sd, p + ".conv_s")) if fin != fout else None))
            for n in _block_norms(p, fin, fout):
                norms[n] = dict(shared=prep_fwd(sd[n + ".mlp_shared.0.weight"], None, sd[n + ".mlp_shared.0.bias"]),
                                gb=prep_fwd(torch.cat([sd[n + ".mlp_gamma.weight"], sd[n + ".mlp_beta.weight"]]), None,
                                            torch.cat([sd[n + ".mlp_gamma.bias"], sd[n + ".mlp_beta.bias"]])))
        stacked = [prep_fwd(torch.cat([sd[n + ".mlp_shared.0.weight"] for n in level]), None, torch.cat([sd[n + ".mlp_shared.0.bias"] for n in level]))
                   for level in _LEVELS]
        return dict(fc=prep_fwd(sd["fc.weight"], None, sd["fc.bias"]), blocks=blocks, norms=norms, stacked=stacked,
                    img=(sd["conv_img.weight"].contiguous(), sd["conv_img.bias"].contiguous()))


# ------------------------------------------------------------------------------------------------ the two kernels
def _out_checked(name, nm, out, shape, like):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError(f"{name}: {nm}: expected a dense float32 tensor of shape {tuple(shape)}")
    if not out.is_cuda or out.device != like.device:
        raise RuntimeError(f"{name}: {nm} must be a CUDA tensor on the inputs' device")
    return out


def spade_norm(x, stats, gamma_beta, gamma_beta_s=None, up=1, *, out=None, out_s=None):
    """``e4s_v2v_spade_norm``: ``leaky_0.2((up(x) - mean) rstd (1 + gamma) + beta)`` of a float32 ``x [bs, C, h / up, w / up]`` with ``stats = (mean, rstd)``,
    float32 ``[bs C]`` as ``e4s_plane_stats`` gives them for x itself, ``gamma_beta [bs, 2 C, h, w]`` (gamma | beta) and ``up`` 1 or 2, the nearest upsampling
    folded into the read.  With ``gamma_beta_s`` (a second norm of the same x: the ``norm_s`` of a learned shortcut) the result is the pair ``(out, out_s)``,
    ``out_s`` without the activation, both from one read of x.  ``out`` / ``out_s``: dense tensors to write into."""
    name = "spade_norm"
    if out_s is not None and gamma_beta_s is None:
        raise ValueError(f"{name}: out_s without gamma_beta_s")
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, C, h, w] tensor")
    if up not in (1, 2):
        raise ValueError(f"{name}: up is {up!r}: 1, or 2 for the nearest x2 folded into the read")
    bs, C, hl, wl = x.shape
    h, w = hl * up, wl * up
    if C < 1 or hl < 1 or wl < 1 or max(h, w) > MAX_SIDE:
        raise ValueError(f"{name}: x is {tuple(x.shape)} with up {up}: no empty channel or plane, sides up to {MAX_SIDE}")
    if not isinstance(stats, (tuple, list)) or len(stats) != 2:
        raise TypeError(f"{name}: stats is the pair (mean, rstd)")
    tensors = {"x": x}
    for nm, t in (("mean", stats[0]), ("rstd", stats[1])):
        _tensor_checked(name, nm, t, torch.float32, 1, f"float32 [{bs * C}]")
        if t.shape[0] != bs * C:
            raise ValueError(f"{name}: {nm} is {tuple(t.shape)} for x {tuple(x.shape)}: expected [{bs * C}]")
        tensors[nm] = t
    for nm, t in (("gamma_beta", gamma_beta), ("gamma_beta_s", gamma_beta_s)):
        if t is None and nm == "gamma_beta_s":
            continue
        _tensor_checked(name, nm, t, torch.float32, 4, f"float32 {(bs, 2 * C, h, w)}")
        if tuple(t.shape) != (bs, 2 * C, h, w):
            raise ValueError(f"{name}: {nm} is {tuple(t.shape)} for x {tuple(x.shape)} with up {up}: expected {(bs, 2 * C, h, w)} (gamma | beta)")
        tensors[nm] = t
    _cuda_checked(name, **tensors)
    if any(t.device != x.device for t in tensors.values()):
        raise RuntimeError(f"{name}: device mismatch among the tensors")
    x, mean, rstd, gb = x.detach().contiguous(), stats[0].detach().contiguous(), stats[1].detach().contiguous(), gamma_beta.detach().contiguous()
    gbs = None if gamma_beta_s is None else gamma_beta_s.detach().contiguous()
    out = _out_checked(name, "out", out, (bs, C, h, w), x)
    out_s = None if gbs is None else _out_checked(name, "out_s", out_s, (bs, C, h, w), x)
    lib().call("e4s_v2v_spade_norm", _p(out), _p(out_s), _p(x), _p(mean), _p(rstd), _p(gb), _p(gbs), bs, C, h, w, up, _stream())
    return out if gbs is None else (out, out_s)


def image_head(x, weight, bias, *, out=None):
    """``e4s_v2v_image_head``: ``sigmoid(conv3x3(leaky_0.2(x), weight, zero pad 1) + bias)`` of a float32 ``x [bs, cin, H, W]`` with ``weight [3, cin, 3, 3]`` and
    ``bias [3]``: ``[bs, 3, H, W]`` in exact float32.  ``out``: a dense tensor to write into."""
    name = "image_head"
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, cin, H, W] tensor")
    bs, cin, H, W = x.shape
    if cin < 1 or H < 1 or W < 1 or max(H, W) > MAX_SIDE or bs > 65535:
        raise ValueError(f"{name}: x is {tuple(x.shape)}: no empty channel or plane, sides up to {MAX_SIDE}, a batch up to 65535")
    _tensor_checked(name, "weight", weight, torch.float32, 4, f"float32 {(3, cin, 3, 3)}")
    _tensor_checked(name, "bias", bias, torch.float32, 1, "float32 [3]")
    if tuple(weight.shape) != (3, cin, 3, 3) or tuple(bias.shape) != (3,):
        raise ValueError(f"{name}: weight is {tuple(weight.shape)} and bias {tuple(bias.shape)} for x {tuple(x.shape)}: expected {(3, cin, 3, 3)} and (3,)")
    _cuda_checked(name, x=x, weight=weight, bias=bias)
    if weight.device != x.device or bias.device != x.device:
        raise RuntimeError(f"{name}: device mismatch among the tensors")
    x, weight, bias = x.detach().contiguous(), weight.detach().contiguous(), bias.detach().contiguous()
    out = _out_checked(name, "out", out, (bs, 3, H, W), x)
    lib().call("e4s_v2v_image_head", _p(out), _p(x), _p(weight), _p(bias), bs, cin, H, W, _stream())
    return out


# ------------------------------------------------------------------------------------------------ the decoder
def _up2(x):
    bs, c, h, w = x.shape
    out = torch.empty((bs, c, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    lib().call("e4s_esr_up2", _p(out), _p(x), bs * c, h, w, _stream())
    return out


def _decoder_feature_checked(name, feature):
    _tensor_checked(name, "feature", feature, torch.float32, 4, f"a float32 [n, {DECODER_CHANNELS}, h, w] tensor")
    n, c, h, w = feature.shape
    if c != DECODER_CHANNELS:
        raise ValueError(f"{name}: feature is {tuple(feature.shape)}: the SPADEDecoder takes {DECODER_CHANNELS} channels")
    if h * w < 2:
        raise ValueError(f"{name}: feature is {tuple(feature.shape)}: a plane of {h * w} element(s): the instance norm needs at least 2")
    if 4 * max(h, w) > MAX_SIDE:
        raise ValueError(f"{name}: feature is {tuple(feature.shape)}: the image would be {4 * h} x {4 * w}, sides up to {MAX_SIDE}")
    return n, h, w


def _decoder_run(P, feature):
    """The decoder on prepared weights ``P`` and a dense float32 ``feature [n, 256, h, w]`` on the device, n >= 1."""
    n = feature.shape[0]
    segs = [feature]
    for _ in range(2):
        segs.append(_up2(segs[-1]))
    actv = {}

    def hidden(level):                                                  # the mlp_shared outputs of a resolution, made when its first block is reached
        names = _LEVELS[level]
        if n == 1:
            every = conv_sb(segs[level], *P["stacked"][level], k=3, relu=True)
            for i, nm in enumerate(names):
                actv[nm] = every[:, i * SPADE_HIDDEN:(i + 1) * SPADE_HIDDEN]
        else:
            for nm in names:
                actv[nm] = conv_sb(segs[level], *P["norms"][nm]["shared"], k=3, relu=True)

    def gamma_beta(nm):
        return conv_sb(actv.pop(nm), *P["norms"][nm]["gb"], k=3)

    x = conv_sb(feature, *P["fc"], k=3)
    hidden(0)
    level = 0
    for B in P["blocks"]:
        p, up = B["name"], B["up"]
        if up == 2:
            level += 1
            hidden(level)
        stats = _plane_stats(x)                                         # norm_0 and norm_s normalise the same x
        bs, C, hl, wl = x.shape
        outs = [torch.empty((bs, C, up * hl, up * wl), dtype=torch.float32, device=x.device)]
        gb0 = gamma_beta(p + ".norm_0")
        gbs = None
        if B["conv_s"] is not None:
            gbs = gamma_beta(p + ".norm_s")
            outs.append(torch.empty_like(outs[0]))
        lib().call("e4s_v2v_spade_norm", _p(outs[0]), _p(outs[1]) if gbs is not None else None, _p(x), _p(stats[0]), _p(stats[1]), _p(gb0), _p(gbs), bs, C,
                   up * hl, up * wl, up, _stream())
        del gb0, gbs
        shortcut = conv_sb(outs[1], *B["conv_s"], k=1) if B["conv_s"] is not None else x
        dx = conv_sb(outs[0], *B["conv_0"], k=3)
        del outs
        stats = _plane_stats(dx)
        gb1 = gamma_beta(p + ".norm_1")
        a1 = torch.empty_like(dx)
        lib().call("e4s_v2v_spade_norm", _p(a1), None, _p(dx), _p(stats[0]), _p(stats[1]), _p(gb1), None, bs, dx.shape[1], dx.shape[2], dx.shape[3], 1,
                   _stream())
        x = conv_sb(a1, *B["conv_1"], k=3, residual=shortcut)
    w, b = P["img"]
    out = torch.empty((n, 3, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
    lib().call("e4s_v2v_image_head", _p(out), _p(x), _p(w), _p(b), n, x.shape[1], x.shape[2], x.shape[3], _stream())
    return out


def _decoder_checked_run(name, feature, weights, checked):
    n, h, w = _decoder_feature_checked(name, feature)
    _placed_checked(name, "feature", feature, checked[2])
    if n == 0:
        return feature.new_empty((0, 3, 4 * h, 4 * w))
    with torch.no_grad():
        P = prepare(PreparedSPADEDecoder, weights, checked)
        return _decoder_run(P, feature.detach().contiguous())


def spade_decoder_forward(feature, weights):
    """``SPADEDecoder.forward`` in eval mode on the device: ``prediction [n, 3, 4 h, 4 w]`` in (0, 1) from a float32 ``feature [n, 256, h, w]`` (``generator_warp``'s
    ``'feature'``).  ``weights``: a ``SPADEDecoder``; a generator module, this package's mirror or the reference's own class (only its keys are read); a mapping
    with the decoder's bare keys or with them behind ``decoder.``, ``generator.decoder.`` or ``module.``; or the checkpoint file as ``torch.load`` gives it.
    Refused before any launch: a module in training mode (``NotImplementedError``), a mapping that lacks a decoder key (``KeyError`` naming it), a feature that is
    not float32, has other than 256 channels, a plane of fewer than 2 elements or an image side above 16384 (``ValueError``), then a CPU tensor
    (``RuntimeError``).  ``n == 0`` returns an empty tensor."""
    name = "spade_decoder_forward"
    weights, checked = _decoder_checked(name, weights)
    return _decoder_checked_run(name, feature, weights, checked)


# ------------------------------------------------------------------------------------------------ whole frames
def _frames_checked(name, weights):
    """Both halves of a generator's weights validated before anything runs: (weights for the front, weights and ``_validated`` result for the decoder, what
    the front's tensors are keyed on: storage and version of each)."""
    dec_weights, dec_checked = _decoder_checked(name, weights)
    front, front_checked, _ = _generator_checked(name, weights)
    return front, dec_weights, dec_checked, weights_key(front_checked[2])


def _frames(name, feature_3d, kp_driving, kp_source, front, dec_weights, dec_checked):
    out = generator_warp(feature_3d, kp_driving, kp_source, front)
    feature = out.pop("feature")
    del out["deformation"]                                  # the reference's output_dict holds the mask, the occlusion map and the prediction
    out["prediction"] = _decoder_checked_run(name, feature, dec_weights, dec_checked)
    return out


def generator_frames(feature_3d, kp_driving, kp_source, weights):
    """The per-frame part of ``OcclusionAwareSPADEGenerator.forward`` with its decoder: ``generator_warp`` and ``spade_decoder_forward``, returning the reference's
    ``output_dict`` ``{'mask'[, 'occlusion_map'], 'prediction' [n, 3, H, W]}``.  ``feature_3d`` is ``appearance_feature``'s, of batch n or 1 (shared by every
    frame).  ``weights``: the generator as a module (the mirror or the reference's class), ``checkpoint['generator']``, the checkpoint itself, or such a mapping
    behind ``generator.`` / ``module.``; the decoder's keys are needed here and a mapping without them is refused with ``KeyError`` before any launch."""
    name = "generator_frames"
    return _frames(name, feature_3d, kp_driving, kp_source, *_frames_checked(name, weights)[:3])


def generator_forward(source, kp_driving, kp_source, weights):
    """``OcclusionAwareSPADEGenerator.forward(source, kp_driving, kp_source)`` in eval mode on the device: ``generator_frames(appearance_feature(source, weights),
    ...)``.  ``source`` holds one image, or one per keypoint set."""
    name = "generator_forward"
    checked = _frames_checked(name, weights)
    _tensor_checked(name, "source", source, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    kps = _keypoints_checked(name, kp_driving, kp_source)
    if source.shape[0] not in (1, kps[0].shape[0]):
        raise ValueError(f"{name}: source is {tuple(source.shape)} for keypoints of batch {kps[0].shape[0]}: expected that batch, or 1")
    return _frames(name, appearance_feature(source, checked[0]), kp_driving, kp_source, *checked[:3])


class NativeSPADEGenerator(nn.Module):
    """A loaded ``OcclusionAwareSPADEGenerator`` (this package's mirror or the reference's own class: only its keys are read) whose ``forward(source_image,
    kp_driving, kp_source)`` is ``generator_forward``; positional or by keyword, as the reference's ``make_animation`` calls it, so that function and
    ``drive_source_demo`` run natively when handed this module.  ``make_animation`` passes the same ``source`` tensor for every frame: the wrapper holds the last
    source tensor OBJECT with its ``_version`` and that source's ``feature_3d``, and builds the feature again when either differs.  Holding the object keeps its
    memory from being handed to another tensor under the same pointer.  ``feature_builds`` counts how often the feature was built.  A change of the generator's
    weights (a tensor's storage or version) builds it again too."""

    def __init__(self, generator):
        super().__init__()
        if not isinstance(generator, nn.Module):
            raise TypeError("NativeSPADEGenerator: generator is a loaded OcclusionAwareSPADEGenerator module")
        self.generator = generator
        self.feature_builds = 0
        self._source = self._feature = self._key = None

    def forward(self, source_image, kp_driving, kp_source):
        name = "NativeSPADEGenerator"
        checked = _frames_checked(name, self.generator)
        _tensor_checked(name, "source_image", source_image, torch.float32, 4, "a float32 [bs, 3, H, W] image")
        key = (source_image._version, checked[3])
        if source_image is not self._source or key != self._key:
            self._feature = appearance_feature(source_image, checked[0])
            self._source, self._key = source_image, key
            self.feature_builds += 1
        kps = _keypoints_checked(name, kp_driving, kp_source)
        if self._feature.shape[0] not in (1, kps[0].shape[0]):
            raise ValueError(f"{name}: source_image is {tuple(source_image.shape)} for keypoints of batch {kps[0].shape[0]}: expected that batch, or 1")
        return _frames(name, self._feature, kp_driving, kp_source, *checked[:3])


def make_animation(source, driving, generator, kp_detector, he_estimator, estimate_jacobian=None, free_view=False, yaw=0, pitch=0, roll=0, batch=4):
    """``make_animation`` of drive_demo.py:182-211 for device tensors: float32 ``source [1, 3, H, W]`` and ``driving [n, 3, H, W]`` in [0, 1] to ``prediction
    [n, 3, H', W']`` on the device.  The detector and the appearance feature are computed once, ONE head-pose pass runs over the n + 1 images, ``kp_source`` is
    transformed without the free-view angles and ``kp_driving`` with them, as the reference does, and the generator runs in chunks of ``batch`` frames (the last
    may be short; a frame's bits do not depend on its chunk).  ``estimate_jacobian``: default, whether the detector has a Jacobian head.  The three networks as
    ``generator_frames``, ``kp_detector_forward`` and ``he_estimator_forward`` take weights."""
    name = "make_animation"
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise ValueError(f"{name}: batch is {batch!r}: a positive number of frames per generator call")
    checked = _frames_checked(name, generator)
    for nm, t in (("source", source), ("driving", driving)):
        _tensor_checked(name, nm, t, torch.float32, 4, "a float32 [n, 3, H, W] image batch")
    if source.shape[0] != 1 or driving.shape[1:] != source.shape[1:]:
        raise ValueError(f"{name}: source is {tuple(source.shape)} and driving {tuple(driving.shape)}: expected [1, 3, H, W] and [n, 3, H, W] of one size")
    _cuda_checked(name, source=source, driving=driving)
    n = driving.shape[0]
    feature_3d = appearance_feature(source, checked[0])
    kp_canonical = kp_detector_forward(source, kp_detector)
    if estimate_jacobian is None:
        estimate_jacobian = "jacobian" in kp_canonical
    he = he_estimator_forward(torch.cat((source, driving)), he_estimator)
    part = lambda a, b: {k: v[a:b] for k, v in he.items()}      # noqa: E731
    kp_source = keypoint_transformation(kp_canonical, part(0, 1), estimate_jacobian)
    kp_driving = keypoint_transformation(kp_canonical, part(1, None), estimate_jacobian, free_view=free_view, yaw=yaw, pitch=pitch, roll=roll)
    if n == 0:
        f = 4 * feature_3d.shape[3], 4 * feature_3d.shape[4]
        return source.new_empty((0, 3) + f)
    frames = []
    for i in range(0, n, batch):
        m = min(batch, n - i)
        kd = {k: v[i:i + m] for k, v in kp_driving.items() if v is not None}
        ks = {k: v.expand(m, *v.shape[1:]) for k, v in kp_source.items() if v is not None}
        frames.append(_frames(name, feature_3d, kd, ks, *checked[:3])["prediction"])
    return frames[0] if len(frames) == 1 else torch.cat(frames)


__all__ = ["PreparedSPADEDecoder", "spade_norm", "image_head", "spade_decoder_forward", "generator_frames", "generator_forward", "NativeSPADEGenerator",
           "make_animation"]
