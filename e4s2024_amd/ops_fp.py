"""Face-parsing feature loss (``criteria/face_parsing/face_parsing_loss.py::FaceParsingLoss`` on ``criteria/face_parsing/unet.py::unet(feature_scale=4)``)
on the HIP kernels: forward and gradient with respect to the reconstruction, for the parsing term of the PTI and W-optimisation loops
(training/video_swap_ft_coach.py:179-219, optimization.py:111-145).

    AdaptiveAvgPool2d(512)          unless H is 512: csrc/idloss.hip's banded resampler out = A_y X A_x^T (A [512, H] from PyTorch's adaptive-pool
                                    windows, built here in float64; a 2 x 2 box mean at 1024, pixel replication at 256) and its adjoint
    5 blocks [conv 3x3 + BN + ReLU] x 2, MaxPool2d(2) between them (16, 32, 64, 128, 256 channels)
                                    conv bias and BN folded into the weights in float64; the 3-channel first convolution on csrc/conv.hip's fp32 kernel,
                                    the others on its three-way split-bf16 kernel (fp32-class: near convergence the gradient is a difference of nearly
                                    equal vectors), ReLU in the epilogue; max pool in csrc/fploss.hip
    taps                            every block's output, flattened per sample and l2-normalised; heads on csrc/idloss.hip (fixed-order partial sums:
                                    bit-identical reruns; the loss lands in a device scalar, no host sync)
    data gradients                  per block, csrc/fploss.hip's tap backward (head gradient + the next block's gradient through the max pool to the first
                                    maximum of each window, times the ReLU mask) -> second conv's data gradient -> ReLU mask -> first conv's data gradient,
                                    both convolutions on csrc/conv.hip's two-way split on flipped, transposed weights with the BN scales folded in

``y_hat`` and ``y`` run through the network as one batch of ``2 bs``; only ``y_hat``'s activations are kept for the backward.  Weights are a
``unet``-shaped module (``FaceParsingNet``, or the drop-in ``criteria.face_parsing.face_parsing_loss.FaceParsingLoss`` / its ``G``) or a mapping with
at least the encoder's keys (``state_dict_keys()`` lists all 136; the decoder's ``up_concat*`` / ``final`` are not used by the loss).  They are
frozen: no weight gradient is computed.  BatchNorm uses its running statistics (the reference puts the network in eval mode); a module left in
training mode is refused.  Validation of the weights (keys, shapes, dtypes: once per public call) and the cache of their prepared copies are
``netweights``', as for every network of the package; BN folding, split-bf16 weight preparation and convolution wrapper, the resampler, the heads
and the multi-target helpers are ``lossnet``'s, shared with ``ops_lpips`` and ``ops_id``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from typing import Optional

from . import lossnet, netweights
from ._lib import lib
from .lossnet import (call_args, check_frame, check_image, check_targets, conv_exact, conv_sb, cos_heads, cos_heads_multi, fold_conv_bn, pool_matrix,
                      prep_dgrad, prep_exact, prep_fwd, relu_mask, target_rows)
from .netweights import PreparedNet, _Net, _keys_shapes, _validated, weights_key
from .ops import _c, _p, _stream

SIDE = 512                                   # FaceParsingLoss.face_pool: AdaptiveAvgPool2d((512, 512)) unless x.shape[2] == 512
FILTERS = (16, 32, 64, 128, 256)             # unet(feature_scale=4): [64, 128, 256, 512, 1024] / 4
BLOCKS = ("conv1", "conv2", "conv3", "conv4", "center")
N_CLASSES = 19


# ------------------------------------------------------------------------------------------------ the module (parameter layout only)
class _UnetConv2(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.ReLU())
        self.conv2 = nn.Sequential(nn.Conv2d(cout, cout, 3, 1, 1), nn.BatchNorm2d(cout), nn.ReLU())


class _UnetUp(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.conv = _UnetConv2(cin, cout)
        self.up = nn.ConvTranspose2d(cin, cout, kernel_size=2, stride=2)


class FaceParsingNet(nn.Module):
    """``unet(feature_scale=4, n_classes=19)`` with the reference's module names, so its ``state_dict`` has the reference's 136 keys in their order.
    The submodules only hold the weights: ``extract_feats(x)`` runs the encoder on the HIP kernels.  The decoder (``up_concat*``, ``final``) is kept
    for the checkpoint's sake only; ``forward`` (the segmentation) is not provided.  It starts without weights and refuses to run until
    ``load_state_dict`` has filled it."""

    def __init__(self):
        super().__init__()
        f = FILTERS
        self.conv1 = _UnetConv2(3, f[0])
        self.conv2 = _UnetConv2(f[0], f[1])
        self.conv3 = _UnetConv2(f[1], f[2])
        self.conv4 = _UnetConv2(f[2], f[3])
        self.center = _UnetConv2(f[3], f[4])
        self.up_concat4 = _UnetUp(f[4], f[3])
        self.up_concat3 = _UnetUp(f[3], f[2])
        self.up_concat2 = _UnetUp(f[2], f[1])
        self.up_concat1 = _UnetUp(f[1], f[0])
        self.final = nn.Conv2d(f[0], N_CLASSES, 1)
        self.requires_grad_(False)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if set(encoder_keys()) <= set(state_dict.keys()):
            self._loaded = True
        return out

    def forward(self, x):
        raise NotImplementedError("FaceParsingNet: the segmentation (the unet decoder) is not implemented; the loss uses extract_feats")

    def extract_feats(self, x: torch.Tensor):
        return unet_features(x, self)


def state_dict_keys():
    """The 136 keys of ``unet().state_dict()``, in its order."""
    return [k for k, _ in _keys_shapes(FaceParsingNet)]


def state_dict_shapes():
    """``{key: shape}`` of ``unet().state_dict()``."""
    return dict(_keys_shapes(FaceParsingNet))


def encoder_keys():
    """The 70 keys of the five encoder blocks (``extract_feats``' parameters and BatchNorm statistics)."""
    return [k for k in state_dict_keys() if k.split(".")[0] in BLOCKS]


def encoder_shapes():
    """``{key: shape}`` of the encoder's 70 keys: what the weights of the loss are checked against."""
    return {k: shape for k, shape in _keys_shapes(FaceParsingNet) if k.split(".")[0] in BLOCKS}


# ------------------------------------------------------------------------------------------------ weights
_FP_NET = _Net("unet(feature_scale=4)'s encoder", encoder_shapes, ("G.",), False, ("conv1.conv1.0.weight",), None,
               "the face-parsing loss runs the network in eval mode", ("num_batches_tracked",))


def _network(weights):
    """The network of ``weights``: the drop-in FaceParsingLoss holds it as ``G``.  Its ``_loaded`` and ``training`` flags are the ones that count."""
    return getattr(weights, "G", weights) if isinstance(weights, nn.Module) else weights


def check_loaded(weights):
    """``weights`` itself; raises if it is a module whose weights were never loaded (a loss from initial parameters would be a silently wrong
    objective) or one left in training mode (BatchNorm on batch statistics: different arithmetic from the eval-mode reference)."""
    netweights.check_loaded(None, _network(weights), "the face-parsing weights")
    netweights.check_eval(None, _network(weights), _FP_NET)
    return weights


def _checked(name, weights):
    """(the network of ``weights``, what ``_validated`` returns of its encoder): what a public call makes once, before it looks at its images, and
    hands to ``netweights.prepare``.  Refused in this order: weights never loaded, training mode, a missing key, a wrong shape or dtype."""
    net = _network(weights)
    netweights.check_loaded(name, net, "the face-parsing weights")
    return net, _validated(name, net, _FP_NET)


def weight_tensors(weights, name: str = "fp_loss"):
    """The float tensors of the encoder (``num_batches_tracked`` aside), in key order, their shapes checked: what ``weights_key`` watches."""
    return _checked(name, weights)[1][2]


class PreparedFaceParsingNet(PreparedNet):
    """The kernels' copies of the encoder weights, rebuilt when a tensor changes version or storage: per block the forward weights of both convolutions
    (conv bias and BN folded in; fp32 layout for the 3-channel input, three-way split slabs otherwise) and two-way split slabs of their data gradients
    (BN scales folded in)."""

    __slots__ = ()

    _entry, _net = "fp_loss", _FP_NET

    def _build(self, sd, variant, dev):
        blocks = []
        for i, name in enumerate(BLOCKS):
            cin, cout = (3 if i == 0 else FILTERS[i - 1]), FILTERS[i]
            w1, w2 = sd[name + ".conv1.0.weight"], sd[name + ".conv2.0.weight"]
            s1, t1 = fold_conv_bn(sd, name + ".conv1.0", name + ".conv1.1")
            s2, t2 = fold_conv_bn(sd, name + ".conv2.0", name + ".conv2.1")
            fwd1 = (prep_exact if cin < 16 else prep_fwd)(w1, s1, t1)
            blocks.append(dict(cin=cin, cout=cout, fwd1=fwd1, fwd2=prep_fwd(w2, s2, t2), bwd1=prep_dgrad(w1, out_scale=s1),
                               bwd2=prep_dgrad(w2, out_scale=s2)))
        return tuple(blocks)


def prepare(weights):
    """Prepared copies for ``weights`` (cached on a module; a plain mapping is prepared on every call)."""
    return netweights.prepare(PreparedFaceParsingNet, *_checked("fp_loss", weights))


# ------------------------------------------------------------------------------------------------ input pooling
def resampler(h: int, w: int, device):
    """AdaptiveAvgPool2d((512, 512)) on an h x w image (a cached ``lossnet.Resampler``), or None when h is 512 (the reference then runs the network
    on the image as it is)."""
    if h == SIDE:
        return None
    return lossnet.resampler(h, w, SIDE, device, lambda: (pool_matrix(h, SIDE), pool_matrix(w, SIDE)))


def _network_input(xs, R):
    """The network's input batch: the images of ``xs`` (each [bs, 3, H, W]) one after the other, pooled to 512 x 512 unless H is 512."""
    bs, c, h, w = xs[0].shape
    ho, wo = (h, w) if R is None else (SIDE, SIDE)
    out = torch.empty((bs * len(xs), c, ho, wo), dtype=torch.float32, device=xs[0].device)
    for i, x in enumerate(xs):
        dst = out[i * bs:(i + 1) * bs]
        if R is None:
            dst.copy_(x)
        else:
            R.apply(x, out=dst)
    return out


# ------------------------------------------------------------------------------------------------ forward
def _conv_relu(x, B, which):
    conv = conv_exact if which == 1 and B["cin"] < 16 else conv_sb
    return conv(x, *B["fwd1" if which == 1 else "fwd2"], k=3, relu=True)


def _encoder(x, P):
    """``[(c1, c2)]`` per block: the first convolution's output (its ReLU mask is needed by the backward) and the block output (the tap)."""
    acts = []
    a = x
    for i, B in enumerate(P):
        c1 = _conv_relu(a, B, 1)
        c2 = _conv_relu(c1, B, 2)
        acts.append((c1, c2))
        if i + 1 < len(P):
            n, c, h, w = c2.shape
            a = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
            lib().call("e4s_fp_maxpool2", _p(a), _p(c2), n * c, h, w, _stream())
    return acts


def _input_grad(acts, P, stats, gout, bs, tap_bwd=None):
    """d loss / d (the network's input) of the first ``bs`` samples.  ``tap_bwd(gz, i, gpool)``: writes block i's tap gradient in place of the
    single-target one (the multi-target loss)."""
    g = None
    for i in range(len(P) - 1, -1, -1):
        B = P[i]
        c1, c2 = acts[i]
        _, c, h, w = c2.shape
        gz = torch.empty((bs, c, h, w), dtype=torch.float32, device=c2.device)
        if tap_bwd is None:
            lib().call("e4s_fp_tap_bwd", _p(gz), _p(c2[:bs]), _p(c2[bs:]), _p(stats[i]), _p(gout), _p(g), bs, c, h, w, 1.0 / bs, _stream())
        else:
            tap_bwd(gz, i, g)
        gc1 = conv_sb(gz, B["bwd2"], k=3)
        relu_mask(gc1, c1)                                             # c1[:bs] is the head of c1: same offsets
        g = conv_sb(gc1, B["bwd1"], k=3)
    return g


def _image_grad(g, R, shape):
    """d loss / d image from ``g`` = d loss / d (the network's input)."""
    return g if R is None else R.adjoint(g, shape)


class _FpLoss(torch.autograd.Function):
    """(loss, sim_improvement, stats) of FaceParsingLoss.forward(y_hat, y); differentiable in ``y_hat`` only (the reference detaches ``y``'s features)."""

    @staticmethod
    def forward(ctx, y_hat, y, P, R):
        bs = y_hat.shape[0]
        acts = _encoder(_network_input((y_hat, y), R), P)
        fx = [c2[:bs].reshape(bs, -1) for _, c2 in acts]
        fy = [c2[bs:].reshape(bs, -1) for _, c2 in acts]
        loss, sim, stats = cos_heads(fx, fy)
        ctx.P, ctx.R, ctx.shape = P, R, tuple(y_hat.shape)
        ctx.acts = [(c1[:bs], c2) for c1, c2 in acts]              # y's half of c2 is the head's fy; y's c1 is not needed
        ctx.save_for_backward(stats)
        ctx.mark_non_differentiable(sim, stats)
        ctx.set_materialize_grads(False)                                # no zero-filled gradients for sim / stats
        return loss, sim, stats

    @staticmethod
    def backward(ctx, gloss, gsim, gstats):
        if gloss is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        (stats,) = ctx.saved_tensors
        bs = ctx.shape[0]
        gout = _c(gloss.reshape(1), "grad_output")
        g = _input_grad(ctx.acts, ctx.P, stats, gout, bs)
        ctx.acts = None
        return _image_grad(g, ctx.R, ctx.shape), None, None, None


class _FpLossMulti(torch.autograd.Function):
    """sum_j tw[j] FaceParsingLoss(y_hat, y_j) from the targets' cached block outputs; differentiable in ``y_hat`` only."""

    @staticmethod
    def forward(ctx, y_hat, P, R, ys, tw, frame):
        bs = y_hat.shape[0]
        acts = _encoder(_network_input((y_hat,), R), P)
        fx = [c2.reshape(bs, -1) for _, c2 in acts]
        loss, stats = cos_heads_multi(fx, ys, tw, frame)
        ctx.P, ctx.R, ctx.shape, ctx.ys, ctx.tw, ctx.frame = P, R, tuple(y_hat.shape), ys, tw, frame
        ctx.acts = acts
        ctx.save_for_backward(stats)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        (stats,) = ctx.saved_tensors
        bs = ctx.shape[0]
        gout = _c(gloss.reshape(1), "grad_output")
        acts = ctx.acts

        def tap_bwd(gz, i, gpool):
            c2 = acts[i][1]
            lib().call("e4s_fp_tap_bwd_multi", _p(gz), _p(c2), *call_args([y[i] for y in ctx.ys], ctx.tw, ctx.frame, bs), _p(stats[i]), _p(gout),
                       _p(gpool), bs, c2.shape[1], c2.shape[2], c2.shape[3], 1.0 / bs, _stream())
        g = _input_grad(acts, ctx.P, stats, gout, bs, tap_bwd)
        ctx.acts = None
        return _image_grad(g, ctx.R, ctx.shape), None, None, None, None, None


def target_features(images: torch.Tensor, weights):
    """The raw block outputs of ``images`` ``[n, 3, H, W]`` that ``fp_loss_multi`` reads for a target: five ``[n, D]`` tensors.  Computed a frame at a
    time; no gradient."""
    W = _checked("ops_fp.target_features", weights)
    images = _check(images.detach(), "images")
    P, R = netweights.prepare(PreparedFaceParsingNet, *W), resampler(images.shape[2], images.shape[3], images.device)
    with torch.no_grad():
        return target_rows(lambda x: [c2.reshape(x.shape[0], -1) for _, c2 in _encoder(_network_input((x.contiguous(),), R), P)], images)


def fp_loss_multi(y_hat: torch.Tensor, targets, tw, weights, frame: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sum_j tw[j] * fp_loss(y_hat, y_j)`` (0-d, differentiable in ``y_hat`` only) with one encoder pass and input gradient of ``y_hat``:
    ``targets[j] = target_features(y_j, weights)`` (``bs`` rows, or frames x ``bs`` rows with ``frame``, a device int32 frame index)."""
    W = _checked("fp_loss_multi", weights)
    y_hat = _check(y_hat, "y_hat")
    frame = check_frame(frame, y_hat.device)
    bs = y_hat.shape[0]
    side_h, side_w = (y_hat.shape[2], y_hat.shape[3]) if y_hat.shape[2] == SIDE else (SIDE, SIDE)
    P = netweights.prepare(PreparedFaceParsingNet, *W)
    dims = [B["cout"] * (side_h >> i) * (side_w >> i) for i, B in enumerate(P)]
    ys = check_targets([torch.empty((bs, d), device="meta") for d in dims], targets, tw, frame, "fp_loss_multi")
    return _FpLossMulti.apply(y_hat, P, resampler(y_hat.shape[2], y_hat.shape[3], y_hat.device), ys, [float(w) for w in tw], frame)


def _check(x: torch.Tensor, name: str) -> torch.Tensor:
    x = check_image(x, name)
    if x.shape[2] == SIDE and x.shape[3] % 16:
        raise ValueError(f"{name}: a {SIDE}-high image is not pooled (FaceParsingLoss.extract_feats), so its width must be a multiple of 16 for the "
                         f"four 2 x 2 max pools; got {tuple(x.shape[2:])}")
    return x


def _apply(y_hat, y, weights):
    W = _checked("fp_loss", weights)
    y_hat, y = _check(y_hat, "y_hat"), _check(y.detach(), "y")
    if y_hat.shape != y.shape:
        raise ValueError(f"y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} differ")
    return _FpLoss.apply(y_hat, y, netweights.prepare(PreparedFaceParsingNet, *W), resampler(y.shape[2], y.shape[3], y.device))


def fp_loss_terms(y_hat: torch.Tensor, y: torch.Tensor, weights):
    """``(loss, sim_improvement, per_tap)``: the loss (0-d, differentiable in ``y_hat``), FaceParsingLoss's similarity improvement (0-d, on the device)
    and ``per_tap [5]`` = mean over the batch of 1 - cos per encoder block (no gradient).  No host synchronisation."""
    loss, sim, stats = _apply(y_hat, y, weights)
    return loss, sim, (1.0 - stats[..., 2]).mean(1)


def fp_loss(y_hat: torch.Tensor, y: torch.Tensor, weights) -> torch.Tensor:
    """FaceParsingLoss.forward(y_hat, y)'s loss (a 0-d tensor): ``sum over the five encoder blocks of mean_i (1 - cos(f(y_hat_i), f(y_i)))``.
    ``y_hat``, ``y``: fp32 ``[bs, 3, H, W]`` on the device, pooled to 512 x 512 unless H is 512.  Differentiable in ``y_hat`` only."""
    return _apply(y_hat, y, weights)[0]


def _unet_features(x, W):
    x = _c(x, "x")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 16 or x.shape[3] % 16:
        raise ValueError(f"x: expected [bs, 3, H, W] with H, W multiples of 16, got {tuple(x.shape)}")
    with torch.no_grad():
        acts = _encoder(x, netweights.prepare(PreparedFaceParsingNet, *W))
    bs = x.shape[0]
    return [c2.reshape(bs, -1) / c2.reshape(bs, -1).norm(dim=1, keepdim=True) for _, c2 in acts]


def unet_features(x: torch.Tensor, weights):
    """unet.extract_feats(x): the l2-normalised block outputs of the image as it is (H, W multiples of 16; no gradient)."""
    return _unet_features(x, _checked("unet_features", weights))


def fp_features(x: torch.Tensor, weights):
    """FaceParsingLoss.extract_feats(x): the l2-normalised features after the pooling to 512 x 512 (unless H is 512; no gradient)."""
    W = _checked("fp_features", weights)
    x = _check(x, "x")
    with torch.no_grad():
        x512 = _network_input((x,), resampler(x.shape[2], x.shape[3], x.device))
    return _unet_features(x512, W)


__all__ = ["FaceParsingNet", "PreparedFaceParsingNet", "check_loaded", "weights_key", "weight_tensors", "prepare", "state_dict_keys", "state_dict_shapes",
           "encoder_keys", "encoder_shapes", "resampler", "fp_features", "unet_features", "fp_loss", "fp_loss_terms", "target_features", "fp_loss_multi"]
