"""ArcFace IR-SE50 identity loss (``criteria/id_loss.py::IDLoss`` on ``models/encoders/model_irse.py::Backbone(112, 50, 'ir_se')``) on the HIP
kernels: forward and gradient with respect to the reconstruction, for the identity term of the PTI and W-optimisation loops
(training/video_swap_ft_coach.py:179-219, optimization.py:111-146).

    pool -> crop -> pool            csrc/idloss.hip: out = A_y X A_x^T (A [112, H] from PyTorch's adaptive-pool windows, built here in float64) and its adjoint
    input layer conv 3x3 (+BN)      csrc/conv.hip, three-way split-bf16 (fp32-class: near convergence the gradient is a difference of nearly equal vectors)
    units: BN -> conv -> PReLU      BN as scale / shift (csrc/idloss.hip, exact for gamma = 0), conv three-way split, PReLU keeps its pre-activation
           conv (stride s) + BN     BN folded into the weights (no padding after the conv, so the fold is exact); SE gate and shortcut add on csrc/norm.hip
    output layer BN2d-Linear-BN1d   folded into one [512, 25088] weight once per weight version; GEMV and its transpose in csrc/idloss.hip
    heads                           csrc/idloss.hip: fixed-order partial sums (bit-identical reruns); the loss lands in a device scalar (no host sync)
    data gradients                  stride-1 3x3 / 1x1 on csrc/conv.hip (two-way split, flipped transposed weights with the BN scales folded in);
                                    stride-2 3x3 on csrc/modconv_sb.hip's transposed convolution (two-way split, 1x the MACs); SE and PReLU backward,
                                    the stride-2 shortcut scatter in csrc/idloss.hip

Weights are a ``Backbone``-shaped module (``IdNet``, or the drop-in ``criteria.id_loss.IDLoss`` / its ``facenet``) or a mapping with the
reference's 397 keys (``state_dict_keys()``).  They are frozen: no weight gradient is computed.  BatchNorm uses its running statistics (the
reference puts the network in eval mode); a module left in training mode is refused.  Validation of the weights (keys, shapes, dtypes: once per public call) and the cache of their prepared copies are ``netweights``',
as for every network of the package; BN folding, split-bf16 weight preparation and convolution wrapper, the resampler, the heads and the multi-target
helpers are ``lossnet``'s, shared with ``ops_lpips`` and ``ops_fp``.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from typing import Optional

from . import lossnet, netweights
from ._lib import lib
from .lossnet import (bn_fold, call_args, check_frame, check_image, check_targets, conv_sb, cos_heads, cos_heads_multi as heads_multi, pool_matrix,
                      prep_dgrad, prep_fwd, target_rows)
from .netweights import PreparedNet, _Net, _keys_shapes, _validated, weights_key

_pool_matrix, _bands = pool_matrix, lossnet.bands       # their names before they moved to lossnet, kept for callers outside the package
from .ops import _c, _p, _stream

SIDE = 112                                   # the network's input side (IDLoss.face_pool_2)
CROP = ((35, 223), (32, 220))                # IDLoss.extract_feats: rows, columns of the 256 x 256 image
STAGES = ((64, 64, 3), (64, 128, 4), (128, 256, 14), (256, 512, 3))      # get_blocks(50): (in_channel, depth, units)
TAP_UNITS = (2, 6, 20, 23)                   # Backbone.forward(multi_scale=True): body outputs that are features as well


def units():
    """``(in_channel, depth, stride)`` of the 24 ``bottleneck_IR_SE`` units."""
    out = []
    for cin, depth, n in STAGES:
        out.append((cin, depth, 2))
        out += [(depth, depth, 1)] * (n - 1)
    return out


# ------------------------------------------------------------------------------------------------ the module (parameter layout only)
class _SE(nn.Module):
    def __init__(self, c: int, reduction: int = 16):
        super().__init__()
        self.fc1 = nn.Conv2d(c, c // reduction, 1, bias=False)
        self.fc2 = nn.Conv2d(c // reduction, c, 1, bias=False)


class _Unit(nn.Module):
    def __init__(self, cin: int, depth: int, stride: int):
        super().__init__()
        self.shortcut_layer = nn.MaxPool2d(1, stride) if cin == depth else nn.Sequential(nn.Conv2d(cin, depth, 1, stride, bias=False), nn.BatchNorm2d(depth))
        self.res_layer = nn.Sequential(nn.BatchNorm2d(cin), nn.Conv2d(cin, depth, 3, 1, 1, bias=False), nn.PReLU(depth),
                                       nn.Conv2d(depth, depth, 3, stride, 1, bias=False), nn.BatchNorm2d(depth), _SE(depth))


class IdNet(nn.Module):
    """``Backbone(112, 50, 'ir_se')`` with the reference's module names, so its ``state_dict`` has the reference's 397 keys in their order.
    The submodules only hold the weights: ``forward(x, multi_scale)`` runs the HIP kernels (``features_112``: a 112 x 112 input).  It starts
    without weights and refuses to run until ``load_state_dict`` has filled it."""

    def __init__(self):
        super().__init__()
        self.input_layer = nn.Sequential(nn.Conv2d(3, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.PReLU(64))
        self.output_layer = nn.Sequential(nn.BatchNorm2d(512), nn.Dropout(0.6), nn.Flatten(), nn.Linear(512 * 7 * 7, 512), nn.BatchNorm1d(512))
        self.body = nn.Sequential(*[_Unit(*u) for u in units()])
        self.requires_grad_(False)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if set(state_dict_keys()) <= set(state_dict.keys()):
            self._loaded = True
        return out

    def forward(self, x: torch.Tensor, multi_scale: bool = False):
        return features_112(x, self, multi_scale)


def state_dict_keys():
    """The 397 keys of ``Backbone(112, 50, 'ir_se').state_dict()``, in its order."""
    return [k for k, _ in _keys_shapes(IdNet)]


def state_dict_shapes():
    """``{key: shape}`` of ``Backbone(112, 50, 'ir_se').state_dict()``."""
    return dict(_keys_shapes(IdNet))


# ------------------------------------------------------------------------------------------------ weights
_ID_NET = _Net("Backbone(112, 50, 'ir_se')", state_dict_shapes, ("facenet.",), False, ("input_layer.0.weight",), None,
               "the identity loss runs the network in eval mode", ("num_batches_tracked",))


def _network(weights):
    """The network of ``weights``: the drop-in IDLoss holds it as ``facenet``.  Its ``_loaded`` and ``training`` flags are the ones that count."""
    return getattr(weights, "facenet", weights) if isinstance(weights, nn.Module) else weights


def check_loaded(weights):
    """``weights`` itself; raises if it is a module whose weights were never loaded (a loss from initial parameters would be a silently wrong
    objective) or one left in training mode (BatchNorm on batch statistics and active dropout: different arithmetic from the eval-mode
    reference)."""
    netweights.check_loaded(None, _network(weights), "the ArcFace weights")
    netweights.check_eval(None, _network(weights), _ID_NET)
    return weights


def _checked(name, weights):
    """(the network of ``weights``, what ``_validated`` returns of it): what a public call makes once, before it looks at its images, and hands to
    ``netweights.prepare``.  Refused in this order: weights never loaded, training mode, a missing key, a wrong shape or dtype."""
    net = _network(weights)
    netweights.check_loaded(name, net, "the ArcFace weights")
    return net, _validated(name, net, _ID_NET)


def weight_tensors(weights, name: str = "id_loss"):
    """The float tensors of ``weights`` (``num_batches_tracked`` aside), in key order, their shapes checked: what ``weights_key`` watches."""
    return _checked(name, weights)[1][2]


def _prep_tconv(w, out_scale):
    """Slabs of the stride-2 3x3 data gradient for e4s_modconv_tconv_sb: its transposed convolution with weight W_t [ci][co] = w[co][ci] * scale[co],
    pre-multiplied by sqrt(9 * depth) to cancel the kernel's 1 / sqrt(9 cin)."""
    depth, cin = w.shape[0], w.shape[1]
    wt = ((w.double() * out_scale[:, None, None, None]).transpose(0, 1) * math.sqrt(9.0 * depth)).float().contiguous()    # [cin][depth][3][3]
    whi = torch.empty((1, (depth + 15) // 16, 9, 2, cin, 8), dtype=torch.int16, device=w.device)
    wlo = torch.empty_like(whi)
    lib().call("e4s_modconv_prep_weights_sb", _p(whi), _p(wlo), None, _p(wt), None, cin, depth, 0, _stream())
    return whi, wlo


class PreparedIdNet(PreparedNet):
    """The kernels' copies of the ArcFace weights, rebuilt when a tensor changes version or storage: per unit the input BN's scale / shift, three-way
    split slabs of both convolutions (the second with its BN folded in) and of the shortcut convolution, two-way split slabs of their data gradients
    (BN scales folded in), the SE and PReLU weights; the output layer folded into one weight and bias."""

    __slots__ = ()

    _entry, _net = "id_loss", _ID_NET

    def _build(self, sd, variant, dev):
        s0, t0 = bn_fold(sd, "input_layer.1")
        w0 = sd["input_layer.0.weight"]
        inp = (prep_fwd(w0, s0, t0), prep_dgrad(w0, out_scale=s0), sd["input_layer.2.weight"])
        us = []
        for i, (cin, depth, stride) in enumerate(units()):
            p = f"body.{i}."
            s1, t1 = bn_fold(sd, p + "res_layer.0")
            w1, w2 = sd[p + "res_layer.1.weight"], sd[p + "res_layer.3.weight"]
            s2, t2 = bn_fold(sd, p + "res_layer.4")
            fwd1, _ = prep_fwd(w1)
            fwd2 = prep_fwd(w2, s2, t2)
            bwd2 = _prep_tconv(w2, s2) if stride == 2 else prep_dgrad(w2, out_scale=s2)
            sc = None
            if cin != depth:
                ssc, tsc = bn_fold(sd, p + "shortcut_layer.1")
                wsc = sd[p + "shortcut_layer.0.weight"]
                sc = (prep_fwd(wsc, ssc, tsc), prep_dgrad(wsc, out_scale=ssc))
            us.append(dict(cin=cin, depth=depth, stride=stride, bn_scale=s1.float().contiguous(), bn_shift=t1.float().contiguous(), fwd1=fwd1,
                           bwd1=prep_dgrad(w1, in_scale=s1), slope=sd[p + "res_layer.2.weight"], fwd2=fwd2, bwd2=bwd2,
                           fc1=sd[p + "res_layer.5.fc1.weight"].reshape(depth // 16, depth).contiguous(),
                           fc2=sd[p + "res_layer.5.fc2.weight"].reshape(depth, depth // 16).contiguous(), sc=sc))
        so, to = bn_fold(sd, "output_layer.0")
        s4, t4 = bn_fold(sd, "output_layer.4")
        W = sd["output_layer.3.weight"].double()
        b = sd["output_layer.3.bias"].double()
        so, to = so.repeat_interleave(49), to.repeat_interleave(49)          # BN2d's channel c covers features c * 49 .. c * 49 + 48 (Flatten)
        wout = (W * so[None, :] * s4[:, None]).float().contiguous()
        bout = (((W * to[None, :]).sum(1) + b) * s4 + t4).float().contiguous()
        return inp, tuple(us), wout, bout


def prepare(weights):
    """Prepared copies for ``weights`` (cached on a module; a plain mapping is prepared on every call)."""
    return netweights.prepare(PreparedIdNet, *_checked("id_loss", weights))


# ------------------------------------------------------------------------------------------------ pre-processing operator
def axis_matrix(n: int, pooled: bool, crop) -> np.ndarray:
    """float64 [112, n]: AdaptiveAvgPool(256) (when ``pooled``) -> slice ``crop`` (Python slicing of the 256- or n-long axis) -> AdaptiveAvgPool(112)."""
    P1 = pool_matrix(n, 256) if pooled else np.eye(n)
    m = P1.shape[0]
    lo, hi = min(crop[0], m), min(crop[1], m)
    if hi - lo < 1:
        raise ValueError(f"an image side of {n} leaves nothing of the crop {crop}")
    return pool_matrix(hi - lo, SIDE) @ P1[lo:hi]


def resampler(h: int, w: int, device):
    """The pre-processing operator of an h x w image (a cached ``lossnet.Resampler`` to 112 x 112)."""
    pooled = h != 256                           # IDLoss.extract_feats pools when x.shape[2] != 256 (both sides, to 256 x 256)
    return lossnet.resampler(h, w, SIDE, device, lambda: (axis_matrix(h, pooled, CROP[0]), axis_matrix(w, pooled, CROP[1])))


# ------------------------------------------------------------------------------------------------ forward
def _affine(x, scale, shift, slope):
    out = torch.empty_like(x)
    lib().call("e4s_id_affine", _p(out), _p(x), _p(scale), _p(shift), _p(slope), x.shape[0], x.shape[1], x.shape[2] * x.shape[3], _stream())
    return out


def _unit_fwd(x, U):
    bs = x.shape[0]
    depth, stride = U["depth"], U["stride"]
    a = _affine(x, U["bn_scale"], U["bn_shift"], None)
    c1 = conv_sb(a, U["fwd1"], k=3)                                                # PReLU's pre-activation, kept for the backward
    r = conv_sb(_affine(c1, None, None, U["slope"]), *U["fwd2"], k=3, stride=stride)
    ho, wo = r.shape[2], r.shape[3]
    pooled = torch.empty((bs, depth), dtype=torch.float32, device=x.device)
    lib().call("e4s_plane_stats", _p(pooled), None, None, _p(r), bs * depth, ho * wo, 0.0, _stream())
    gate = torch.empty((bs, depth), dtype=torch.float32, device=x.device)
    lib().call("e4s_se_gate", _p(gate), _p(pooled), _p(U["fc1"]), _p(U["fc2"]), bs, depth, depth // 16, _stream())
    if U["sc"] is not None:
        short, sc_stride = conv_sb(x, *U["sc"][0], k=1, stride=stride), 1
    else:
        short, sc_stride = x, stride
    y = torch.empty_like(r)
    lib().call("e4s_norm_gate_add", _p(y), _p(r), None, None, _p(gate), _p(short), None, None, sc_stride, None, bs, depth, ho, wo, _stream())
    return y, (c1, r, pooled, gate)


def _features(x112, P, multiscale: bool, save: bool):
    """The features (flattened, not normalised) of the 112 x 112 input: [tap 2, 6, 20, 23 outputs,] output layer; and what the backward needs."""
    inp, us, wout, bout = P
    bs = x112.shape[0]
    c0 = conv_sb(x112, *inp[0], k=3)
    a = _affine(c0, None, None, inp[2])
    taps, saved = [], []
    for i, U in enumerate(us):
        a, rec = _unit_fwd(a, U)
        if save:
            saved.append(rec)
        if multiscale and i in TAP_UNITS:
            taps.append(a.reshape(bs, -1))
    feat = torch.empty((bs, 512), dtype=torch.float32, device=x112.device)
    lib().call("e4s_id_linear", _p(feat), _p(a), _p(wout), _p(bout), bs, wout.shape[1], 512, _stream())
    taps.append(feat)
    return taps, (c0, saved)


# ------------------------------------------------------------------------------------------------ backward
def _unit_bwd(gy, U, rec, bs, h, w):
    """d loss / d (unit input) from ``gy`` = d loss / d (unit output)."""
    c1, r, pooled, gate = rec
    depth, stride, cin = U["depth"], U["stride"], U["cin"]
    ho, wo = r.shape[2], r.shape[3]
    dr = torch.empty_like(r)
    tmp = torch.empty((2, bs, depth), dtype=torch.float32, device=gy.device)
    lib().call("e4s_id_se_bwd", _p(dr), _p(tmp[0]), _p(tmp[1]), _p(gy), _p(r), _p(pooled), _p(gate), _p(U["fc1"]), _p(U["fc2"]), bs, depth, depth // 16,
               ho * wo, _stream())
    gc1 = torch.empty_like(c1)
    if stride == 2:
        z = torch.empty((bs, depth, 2 * ho + 1, 2 * wo + 1), dtype=torch.float32, device=gy.device)
        ones = torch.ones((bs, 1, depth), dtype=torch.float32, device=gy.device)
        lib().call("e4s_modconv_tconv_sb", _p(z), _p(dr), _p(U["bwd2"][0]), _p(U["bwd2"][1]), _p(ones), bs, depth, depth, ho, wo, _stream())
        src, sh, sw, off = z, 2 * ho + 1, 2 * wo + 1, 1                     # the forward's padding of 1: rows / columns 1 .. 2 ho of the full transposed conv
    else:
        src, sh, sw, off = conv_sb(dr, U["bwd2"], k=3), h, w, 0
    lib().call("e4s_id_prelu_bwd", _p(gc1), _p(src), _p(c1), _p(U["slope"]), bs, depth, h, w, sh, sw, off, _stream())
    if stride == 1:
        return conv_sb(gc1, U["bwd1"], k=3, residual=gy)                        # MaxPool2d(1, 1) shortcut: the identity
    gx = conv_sb(gc1, U["bwd1"], k=3)
    gsc = conv_sb(gy, U["sc"][1], k=1) if U["sc"] is not None else gy           # the 1x1 stride-2 shortcut's data gradient at its output resolution
    lib().call("e4s_id_scatter_add", _p(gx), _p(gsc), bs * cin, h, w, _stream())
    return gx


def _input_grad(fx, fy, stats, gout, P, state, multiscale: bool, head_bwd=None):
    """d loss / d (the 112 x 112 input).  ``head_bwd(g, k, scale, accumulate)``: writes (adds) tap k's head gradient to ``g`` in place of the
    single-target head (the multi-target loss)."""
    inp, us, wout, _ = P
    c0, saved = state
    bs = c0.shape[0]
    scale = 1.0 / bs
    if head_bwd is None:
        def head_bwd(g, k, scale, accumulate):
            lib().call("e4s_id_head_bwd", _p(g), _p(fx[k]), _p(fy[k]), _p(stats[k]), _p(gout), bs, fx[k].shape[1], scale, accumulate, _stream())
    gfeat = torch.empty_like(fx[-1])
    head_bwd(gfeat, len(fx) - 1, scale, 0)
    g = torch.empty((bs, 512, 7, 7), dtype=torch.float32, device=c0.device)
    lib().call("e4s_id_linear_t", _p(g), _p(gfeat), _p(wout), bs, wout.shape[1], 512, _stream())
    taps = {u: k for k, u in enumerate(TAP_UNITS)} if multiscale else {}
    h = w = 7
    for i in range(len(us) - 1, -1, -1):
        if i in taps:
            head_bwd(g, taps[i], scale, 1)
        U = us[i]
        h, w = h * U["stride"], w * U["stride"]
        g = _unit_bwd(g, U, saved[i], bs, h, w)
    gc0 = torch.empty_like(c0)
    lib().call("e4s_id_prelu_bwd", _p(gc0), _p(g), _p(c0), _p(inp[2]), bs, 64, SIDE, SIDE, SIDE, SIDE, 0, _stream())
    return conv_sb(gc0, inp[1], k=3)


class _IdLoss(torch.autograd.Function):
    """(loss, sim_improvement) of IDLoss.forward(y_hat, y); differentiable in ``y_hat`` only (the reference detaches ``y``'s features)."""

    @staticmethod
    def forward(ctx, y_hat, y, P, R, multiscale):
        fx, state = _features(R.apply(y_hat), P, multiscale, save=True)
        fy, _ = _features(R.apply(y), P, multiscale, save=False)
        loss, sim, stats = cos_heads(fx, fy)
        ctx.P, ctx.R, ctx.multiscale, ctx.shape, ctx.state = P, R, multiscale, tuple(y_hat.shape), state
        ctx.save_for_backward(stats, *fx, *fy)
        ctx.mark_non_differentiable(sim, stats)
        return loss, sim, stats

    @staticmethod
    def backward(ctx, gloss, gsim, gstats):
        if gloss is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        saved = ctx.saved_tensors
        n = (len(saved) - 1) // 2
        stats, fx, fy = saved[0], list(saved[1:1 + n]), list(saved[1 + n:])
        gout = _c(gloss.reshape(1), "grad_output")
        g112 = _input_grad(fx, fy, stats, gout, ctx.P, ctx.state, ctx.multiscale)
        return ctx.R.adjoint(g112, ctx.shape), None, None, None, None


def _feature_dims(multiscale: bool):
    """Per-sample sizes of the features: the outputs of the TAP_UNITS (with ``multiscale``), then the 512-d embedding."""
    dims, side = [], SIDE
    for i, (_, depth, stride) in enumerate(units()):
        side //= stride
        if multiscale and i in TAP_UNITS:
            dims.append(depth * side * side)
    return dims + [512]


class _IdLossMulti(torch.autograd.Function):
    """sum_j tw[j] IDLoss(y_hat, y_j) from the targets' cached features; differentiable in ``y_hat`` only."""

    @staticmethod
    def forward(ctx, y_hat, P, R, multiscale, ys, tw, frame):
        fx, state = _features(R.apply(y_hat), P, multiscale, save=True)
        loss, stats = heads_multi(fx, ys, tw, frame)
        ctx.P, ctx.R, ctx.multiscale, ctx.shape, ctx.state, ctx.ys, ctx.tw, ctx.frame = P, R, multiscale, tuple(y_hat.shape), state, ys, tw, frame
        ctx.save_for_backward(stats, *fx)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None, None
        saved = ctx.saved_tensors
        stats, fx = saved[0], list(saved[1:])
        gout = _c(gloss.reshape(1), "grad_output")
        bs = fx[0].shape[0]

        def head_bwd(g, k, scale, accumulate):
            lib().call("e4s_id_head_bwd_multi", _p(g), _p(fx[k]), *call_args([y[k] for y in ctx.ys], ctx.tw, ctx.frame, bs), _p(stats[k]), _p(gout), bs,
                       fx[k].shape[1], scale, accumulate, _stream())
        g112 = _input_grad(fx, None, None, gout, ctx.P, ctx.state, ctx.multiscale, head_bwd)
        return ctx.R.adjoint(g112, ctx.shape), None, None, None, None, None, None


def target_features(images: torch.Tensor, weights, multiscale: bool = True):
    """The raw (not normalised) features of ``images`` ``[n, 3, H, W]`` that ``id_loss_multi`` reads for a target: a list of ``[n, D]`` tensors
    (five with ``multiscale``, the embedding alone without).  Computed a frame at a time; no gradient."""
    W = _checked("ops_id.target_features", weights)
    images = check_image(images.detach(), "images")
    P, R = netweights.prepare(PreparedIdNet, *W), resampler(images.shape[2], images.shape[3], images.device)
    with torch.no_grad():
        return target_rows(lambda x: _features(R.apply(x.contiguous()), P, bool(multiscale), save=False)[0], images)


def id_loss_multi(y_hat: torch.Tensor, targets, tw, weights, multiscale: bool = True, frame: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sum_j tw[j] * id_loss(y_hat, y_j)`` (0-d, differentiable in ``y_hat`` only) with one network pass and input gradient of ``y_hat``:
    ``targets[j] = target_features(y_j, weights, multiscale)`` (``bs`` rows, or frames x ``bs`` rows with ``frame``, a device int32 frame index)."""
    W = _checked("id_loss_multi", weights)
    y_hat = check_image(y_hat, "y_hat")
    frame = check_frame(frame, y_hat.device)
    bs = y_hat.shape[0]
    ys = check_targets([torch.empty((bs, d), device="meta") for d in _feature_dims(multiscale)], targets, tw, frame, "id_loss_multi")
    return _IdLossMulti.apply(y_hat, netweights.prepare(PreparedIdNet, *W), resampler(y_hat.shape[2], y_hat.shape[3], y_hat.device), bool(multiscale), ys,
                              [float(w) for w in tw], frame)


def id_loss_terms(y_hat: torch.Tensor, y: torch.Tensor, weights, multiscale: bool = True):
    """``(loss, sim_improvement, per_scale)``: the loss (0-d, differentiable in ``y_hat``), IDLoss's similarity improvement (0-d, on the device) and
    ``per_scale [scales]`` = mean over the batch of 1 - cos per scale (no gradient).  No host synchronisation."""
    W = _checked("id_loss", weights)
    y_hat, y = check_image(y_hat, "y_hat"), check_image(y.detach(), "y")
    if y_hat.shape != y.shape:
        raise ValueError(f"y_hat {tuple(y_hat.shape)} and y {tuple(y.shape)} differ")
    loss, sim, stats = _IdLoss.apply(y_hat, y, netweights.prepare(PreparedIdNet, *W), resampler(y.shape[2], y.shape[3], y.device), bool(multiscale))
    return loss, sim, (1.0 - stats[..., 2]).mean(1)


def id_loss(y_hat: torch.Tensor, y: torch.Tensor, weights, multiscale: bool = True) -> torch.Tensor:
    """IDLoss.forward(y_hat, y)'s loss (a 0-d tensor): ``sum over scales of mean_i (1 - cos(f(y_hat_i), f(y_i)))``, five scales with ``multiscale``
    (body units 2, 6, 20, 23 and the 512-d embedding), the embedding alone without.  ``y_hat``, ``y``: fp32 ``[bs, 3, H, W]`` on the device, pooled
    to 256 x 256 unless H is 256, cropped and pooled to 112 x 112 as IDLoss.extract_feats does.  Differentiable in ``y_hat`` only."""
    return id_loss_terms(y_hat, y, weights, multiscale)[0]


def _features_112(x, W, multiscale):
    x = check_image(x, "x")
    if x.shape[2:] != (SIDE, SIDE):
        raise ValueError(f"x: the network takes 112 x 112 inputs, got {tuple(x.shape[2:])}")
    with torch.no_grad():
        taps, _ = _features(x, netweights.prepare(PreparedIdNet, *W), multiscale, save=False)
    return [t / t.norm(dim=1, keepdim=True) for t in taps]


def features_112(x: torch.Tensor, weights, multiscale: bool = True):
    """Backbone.forward(x, multi_scale): the l2-normalised features of a 112 x 112 input (no gradient)."""
    return _features_112(x, _checked("features_112", weights), multiscale)


def id_features(x: torch.Tensor, weights, multiscale: bool = True):
    """IDLoss.extract_feats(x): the l2-normalised features of an image batch after the pool -> crop -> pool pre-processing (no gradient)."""
    W = _checked("id_features", weights)
    x = check_image(x, "x")
    with torch.no_grad():
        x112 = resampler(x.shape[2], x.shape[3], x.device).apply(x)
    return _features_112(x112, W, multiscale)


__all__ = ["IdNet", "PreparedIdNet", "check_loaded", "weights_key", "weight_tensors", "prepare", "state_dict_keys", "state_dict_shapes", "axis_matrix", "resampler",
           "id_features", "features_112", "id_loss", "id_loss_terms", "units", "target_features", "id_loss_multi", "heads_multi"]
