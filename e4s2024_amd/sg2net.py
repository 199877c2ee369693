"""What the two StyleGAN2 generators behind a strided-convolution encoder (``ops_gpen``, row f12; ``ops_inpaint``, row f25) have in common on the host side: the
modules that mirror the reference's ``state_dict`` keys, the stock-PyTorch restatement of their layers, weight preparation for and the calls of the library
entries both run on (``e4s_conv2d[_sb]`` through ``lossnet``, ``e4s_upfirdn2d``, ``e4s_style_demod_batched``, ``e4s_region_modconv3x3[_sb]``,
``e4s_modconv_up_fused_sb``, ``e4s_region_torgb``).  Nothing network-specific: key names that differ, the noise handling, the condition tables and the buffers
stay with each network, and so do ``ARITH`` and ``UP_COMPOSED_MAX_WIDTH``, which come in as arguments.  The library is resolved inside the calls only, so the
module imports on a machine without it."""
from __future__ import annotations

import ctypes
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lossnet
from ._lib import MAX_STYLE_JOBS, StyleJob, lib
from .ops import _p, _stream, _workspace, SPLITK_MAX_OUT_FLOATS

SQRT2 = math.sqrt(2.0)
_FIR = (1.0, 3.0, 3.0, 1.0)


# ------------------------------------------------------------------------------------------------ the modules: the reference's keys
class Bias(nn.Module):
    """``FusedLeakyReLU``: its bias."""

    def __init__(self, c):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(c))


class EqualLinear(nn.Module):
    def __init__(self, in_dim, out_dim, bias_init=0.0, lr_mul=1.0):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(out_dim, in_dim).div_(lr_mul))
        self.bias = nn.Parameter(torch.zeros(out_dim).fill_(bias_init))
        self.lr_mul = lr_mul
        self.scale = (1 / math.sqrt(in_dim)) * lr_mul


class EqualConv(nn.Module):
    def __init__(self, cin, cout, k=3, bias=False):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin, k, k))
        if bias:
            self.bias = nn.Parameter(torch.zeros(cout))


class Fir(nn.Module):
    """``Blur`` / ``Upsample``: the FIR buffer ``kernel``."""

    def __init__(self, gain: float = 1.0):
        super().__init__()
        self.register_buffer("kernel", _fir(gain))                                             # (not the cached one: a module may be built on the meta device)


class ModConv(nn.Module):
    """``ModulatedConv2d``; with ``blur_gain`` (GPEN's up layers) the ``blur`` FIR buffer comes before ``weight``."""

    def __init__(self, cin, cout, k, style_dim, blur_gain=None):
        super().__init__()
        if blur_gain is not None:
            self.blur = Fir(blur_gain)
        self.weight = nn.Parameter(torch.randn(1, cout, cin, k, k))
        self.modulation = EqualLinear(style_dim, cin, bias_init=1.0)


# ------------------------------------------------------------------------------------------------ the layers on stock PyTorch
def flrelu(x, bias):
    return F.leaky_relu(x + bias.view((1, -1) + (1,) * (x.dim() - 2)), 0.2) * SQRT2


def _fir(gain=1.0, device=None):
    k = torch.tensor(_FIR, dtype=torch.float32, device=device)
    k = k[None, :] * k[:, None]
    k = k / k.sum()
    return k * gain if gain != 1.0 else k


@functools.lru_cache(maxsize=None)
def fir(gain=1.0, device=None):
    """The 4 x 4 FIR times ``gain`` on ``device``, made once per device (no host-to-device copy inside a captured forward); read-only."""
    return _fir(gain, device)


def upfirdn(x, k, up, pad):
    bs, c, h, w = x.shape
    if up > 1:
        z = x.new_zeros(bs, c, h, up, w, up)
        z[:, :, :, 0, :, 0] = x
        x = z.reshape(bs, c, h * up, w * up)
    x = F.pad(x, (pad[0], pad[1], pad[0], pad[1]))
    out = F.conv2d(x.reshape(bs * c, 1, x.shape[2], x.shape[3]), torch.flip(k, [0, 1])[None, None])
    return out.reshape(bs, c, out.shape[2], out.shape[3])


def torch_modconv(sd, p, x, w, up=False, demodulate=True, blur=None):
    """``ModulatedConv2d`` under the prefix ``p`` with the style ``w [bs, style_dim]``; an up layer blurs with ``blur``, the FIR times 4."""
    W = sd[p + ".weight"][0]
    cout, cin, k, _ = W.shape
    s = F.linear(w, sd[p + ".modulation.weight"] * (1 / math.sqrt(w.shape[1])), sd[p + ".modulation.bias"])
    Wm = (1 / math.sqrt(cin * k * k)) * W[None] * s[:, None, :, None, None]
    if demodulate:
        Wm = Wm * torch.rsqrt(Wm.pow(2).sum([2, 3, 4]) + 1e-8)[:, :, None, None, None]
    bs, _, h, wd = x.shape
    xg = x.reshape(1, bs * cin, h, wd)
    if up:
        out = F.conv_transpose2d(xg, Wm.transpose(1, 2).reshape(bs * cin, cout, k, k), stride=2, groups=bs)
        return upfirdn(out.reshape(bs, cout, out.shape[2], out.shape[3]), blur, 1, (1, 1))
    return F.conv2d(xg, Wm.reshape(bs * cout, cin, k, k), padding=k // 2, groups=bs).reshape(bs, cout, h, wd)


# ------------------------------------------------------------------------------------------------ weights
def use_composed(arith: str, max_width: int, w_in: int) -> bool:
    """Whether an up layer with a ``w_in`` wide input takes the parity-composed, split-K form (the exact-fp32 arithmetic has no other)."""
    return arith != "sb" or w_in <= max_width


def arith_checked(name, module_name, arith):
    if arith not in ("sb", "f32"):
        raise ValueError(f"{name}: {module_name}.ARITH is 'sb' or 'f32', got {arith!r}")


def prep_conv3x3(W, bias, gain, sb, slope):
    """A plain 3 x 3 convolution with EqualConv's scale and ``gain`` (sqrt(2) of a fused leaky-relu, which is positively homogeneous) folded into weight and
    bias in float64: two-way split-bf16 slabs or the K-major fp32 weight, the bias, and with ``slope`` the 0.2 slope vector that makes PReLU the activation."""
    cout, cin = W.shape[:2]
    w = (W.double() * (gain / math.sqrt(cin * 9))).float()
    wt = lossnet.prep_fwd(w, terms=2)[0] if sb else lossnet.prep_exact(w)[0]
    return dict(wt=wt, bias=(bias.double() * gain).float().contiguous(), slope=torch.full((cout,), 0.2, dtype=torch.float32, device=W.device) if slope else None,
                cin=cin, cout=cout)


def prep_styled(W, blur, composed, sb):
    """(weight, ``wsq`` table) of the 3 x 3 modulated convolution ``W [1, cout, cin, 3, 3]``: split-bf16 slabs or the K-major fp32 weight, four parity
    weights composed with ``blur`` for a ``composed`` up layer."""
    _, cout, cin, _, _ = W.shape
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=W.device)      # noqa: E731
    wsq = new((cin, cout))
    if sb:
        shape = (4 if composed else 1, (cin + 15) // 16, 9, 2, cout, 8)
        wt = (new(shape, torch.int16), new(shape, torch.int16))
        lib().call("e4s_modconv_prep_weights_sb", _p(wt[0]), _p(wt[1]), _p(wsq), _p(W), _p(blur) if composed else None, cout, cin, 1 if composed else 0, _stream())
    else:
        wt = new((4 if composed else 1, cin, 9, cout))
        lib().call("e4s_modconv_prep_weights", _p(wt), _p(wsq), _p(W), _p(blur) if composed else None, cout, cin, 3, 1 if composed else 0, _stream())
    return wt, wsq


def prep_rgb(W):
    """The ``k = 1`` weight ``[1, cin, 1, 3]`` of a ToRGB's modulated convolution ``W [1, 3, cin, 1, 1]``."""
    cin = W.shape[2]
    wt = torch.empty((1, cin, 1, 3), dtype=torch.float32, device=W.device)
    lib().call("e4s_modconv_prep_weights", _p(wt), None, _p(W), None, 3, cin, 1, 0, _stream())
    return wt


# ------------------------------------------------------------------------------------------------ calls
def conv3x3(L, x, out, bs, h, sb, st, fir=None, scratch=None):
    """The plain 3 x 3 convolution ``L`` (``prep_conv3x3``) of the batch ``x [bs, cin, h, h]`` into ``out`` on the stream ``st``: pad 1, or for a ``fir`` the
    4 x 4 FIR with pad (2, 2) into ``scratch [bs, cin, h + 1, h + 1]`` (made here without one), then stride 2 without padding."""
    stride, pad = 1, 1
    if fir is not None:
        if scratch is None:
            scratch = torch.empty((bs, L["cin"], h + 1, h + 1), dtype=torch.float32, device=x.device)
        lib().call("e4s_upfirdn2d", _p(scratch), _p(x), _p(fir), bs * L["cin"], h, h, 4, 4, 1, 1, 1, 1, 2, 2, 2, 2, st)
        x, stride, pad = scratch, 2, 0
    (lossnet.conv_sb if sb else lossnet.conv_exact)(x, L["wt"], L["bias"], k=3, stride=stride, pad=pad, slope=L["slope"], out=out, stream=st)


def style_tables(layers, styles, bs, sdim, s_buf, d_buf):
    """Every layer's style table ``s [bs * cin]`` and, for a layer with a ``wsq``, demodulation table ``d [bs * cout]``, cut from ``s_buf`` and ``d_buf`` in
    layer order and filled in one batched pass.  ``styles``: per layer (address of the first sample's style vector, its sample stride, its region stride).
    Returns [(s, d)] for the convolutions and [s] for the ToRGBs."""
    arr = (StyleJob * len(layers))()
    so = do = 0
    conv_t, rgb_t = [], []
    for i, (L, (ptr, stride0, stride1)) in enumerate(zip(layers, styles)):
        s_t = s_buf[so:so + bs * L["cin"]]
        so += bs * L["cin"]
        d_t = None
        if "wsq" in L:
            d_t = d_buf[do:do + bs * L["cout"]]
            do += bs * L["cout"]
            conv_t.append((s_t, d_t))
        else:
            rgb_t.append(s_t)
        arr[i] = StyleJob(s_t.data_ptr(), None if d_t is None else d_t.data_ptr(), ptr, stride0, stride1, L["mw"].data_ptr(), L["mb"].data_ptr(),
                          None if d_t is None else L["wsq"].data_ptr(), 1, L["cin"], L.get("cout", 3), 0)
    for i0 in range(0, len(layers), MAX_STYLE_JOBS):
        lib().call("e4s_style_demod_batched", ctypes.byref(arr, i0 * ctypes.sizeof(StyleJob)), min(MAX_STYLE_JOBS, len(layers) - i0), bs, sdim, _stream())
    return conv_t, rgb_t


def _region_modconv(L, x, out, s, d, sb, nz, bias, act, n, h, ws, wsn, st):
    up = 1 if L["up"] else 0
    if sb:
        lib().call("e4s_region_modconv3x3_sb", _p(out), _p(x), _p(L["wt"][0]), _p(L["wt"][1]), _p(s), _p(d), None, 0, 0, *nz, _p(bias), act,
                   n, L["cin"], L["cout"], h, h, 1, up, _p(ws), wsn, None, None, None, None, None, None, None, None, None, st)
    else:
        lib().call("e4s_region_modconv3x3", _p(out), _p(x), _p(L["wt"]), _p(s), _p(d), None, 0, 0, *nz, _p(bias), act, n, L["cin"], L["cout"], h, h, 1, up,
                   _p(ws), wsn, st)


def modconv(L, x, out, s, d, *, sb, blur, noise=None, bias, act, bs, h, st):
    """The single-region modulated convolution ``L`` (``prep_styled``'s weight, ``up``, ``composed``, ``cin``, ``cout``; ``nw`` with a noise map) of
    ``x [bs, cin, h, h]`` into ``out`` with the tables ``s [bs * cin]``, ``d [bs * cout]`` on the stream ``st``: the one-launch up entry with ``blur``, or the
    parity-composed / same-resolution entry.  ``noise``: None or ``[bs or 1, 1, ho, ho]``, added times the device scalar ``L["nw"]``; ``bias``, ``act``: the
    entry's epilogue."""
    cin, cout = L["cin"], L["cout"]
    nz = (None, 0, None) if noise is None else (_p(noise), noise.shape[0], _p(L["nw"]))
    if L["up"] and not L["composed"]:
        lib().call("e4s_modconv_up_fused_sb", _p(out), _p(x), _p(L["wt"][0]), _p(L["wt"][1]), _p(s), _p(d), _p(blur), *nz, _p(bias), act, bs, cin, cout, h, h,
                   None, st)
        return
    ho = 2 * h if L["up"] else h
    if cout * ho * ho > SPLITK_MAX_OUT_FLOATS:
        _region_modconv(L, x, out, s, d, sb, nz, bias, act, bs, h, None, 0, st)
        return
    # a map small enough for split-K: the entry picks the number of K slices from its grid, the batch included, and the slices set the order of the sums.  Sample
    # by sample every call is a batch-of-one call (and fills the chip through its slices), so a sample gets the bits it gets alone
    wsn = 16 * cout * ho * ho
    ws = _workspace(x.device, wsn)
    if bs == 1:
        _region_modconv(L, x, out, s, d, sb, nz, bias, act, 1, h, ws, wsn, st)
        return
    per_sample = noise is not None and noise.shape[0] == bs
    for b in range(bs):
        if per_sample:
            nz = (_p(noise[b:b + 1]), 1, nz[2])
        _region_modconv(L, x[b:b + 1], out[b:b + 1], s[b * cin:(b + 1) * cin], d[b * cout:(b + 1) * cout], sb, nz, bias, act, 1, h, ws, wsn, st)


def torgb(R, x, s, skip, upk, out, bs, h, st):
    """The ToRGB ``R`` (``prep_rgb``'s weight, ``bias [3]``, ``cin``) of ``x [bs, cin, h, h]`` into ``out [bs, 3, h, h]`` on the stream ``st``;
    ``skip [bs, 3, h / 2, h / 2]`` or None is upsampled with the FIR ``upk`` and added."""
    lib().call("e4s_region_torgb", _p(out), _p(x), _p(R["wt"]), _p(s), None, 0, 0, _p(R["bias"]), _p(skip), _p(upk) if skip is not None else None,
               bs, R["cin"], h, h, 1, st)
