"""Row f25: face inpainting, stage 1 — the GCFSR inpainting generator, ``FaceInpaintingArch`` of swap_face_fine/gcfsr_arch.py:1347-1540, in eval mode, and the
whole of ``inpainting(face_img, mask)`` (swap_face_fine/face_inpainting.py:21-51) between its two resizes: ``inpaint_forward``, ``inpaint_image``.  Stage 2 (the
rest of ``_inpaint_face``, Face_swap_with_two_imgs.py:293-336: ``cv2.dilate``, the Gaussian blurs on uint8 masks, the chain into ``codeformer_enhance``,
``pil_resize`` and ``blend_with_mask``, and the wiring into ``pipeline.swap_images``) is not here.

The network is a StyleGAN2 synthesis network that starts at the encoder's 16 x 16 feature, behind a strided-convolution encoder, with one latent row per
layer, and one new element: every second style convolution scales its output by a normalised pair of condition scales, adds a scaled shift map made from the
encoder feature of its resolution, and only then applies bias and activation.  The whole batch runs at once (nothing is concatenated, so every entry takes
``bs``), except the modulated convolutions on maps small enough for split-K (up to 64 x 64 at 512 channels), which run sample by sample: that entry picks its
number of K slices from its grid, the batch included, so only a batch-of-one call gives a sample the bits it gets alone.  The contractions run on kernels the
library has, the rest on csrc/gcfsr.hip.  The key-mirror modules, the stock restatement of the layers, the weight preparation and the calls it shares with
``ops_gpen`` are ``sg2net``'s:

    conv_body_first, final_conv   e4s_conv2d_sb / e4s_conv2d (3 x 3, pad 1): sqrt(2) of the fused activation folded into weight and bias in float64, PReLU with a
                                  0.2 slope vector is then FusedLeakyReLU exactly (as ``ops_gpen``'s encoder levels)
    conv_body_down, final_down1/2 e4s_upfirdn2d (4 x 4 FIR, pad (2, 2)), then the strided convolution, the same folding
    final_linear                  e4s_grouped_linear (groups = 1, act = 2) on the channel-major flattening of the 4 x 4 map: the ``num_latent`` latent rows
    tables                        every layer's style and demodulation tables in one batched pass (``sg2net.style_tables``); layer i reads ``latent[:, i]``
    condition_scale1/2, Norm2Scale  e4s_gcfsr_condition: every level in one launch
    condition_shift               e4s_conv2d_sb / e4s_conv2d with bias, no activation, on the encoder feature of each level
    StyleConv (the up layers)     e4s_region_modconv3x3_sb(up = 1) for inputs up to ``UP_COMPOSED_MAX_WIDTH`` wide, e4s_modconv_up_fused_sb above; the noise map
                                  ``[bs or 1, 1, h, w]`` with the device scalar ``weight``, bias and activation in the entry
    StyleConv_norm_scale_shift    the same-resolution modulated convolution with its noise, no bias and no activation, then e4s_gcfsr_scale_shift_act in place
    ToRGB                         e4s_region_torgb, which chains the skips through the FIR upsampling; latent rows 1, then 2 j + 3

``ARITH`` (module attribute): ``"sb"``, the default, runs the convolutions on the two-way split-bf16 entries (bar: 1e-3 on the raw output); ``"f32"`` on the
exact-fp32 entries, with every up layer in the parity-composed form.  The linear layer, the tables, the condition, the epilogue, ToRGB and the ends are float32 in
both.  ``UP_COMPOSED_MAX_WIDTH`` as in ``ops_gpen``; both enter the prepared-weights key.

Noise.  The reference's stored ``noises.noise{i}`` buffers have the wrong resolutions (4, 8, 8, 16, ... for layers that run at 16, 32, 32, 64, ...), so its
``randomize_noise=False`` raises; its caller never passes the flag and every call draws fresh normal noise.  The buffers are kept here at their reference shapes
so that the checkpoint loads with ``strict=True``, and are never read.  ``inpaint_forward(noise=None)`` draws the maps with ``torch.randn(..., generator=generator)``
on the device in layer order: reproducible under a seeded generator, never bit-equal to the reference's own draws.

``cv_mask_support`` restates the support of ``cv2.resize`` on the mask; cv2 itself has never been run against it (no tree here has it), and negative or NaN mask
values are outside the rule.

Forward only; no host synchronisation; the same inputs give the same bits, and a sample of a batch gets the bits it gets alone; after one eager call (which
prepares the weights) a call with explicit noise captures in a graph."""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import netweights, sg2net
from ._lib import lib
from .ops import _p, _stream, grouped_linear
from .netweights import PreparedNet, _Net, _cuda_checked, _keys_shapes, _placed_checked, _tensor_checked, _validated, module_net, prepare
from .sg2net import SQRT2, Bias, EqualConv, EqualLinear, ModConv, fir, flrelu, torch_modconv, upfirdn

ARITH = "sb"                                 # "sb" | "f32" (module attribute: tests and tools set it)
UP_COMPOSED_MAX_WIDTH = 32                   # up layers with an input at most this wide take the parity-composed, split-K form
STYLE_DIM = 512
INPAINT_MAX_SIDE = 16384                     # the largest mask side ``cv_mask_support`` takes


def inpaint_channels():
    """Channels per resolution at ``channel_multiplier=2, narrow=1`` (gcfsr_arch.py:1359-1369), the one configuration the reference runs at."""
    return {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}


# ------------------------------------------------------------------------------------------------ the module: the reference's keys, a stock-PyTorch forward
def _conv_layer(cin, cout, down=False, activate=True):
    """``ConvLayer``: (the FIR, which has no keys,) the convolution, the activation's bias; without activation the bias is the convolution's."""
    layers = [nn.Identity()] if down else []
    layers.append(EqualConv(cin, cout, bias=not activate))
    if activate:
        layers.append(Bias(cout))
    return nn.Sequential(*layers)


class _StyleConv(nn.Module):
    """``StyleConv`` and ``StyleConv_norm_scale_shift``: the same keys."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1))
        self.modulated_conv = ModConv(cin, cout, 3, STYLE_DIM)
        self.activate = Bias(cout)


class _ToRGB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))
        self.modulated_conv = ModConv(cin, 3, 1, STYLE_DIM)


def _size_checked(out_size):
    if isinstance(out_size, bool) or not isinstance(out_size, int) or out_size < 32 or out_size > 1024 or out_size & (out_size - 1):
        raise ValueError(f"FaceInpainting: out_size is a power of two in 32..1024, got {out_size!r}")
    return int(math.log2(out_size))


class FaceInpainting(nn.Module):
    """``FaceInpaintingArch(out_size)`` of swap_face_fine/gcfsr_arch.py with its ``state_dict`` keys, shapes and order (``net_g_50000.pth``'s ``params_ema``
    loads with ``strict=True`` at 256); ``num_style_feat=512, channel_multiplier=2, narrow=1``: the reference's ``final_linear`` is hard-coded to them.  The three
    FIR kernels are plain attributes in the reference, not keys; the ``noises.noise{i}`` buffers keep their (wrong) reference shapes and are never read.
    ``forward(x, in_size, noise)`` is the plain PyTorch composition in eval mode — what the tests and the timing compare ``inpaint_forward`` with;
    ``inpaint_forward(x, in_size, module)`` runs the same weights on the HIP kernels.  It starts with random weights and ``inpaint_forward`` refuses it until
    ``load_state_dict`` has filled it."""

    def __init__(self, out_size: int = 256):
        super().__init__()
        self.log_size = _size_checked(out_size)
        self.out_size, self.num_style_feat = out_size, STYLE_DIM
        self.num_latent = (self.log_size - 2) * 2 - 2
        self.num_layers = (self.log_size - 4) * 2 + 1
        ch = inpaint_channels()
        self.conv_body_first = _conv_layer(4, ch[out_size])
        self.conv_body_down = nn.ModuleList(_conv_layer(ch[2 ** (i + 1)], ch[2 ** i], down=True) for i in range(self.log_size - 1, 3, -1))
        self.final_conv = _conv_layer(ch[16], ch[16])
        self.final_down1 = _conv_layer(ch[16], ch[8], down=True)
        self.final_down2 = _conv_layer(ch[8], ch[4] // 2, down=True)
        self.final_linear = EqualLinear(2 * 4 * 512, STYLE_DIM * self.num_latent)
        levels = [ch[2 ** i] for i in range(self.log_size, 3, -1)]
        self.condition_scale1 = nn.ModuleList(EqualLinear(1, c, bias_init=1.0) for c in levels)
        self.condition_scale2 = nn.ModuleList(EqualLinear(1, c, bias_init=1.0) for c in levels)
        self.condition_shift = nn.ModuleList(_conv_layer(c, c, activate=False) for c in levels)
        self.style_conv1 = _StyleConv(ch[16], ch[16])
        self.to_rgb1 = _ToRGB(ch[16])
        self.style_convs, self.to_rgbs, self.noises = nn.ModuleList(), nn.ModuleList(), nn.Module()
        for i in range(self.num_layers):
            r = 2 ** ((i + 5) // 2)
            self.noises.register_buffer(f"noise{i}", torch.randn(1, 1, r, r))
        cin = ch[16]
        for i in range(5, self.log_size + 1):
            cout = ch[2 ** i]
            self.style_convs.extend([_StyleConv(cin, cout), _StyleConv(cout, cout)])
            self.to_rgbs.append(_ToRGB(cout))
            cin = cout
        self.requires_grad_(False)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if "conv_body_first.0.weight" in state_dict and "final_linear.weight" in state_dict:
            self._loaded = True
        return out

    def forward(self, x, in_size, noise=None, return_latents: bool = False):
        if self.training:
            raise NotImplementedError("FaceInpainting: training mode is not implemented; call .eval()")
        with torch.no_grad():
            if noise is None:
                noise = [torch.randn(x.shape[0], 1, r, r, device=x.device) for r in noise_sizes(self.out_size)]
            image, latent = _torch_forward(dict(self.state_dict()), x, in_size, noise, self.log_size)
        return image, (latent if return_latents else None)


def noise_sizes(out_size: int):
    """The resolutions of the ``num_layers`` noise maps: 16, 32, 32, 64, 64, ..."""
    log_size = _size_checked(out_size)
    return [16] + [2 ** i for i in range(5, log_size + 1) for _ in (0, 1)]


def _torch_conv_layer(sd, p, x, down=False, activate=True):
    i = 1 if down else 0
    W = sd[f"{p}.{i}.weight"]
    w = W * (1 / math.sqrt(W.shape[1] * 9))
    if down:
        y = F.conv2d(upfirdn(x, fir(device=x.device), 1, (2, 2)), w, stride=2)
    else:
        y = F.conv2d(x, w, bias=None if activate else sd[f"{p}.{i}.bias"], padding=1)
    return flrelu(y, sd[f"{p}.{i + 1}.bias"]) if activate else y


def _torch_style_conv(sd, p, x, w, noise, up=False, cond=None):
    out = torch_modconv(sd, p + ".modulated_conv", x, w, up, blur=fir(4.0, x.device) if up else None) + sd[p + ".weight"] * noise
    if cond is not None:
        s1, s2, shift = cond
        n = s1 ** 2 + s2 ** 2 + 1e-8
        s1, s2 = s1 * torch.rsqrt(n), s2 * torch.rsqrt(n)
        out = out * s1.view(-1, out.shape[1], 1, 1) + shift * s2.view(-1, out.shape[1], 1, 1)
    return flrelu(out, sd[p + ".activate.bias"])


def _torch_to_rgb(sd, p, x, w, skip):
    out = torch_modconv(sd, p + ".modulated_conv", x, w, demodulate=False) + sd[p + ".bias"]
    if skip is not None:
        out = out + upfirdn(skip, fir(4.0, x.device), 2, (2, 1))
    return out


def _torch_forward(sd, x, in_size, noise, log_size):
    n_cond = log_size - 3
    bs = x.shape[0]
    c = in_size.reshape(-1, 1)
    feat = _torch_conv_layer(sd, "conv_body_first", x)
    cond = []
    for j in range(n_cond):
        if j:
            feat = _torch_conv_layer(sd, f"conv_body_down.{j - 1}", feat, down=True)
        cond.append((F.linear(c, sd[f"condition_scale1.{j}.weight"], sd[f"condition_scale1.{j}.bias"]),
                     F.linear(c, sd[f"condition_scale2.{j}.weight"], sd[f"condition_scale2.{j}.bias"]),
                     _torch_conv_layer(sd, f"condition_shift.{j}", feat, activate=False)))
    cond = cond[::-1]
    tmp = _torch_conv_layer(sd, "final_down2", _torch_conv_layer(sd, "final_down1", feat, down=True), down=True)
    W = sd["final_linear.weight"]
    latent = flrelu(F.linear(tmp.reshape(bs, -1), W * (1 / math.sqrt(W.shape[1]))), sd["final_linear.bias"]).view(bs, -1, STYLE_DIM)
    out = _torch_conv_layer(sd, "final_conv", feat)
    out = _torch_style_conv(sd, "style_conv1", out, latent[:, 0], noise[0], cond=cond[0])
    skip = _torch_to_rgb(sd, "to_rgb1", out, latent[:, 1], None)
    for j in range(n_cond - 1):
        out = _torch_style_conv(sd, f"style_convs.{2 * j}", out, latent[:, 2 * j + 1], noise[2 * j + 1], up=True)
        out = _torch_style_conv(sd, f"style_convs.{2 * j + 1}", out, latent[:, 2 * j + 2], noise[2 * j + 2], cond=cond[j + 1])
        skip = _torch_to_rgb(sd, f"to_rgbs.{j}", out, latent[:, 2 * j + 3], skip)
    return skip, latent


# ------------------------------------------------------------------------------------------------ weights
def inpaint_state_dict_shapes(out_size: int = 256):
    """``{key: shape}`` of ``FaceInpainting(out_size).state_dict()``, in its order."""
    return dict(_keys_shapes(FaceInpainting, out_size))


def _inpaint_variant(name, sd):
    """(out_size,) read off the keys of ``sd``; a ``narrow`` or ``channel_multiplier`` other than (1, 2) is refused by name."""
    for probe in ("conv_body_first.0.weight", "final_linear.weight", "style_conv1.modulated_conv.weight"):
        t = sd.get(probe)
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise KeyError(f"{name}: the weights lack '{probe}': expected the keys of FaceInpaintingArch (ops.inpaint_state_dict_shapes())")
    levels = 0
    while f"condition_scale1.{levels}.weight" in sd:
        levels += 1
    if not 2 <= levels <= 7:
        raise KeyError(f"{name}: the weights do not describe a FaceInpaintingArch ({levels} condition levels, expected 2..7 for out_size 32..1024)")
    out_size = 2 ** (levels + 3)
    c16, c_top = int(sd["style_conv1.modulated_conv.weight"].shape[1]), int(sd["conv_body_first.0.weight"].shape[0])
    if c16 != 512:
        raise ValueError(f"{name}: narrow: the 16 x 16 level has {c16} channels, {c16 / 512:g} of 512; only narrow = 1 is implemented (the reference's final_linear "
                         "is hard-coded to it)")
    if c_top != inpaint_channels()[out_size]:
        raise ValueError(f"{name}: channel_multiplier: the {out_size} x {out_size} level has {c_top} channels, expected {inpaint_channels()[out_size]} at "
                         "channel_multiplier = 2, the only one implemented")
    return (out_size,)


def _inpaint_shapes(variant):
    return inpaint_state_dict_shapes(*variant)


_INPAINT_NET = _Net("FaceInpaintingArch", _inpaint_shapes, ("module.", "params_ema.", "params."), True, ("conv_body_first.0.weight",), _inpaint_variant,
                    "the native path is the eval-mode forward", ())


def _net_of(weights):
    if not isinstance(weights, FaceInpainting):
        return _INPAINT_NET
    return module_net(_INPAINT_NET, (weights.out_size,))


def inpaint_weight_tensors(weights, name: str = "inpaint_forward"):
    """The tensors of the network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _net_of(weights))[2]


class PreparedInpaint(PreparedNet):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage or the arithmetic changes.  Per plain convolution (FIR or
    None, slabs or K-major fp32 weight, bias, slope vector or None) with sqrt(2) folded into weight and bias in float64 where an activation follows; the
    condition levels' four vectors in decoder order; ``final``: the EqualLinear as it is (its scale is a call argument); per modulated convolution its
    split-bf16 slabs (or K-major fp32 weight), ``wsq`` table, modulation weights, noise weight and activation bias; per ToRGB its ``k = 1`` weight."""

    __slots__ = ()
    _entry = "inpaint_forward"

    def _net(self, weights):
        return _net_of(weights)

    def _settings(self):
        return ARITH, UP_COMPOSED_MAX_WIDTH

    def _build(self, sd, variant, dev):
        out_size, = variant
        log_size = int(math.log2(out_size))
        n_cond = log_size - 3
        sb = ARITH == "sb"
        fir1, fir4 = fir(device=dev).contiguous(), fir(4.0, dev).contiguous()

        def conv(p, down=False, activate=True):
            i = 1 if down else 0
            b = sd[f"{p}.{i + 1}.bias"] if activate else sd[f"{p}.{i}.bias"]
            return dict(sg2net.prep_conv3x3(sd[f"{p}.{i}.weight"], b, SQRT2 if activate else 1.0, sb, activate), fir=fir1 if down else None)

        def styled(p, up, w_in, norm):
            W = sd[p + ".modulated_conv.weight"]
            composed = up and sg2net.use_composed(ARITH, UP_COMPOSED_MAX_WIDTH, w_in)
            wt, wsq = sg2net.prep_styled(W, fir4, composed, sb)
            return dict(wt=wt, wsq=wsq, mw=sd[p + ".modulated_conv.modulation.weight"], mb=sd[p + ".modulated_conv.modulation.bias"], nw=sd[p + ".weight"],
                        bias=sd[p + ".activate.bias"], up=up, composed=composed, norm=norm, cin=W.shape[2], cout=W.shape[1])

        def rgb(p):
            W = sd[p + ".modulated_conv.weight"]
            return dict(wt=sg2net.prep_rgb(W), mw=sd[p + ".modulated_conv.modulation.weight"], mb=sd[p + ".modulated_conv.modulation.bias"],
                        bias=sd[p + ".bias"].reshape(3).contiguous(), cin=W.shape[2])

        convs, rgbs = [styled("style_conv1", False, 16, True)], [rgb("to_rgb1")]
        for j in range(n_cond - 1):
            convs += [styled(f"style_convs.{2 * j}", True, 16 << j, False), styled(f"style_convs.{2 * j + 1}", False, 32 << j, True)]
            rgbs.append(rgb(f"to_rgbs.{j}"))
        order = range(n_cond - 1, -1, -1)                                                      # decoder order: the 16 x 16 level first
        return dict(size=out_size, log_size=log_size, n_cond=n_cond, num_latent=2 * log_size - 6, sb=sb, fir4=fir4,
                    first=conv("conv_body_first"), down=[conv(f"conv_body_down.{j}", down=True) for j in range(n_cond - 1)],
                    final_conv=conv("final_conv"), fd1=conv("final_down1", down=True), fd2=conv("final_down2", down=True),
                    final=(sd["final_linear.weight"], sd["final_linear.bias"]),
                    shift=[conv(f"condition_shift.{j}", activate=False) for j in range(n_cond)],                # encoder order
                    cond=[tuple(sd[f"condition_scale{k}.{j}.{t}"] for k in (1, 2) for t in ("weight", "bias")) for j in order],
                    cond_c=[int(sd[f"condition_scale1.{j}.bias"].shape[0]) for j in order], convs=convs, rgbs=rgbs)


# ------------------------------------------------------------------------------------------------ the forward pass
def _conv(P, L, x, out, bs, h, st):
    """A plain 3 x 3 convolution layer of the batch ``x [bs, cin, h, h]`` into ``out``; a ``down`` layer blurs into a scratch map first."""
    sg2net.conv3x3(L, x, out, bs, h, P["sb"], st, L["fir"])


def _tables(P, latent, bs, dev):
    """Every layer's (s, d) from its own latent row in one batched pass; returns [(s, d)] for the convolutions and [s] for the ToRGBs."""
    convs, rgbs = P["convs"], P["rgbs"]
    rows = [0] + [i for j in range(len(rgbs) - 1) for i in (2 * j + 1, 2 * j + 2)] + [1] + [2 * j + 3 for j in range(len(rgbs) - 1)]
    layers = convs + rgbs
    s_all = torch.empty(bs * sum(L["cin"] for L in layers), dtype=torch.float32, device=dev)
    d_all = torch.empty(bs * sum(L["cout"] for L in convs), dtype=torch.float32, device=dev)
    base, row_bytes = latent.data_ptr(), 4 * latent.stride(1)
    return sg2net.style_tables(layers, [(base + row * row_bytes, latent.stride(0), 0) for row in rows], bs, STYLE_DIM, s_all, d_all)


def _modconv(P, L, x, out, s, d, noise, bs, h, st):
    """The layer's modulated convolution with its noise; a plain StyleConv adds bias and activation, a norm layer leaves both to the epilogue kernel."""
    bias, act = (None, 0) if L["norm"] else (L["bias"], 1)
    sg2net.modconv(L, x, out, s, d, sb=P["sb"], blur=P["fir4"], noise=noise, bias=bias, act=act, bs=bs, h=h, st=st)


def _condition(P, in_size, bs, dev):
    """Norm2Scale of both condition linears for every level: two tables ``[bs, sum C]`` in decoder order, and each level's first column."""
    n = len(P["cond"])
    total = sum(P["cond_c"])
    s1n, s2n = (torch.empty((bs, total), dtype=torch.float32, device=dev) for _ in (0, 1))
    ptrs = [(ctypes.c_void_p * n)(*[lv[k].data_ptr() for lv in P["cond"]]) for k in range(4)]
    lib().call("e4s_gcfsr_condition", _p(s1n), _p(s2n), _p(in_size), ptrs[0], ptrs[1], ptrs[2], ptrs[3], (ctypes.c_int * n)(*P["cond_c"]), n, bs, _stream())
    begin = [sum(P["cond_c"][:l]) for l in range(n)]
    return s1n, s2n, begin


def _scale_shift_act(y, shift, s1n, s2n, col, bias):
    bs, C, h, w = y.shape
    lib().call("e4s_gcfsr_scale_shift_act", _p(y), _p(shift), _p(s1n[:, col:]), _p(s2n[:, col:]), _p(bias), bs, C, h * w, s1n.stride(0), _stream())


def _inpaint_run(P, x, in_size, noise, want_latent):
    bs, dev = x.shape[0], x.device
    size, n_cond = P["size"], P["n_cond"]
    st = _stream()
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)               # noqa: E731
    # encoder: a feature per condition level (encoder order: the full size first), its shift map, then the latent rows
    feats, shifts = [], []
    f = new(bs, P["first"]["cout"], size, size)
    _conv(P, P["first"], x, f, bs, size, st)
    r = size
    for j in range(n_cond):
        if j:
            L = P["down"][j - 1]
            nxt = new(bs, L["cout"], r // 2, r // 2)
            _conv(P, L, f, nxt, bs, r, st)
            f, r = nxt, r // 2
        feats.append(f)
        sh = new(bs, P["shift"][j]["cout"], r, r)
        _conv(P, P["shift"][j], f, sh, bs, r, st)
        shifts.append(sh)
    shifts = shifts[::-1]
    d1, d2 = new(bs, P["fd1"]["cout"], 8, 8), new(bs, P["fd2"]["cout"], 4, 4)
    _conv(P, P["fd1"], f, d1, bs, 16, st)
    _conv(P, P["fd2"], d1, d2, bs, 8, st)
    W, b = P["final"]
    latent = new(bs, P["num_latent"], STYLE_DIM)
    grouped_linear(d2.view(bs, 1, -1), [W], [b], scale=1 / math.sqrt(W.shape[1]), bias_mul=1.0, act=2, out=latent.view(bs, 1, -1))
    conv_t, rgb_t = _tables(P, latent, bs, dev)
    s1n, s2n, begin = _condition(P, in_size, bs, dev)
    # decoder
    convs, rgbs = P["convs"], P["rgbs"]
    out = new(bs, P["final_conv"]["cout"], 16, 16)
    _conv(P, P["final_conv"], f, out, bs, 16, st)

    def torgb(j, x, skip, h):
        R = rgbs[j]
        dst = new(bs, 3, h, h)
        sg2net.torgb(R, x, rgb_t[j], skip, P["fir4"], dst, bs, h, st)
        return dst

    def norm_layer(i, level, x, h):
        L = convs[i]
        y = new(bs, L["cout"], h, h)
        _modconv(P, L, x, y, *conv_t[i], noise[i], bs, h, st)
        _scale_shift_act(y, shifts[level], s1n, s2n, begin[level], L["bias"])
        return y

    out = norm_layer(0, 0, out, 16)
    skip = torgb(0, out, None, 16)
    h = 16
    for j in range(1, len(rgbs)):
        a = 2 * j - 1
        up = new(bs, convs[a]["cout"], 2 * h, 2 * h)
        _modconv(P, convs[a], out, up, *conv_t[a], noise[a], bs, h, st)
        h *= 2
        out = norm_layer(a + 1, j, up, h)
        skip = torgb(j, out, skip, h)
    return skip, (latent if want_latent else None)


def _noise_checked(name, noise, bs, size, dev=None):
    """The noise list's length, dtypes and shapes; with ``dev``, its placement too.  Returns detached contiguous maps."""
    sizes = noise_sizes(size)
    if not isinstance(noise, (list, tuple)) or len(noise) != len(sizes):
        raise ValueError(f"{name}: noise is a list of {len(sizes)} float32 maps [bs or 1, 1, h, w] at resolutions {sizes}, got "
                         f"{len(noise) if isinstance(noise, (list, tuple)) else type(noise).__name__}")
    out = []
    for i, (t, r) in enumerate(zip(noise, sizes)):
        _tensor_checked(name, f"noise[{i}]", t, torch.float32, 4, f"a float32 [bs or 1, 1, {r}, {r}] map")
        if t.shape[0] not in (1, bs) or tuple(t.shape[1:]) != (1, r, r):
            raise ValueError(f"{name}: noise[{i}] is {tuple(t.shape)}, expected [{bs} or 1, 1, {r}, {r}]")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"{name}: device mismatch: noise[{i}] on {t.device}, the input on {dev}")
        out.append(t.detach().contiguous())
    return out


def _arith_checked(name):
    sg2net.arith_checked(name, "ops_inpaint", ARITH)


def _weights_checked(name, weights):
    netweights.check_loaded(name, weights, "the inpainting weights")
    return _validated(name, weights, _net_of(weights))


def _generator_checked(name, generator, dev):
    if generator is not None and (not isinstance(generator, torch.Generator) or generator.device != dev):
        raise ValueError(f"{name}: generator is a torch.Generator on {dev} (the noise is drawn on the device), got {getattr(generator, 'device', type(generator).__name__)}")


def _draw_noise(bs, size, dev, generator):
    return [torch.randn((bs, 1, r, r), generator=generator, device=dev, dtype=torch.float32) for r in noise_sizes(size)]


def inpaint_forward(x: torch.Tensor, in_size: torch.Tensor, weights, noise=None, generator=None, return_latents: bool = False):
    """``FaceInpaintingArch.forward(x, in_size, noise=noise)`` (gcfsr_arch.py:1473-1540) in eval mode on the device: ``(image, latent or None)`` with the float32
    image ``[bs, 3, S, S]`` and the latent ``[bs, num_latent, 512]``, from a float32 ``x [bs, 4, S, S]`` (the masked image and the mask plane) and the hole share
    ``in_size``, float32 ``[bs]`` or ``[bs, 1]`` (the reference's caller passes ``[1]``: batch 1 only).  ``weights``: a module with the network's keys
    (``FaceInpainting``) or a mapping such as ``torch.load('net_g_50000.pth')['params_ema']``; ``S`` is read off the keys.  ``noise``: a list of ``num_layers``
    float32 maps ``[bs or 1, 1, h, w]`` at ``noise_sizes(S)``; None: drawn with ``torch.randn(..., generator=generator)`` on the device in layer order,
    reproducible under a seeded generator and never bit-equal to the reference's draws.  Refused, before any launch: a CPU tensor, another dtype or rank, a
    module in training mode, a module that never loaded weights, an image of another size, an ``in_size`` of another batch, a noise list of the wrong length or
    shapes, an ``ARITH`` outside the two."""
    name = "inpaint_forward"
    checked = _weights_checked(name, weights)
    size = checked[1][0]
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, 4, S, S] tensor: the masked image and the mask plane")
    bs = x.shape[0]
    if tuple(x.shape[1:]) != (4, size, size):
        raise ValueError(f"{name}: x is {tuple(x.shape)}: the network's size is {size}, expected [bs, 4, {size}, {size}]")
    if not isinstance(in_size, torch.Tensor):
        raise TypeError(f"{name}: in_size must be a torch.Tensor")
    if in_size.dtype != torch.float32 or tuple(in_size.shape) not in ((bs,), (bs, 1)):
        raise ValueError(f"{name}: in_size: expected float32 [{bs}] or [{bs}, 1], got {in_size.dtype} {tuple(in_size.shape)}")
    if noise is not None:
        _noise_checked(name, noise, bs, size)
    _placed_checked(name, "x", x, checked[2])
    if in_size.device != x.device:
        raise RuntimeError(f"{name}: device mismatch: in_size on {in_size.device}, x on {x.device}")
    if noise is not None:
        noise = _noise_checked(name, noise, bs, size, x.device)
    _generator_checked(name, generator, x.device)
    _arith_checked(name)
    if bs == 0:
        return x.new_empty((0, 3, size, size)), (x.new_empty((0, 2 * int(math.log2(size)) - 6, STYLE_DIM)) if return_latents else None)
    with torch.no_grad():
        if noise is None:
            noise = _draw_noise(bs, size, x.device, generator)
        return _inpaint_run(prepare(PreparedInpaint, weights, checked), x.detach().contiguous(), in_size.detach().reshape(bs).contiguous(), noise, return_latents)


def _faces_mask_checked(name, faces_u8, hole_u8, size=None):
    _tensor_checked(name, "faces_u8", faces_u8, torch.uint8, 4, "a uint8 [n, S, S, 3] RGB image")
    _tensor_checked(name, "hole_u8", hole_u8, torch.uint8, 3, "a uint8 [n, S, S] 0/1 hole mask")
    n, H, W, c = faces_u8.shape
    if c != 3 or H != W or H < 1 or H > 4096 or (size is not None and H != size):
        want = f"[n, {size}, {size}, 3] (resizing to the network's size is pipeline.inpaint_faces')" if size is not None else "[n, S, S, 3] with 1 <= S <= 4096"
        raise ValueError(f"{name}: faces_u8 is {tuple(faces_u8.shape)}, expected {want}")
    if tuple(hole_u8.shape) != (n, H, W):
        raise ValueError(f"{name}: hole_u8 is {tuple(hole_u8.shape)}: a mask of another batch or size, expected {(n, H, W)}")
    _cuda_checked(name, faces_u8=faces_u8, hole_u8=hole_u8)
    if hole_u8.device != faces_u8.device:
        raise RuntimeError(f"{name}: device mismatch: hole_u8 on {hole_u8.device}, faces_u8 on {faces_u8.device}")
    return n, H


def inpaint_input(faces_u8: torch.Tensor, hole_u8: torch.Tensor):
    """The network's input as ``inpainting()`` forms it (``e4s_gcfsr_input``): ``(x, in_size, count)`` with ``x [n, 4, S, S]`` = the image ``/ 255`` (a float64
    division rounded to float32) with the hole zeroed and the mask plane, ``count [n]`` (int32) the hole pixels and ``in_size [n] = count / S^2``, from uint8
    ``faces_u8 [n, S, S, 3]`` and the uint8 hole mask ``hole_u8 [n, S, S]`` (0 = keep, anything else = hole)."""
    n, S = _faces_mask_checked("inpaint_input", faces_u8, hole_u8)
    dev = faces_u8.device
    x = torch.empty((n, 4, S, S), dtype=torch.float32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    in_size = torch.empty((n,), dtype=torch.float32, device=dev)
    part = torch.empty((n, 64), dtype=torch.int32, device=dev)
    lib().call("e4s_gcfsr_input", _p(x), _p(count), _p(in_size), _p(part), _p(faces_u8.contiguous()), _p(hole_u8.contiguous()), n, S, _stream())
    return x, in_size, count


def inpaint_condition(in_size: torch.Tensor, scale1, scale2):
    """``Norm2Scale`` of the two condition linears for every level in one launch (``e4s_gcfsr_condition``): ``(s1n, s2n)``, two float32 tables
    ``[bs, sum C]`` with the levels side by side in the order given.  ``in_size``: float32 ``[bs]``; ``scale1`` / ``scale2``: per level a pair
    ``(weight [C, 1], bias [C])`` of ``condition_scale1/2``."""
    name = "inpaint_condition"
    _tensor_checked(name, "in_size", in_size, torch.float32, 1, "a float32 [bs] tensor")
    _cuda_checked(name, in_size=in_size)
    if len(scale1) != len(scale2) or not 1 <= len(scale1) <= 8:
        raise ValueError(f"{name}: scale1 and scale2 are lists of 1..8 (weight, bias) pairs of one length, got {len(scale1)} and {len(scale2)}")
    levels = []
    for l, ((w1, b1), (w2, b2)) in enumerate(zip(scale1, scale2)):
        C = b1.shape[0] if isinstance(b1, torch.Tensor) and b1.dim() == 1 else -1
        for nm, t, shape in (("weight", w1, (C, 1)), ("bias", b1, (C,)), ("weight", w2, (C, 1)), ("bias", b2, (C,))):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape or C < 1 or t.device != in_size.device:
                raise ValueError(f"{name}: level {l}: {nm}: expected float32 {shape} on {in_size.device}, got {getattr(t, 'dtype', type(t).__name__)} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
        levels.append(tuple(t.detach().contiguous() for t in (w1, b1, w2, b2)))
    P = dict(cond=levels, cond_c=[int(lv[1].shape[0]) for lv in levels])
    s1n, s2n, _ = _condition(P, in_size.detach().contiguous(), in_size.shape[0], in_size.device)
    return s1n, s2n


def scale_shift_act(y: torch.Tensor, shift: torch.Tensor, s1n: torch.Tensor, s2n: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The epilogue of ``StyleConv_norm_scale_shift`` in place (``e4s_gcfsr_scale_shift_act``): ``y <- lrelu(y * s1n[b, c] + shift * s2n[b, c] + bias[c], 0.2) *
    sqrt(2)``, every operation rounded on its own.  ``y``, ``shift``: contiguous float32 ``[bs, C, h, w]``; ``s1n``, ``s2n``: float32 ``[bs, C]`` (rows may be
    strided: a level's columns of the condition tables); ``bias [C]``.  Returns ``y``."""
    name = "scale_shift_act"
    _tensor_checked(name, "y", y, torch.float32, 4, "a float32 [bs, C, h, w] tensor")
    bs, C, h, w = y.shape
    if not y.is_contiguous() or h < 1 or w < 1 or C < 1:
        raise ValueError(f"{name}: y is updated in place: a contiguous [bs, C, h, w] tensor with C, h, w >= 1, got {tuple(y.shape)} with strides {y.stride()}")
    _tensor_checked(name, "shift", shift, torch.float32, 4, "a float32 [bs, C, h, w] tensor")
    if shift.shape != y.shape:
        raise ValueError(f"{name}: shift is {tuple(shift.shape)}, y {tuple(y.shape)}")
    for nm, t in (("s1n", s1n), ("s2n", s2n)):
        _tensor_checked(name, nm, t, torch.float32, 2, f"a float32 [{bs}, {C}] table")
        if tuple(t.shape) != (bs, C) or t.stride(1) != 1 or (bs > 1 and t.stride(0) < C):
            raise ValueError(f"{name}: {nm} is {tuple(t.shape)} with strides {t.stride()}, expected [{bs}, {C}] with unit column stride")
    if bs > 1 and s1n.stride(0) != s2n.stride(0):
        raise ValueError(f"{name}: s1n and s2n have row strides {s1n.stride(0)} and {s2n.stride(0)}: the two tables share one")
    _tensor_checked(name, "bias", bias, torch.float32, 1, f"a float32 [{C}] vector")
    if bias.shape[0] != C:
        raise ValueError(f"{name}: bias is {tuple(bias.shape)}, expected [{C}]")
    _cuda_checked(name, y=y, shift=shift, s1n=s1n, s2n=s2n, bias=bias)
    stride = s1n.stride(0) if bs > 1 else C
    lib().call("e4s_gcfsr_scale_shift_act", _p(y), _p(shift.contiguous()), _p(s1n), _p(s2n), _p(bias.contiguous()), bs, C, h * w, stride, _stream())
    return y


def inpaint_tail(img: torch.Tensor, faces_u8: torch.Tensor, hole_u8: torch.Tensor) -> torch.Tensor:
    """The end of ``inpainting()`` (``e4s_gcfsr_tail``): uint8 ``[n, S, S, 3]`` = ``round((faces / 255 * (1 - m) + clamp(img, 0, 1) * m) * 255)``, half to even,
    from the network's float32 image ``[n, 3, S, S]``, the input bytes and the hole mask.  Outside the hole the input bytes come back exactly."""
    name = "inpaint_tail"
    n, S = _faces_mask_checked(name, faces_u8, hole_u8)
    _tensor_checked(name, "img", img, torch.float32, 4, f"a float32 [{n}, 3, {S}, {S}] image")
    if tuple(img.shape) != (n, 3, S, S):
        raise ValueError(f"{name}: img is {tuple(img.shape)}, expected {(n, 3, S, S)}")
    _cuda_checked(name, img=img)
    out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=faces_u8.device)
    lib().call("e4s_gcfsr_tail", _p(out), _p(img.detach().contiguous()), _p(faces_u8.contiguous()), _p(hole_u8.contiguous()), n, S, _stream())
    return out


def mask_support_axis(src: int, dst: int, area: bool):
    """(start, count) int32 ``[dst]`` of one axis of ``cv2.resize`` at its default ``INTER_LINEAR``: the source taps with a non-zero weight.  ``area``: the exact
    2 : 1 downscale of both sides, which OpenCV routes to ``INTER_AREA`` (both pixels of the pair).  Otherwise ``f = float32((d + 0.5) src / dst - 0.5)``,
    ``s = floor(f)``, ``f -= s``; ``s < 0``: ``s = 0, f = 0``; ``s >= src - 1``: ``s = src - 1, f = 0``; the first tap's weight ``1 - f`` is never zero, the
    second's, ``f``, is zero at both clamps and wherever the coordinate is whole (every pixel of a copy)."""
    d = np.arange(dst, dtype=np.float64)
    if area:
        return (2 * d).astype(np.int32), np.full(dst, 2, np.int32)
    f = ((d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f)
    return s.astype(np.int32), (1 + (f != 0)).astype(np.int32)


@functools.lru_cache(maxsize=16)
def _mask_support_tables(H, W, S, dev):
    area = H == 2 * S and W == 2 * S
    ys, yc = mask_support_axis(H, S, area)
    xs, xc = mask_support_axis(W, S, area)
    return tuple(torch.from_numpy(a).to(dev) for a in (ys, yc, xs, xc))


def cv_mask_support(mask: torch.Tensor, size: int) -> torch.Tensor:
    """The hole mask at the network's size (``e4s_cv_mask_support``): uint8 0/1 ``[bs, size, size]`` = ``cv2.resize(mask.astype(float64), (size, size)) > 0`` for a
    non-negative float32 or uint8 ``mask [bs, H, W]``.  ``H, W == size``: a copy; both sides exactly ``2 size``: OpenCV's ``INTER_AREA`` route, any pixel of
    the 2 x 2 block counts; otherwise the bilinear taps with a non-zero weight (``mask_support_axis``).  A restatement: cv2 itself has never been run against
    it; negative or NaN mask values are outside the rule."""
    name = "cv_mask_support"
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{name}: mask must be a torch.Tensor")
    if mask.dtype not in (torch.float32, torch.uint8) or mask.dim() != 3:
        raise ValueError(f"{name}: mask: expected a float32 or uint8 [bs, H, W] tensor, got {mask.dtype} {tuple(mask.shape)}")
    bs, H, W = mask.shape
    if isinstance(size, bool) or not isinstance(size, int) or not 1 <= size <= INPAINT_MAX_SIDE or not 1 <= H <= INPAINT_MAX_SIDE or not 1 <= W <= INPAINT_MAX_SIDE:
        raise ValueError(f"{name}: size and the mask's sides are ints in 1..{INPAINT_MAX_SIDE}, got size {size!r} and a {H} x {W} mask")
    _cuda_checked(name, mask=mask)
    out = torch.empty((bs, size, size), dtype=torch.uint8, device=mask.device)
    if bs:
        ys, yc, xs, xc = _mask_support_tables(H, W, size, mask.device)
        lib().call("e4s_cv_mask_support", _p(out), _p(mask.contiguous()), int(mask.dtype == torch.float32), _p(ys), _p(yc), _p(xs), _p(xc), bs, H, W, size, _stream())
    return out


def inpaint_image(faces_u8: torch.Tensor, hole_u8: torch.Tensor, weights, noise=None, generator=None) -> torch.Tensor:
    """``inpainting(face_img, mask)`` between its two resizes, for a batch: uint8 ``faces_u8 [n, S, S, 3]`` RGB and the uint8 hole mask ``hole_u8 [n, S, S]`` at
    the network's size to uint8 ``[n, S, S, 3]``, as three steps: ``e4s_gcfsr_input``, the network with each sample's own hole share, ``e4s_gcfsr_tail``.
    ``weights``, ``noise``, ``generator`` and the refusals as ``inpaint_forward``; a face of another size raises ``ValueError``: the resizes are
    ``pipeline.inpaint_faces``'."""
    name = "inpaint_image"
    checked = _weights_checked(name, weights)
    size = checked[1][0]
    n, _ = _faces_mask_checked(name, faces_u8, hole_u8, size)
    netweights._devices_checked(name, "faces_u8", faces_u8, checked[2])
    if noise is not None:
        noise = _noise_checked(name, noise, n, size, faces_u8.device)
    _generator_checked(name, generator, faces_u8.device)
    _arith_checked(name)
    if n == 0:
        return torch.empty((0, size, size, 3), dtype=torch.uint8, device=faces_u8.device)
    with torch.no_grad():
        faces_u8, hole_u8 = faces_u8.contiguous(), hole_u8.contiguous()
        x, in_size, _ = inpaint_input(faces_u8, hole_u8)
        if noise is None:
            noise = _draw_noise(n, size, faces_u8.device, generator)
        img, _ = _inpaint_run(prepare(PreparedInpaint, weights, checked), x, in_size, noise, False)
        return inpaint_tail(img, faces_u8, hole_u8)


def inpaint_size(weights, name: str = "inpaint_faces") -> int:
    """The size ``weights`` (a module or a mapping) run at, read off their keys."""
    return _weights_checked(name, weights)[1][0]


__all__ = ["FaceInpainting", "PreparedInpaint", "INPAINT_MAX_SIDE", "inpaint_channels", "noise_sizes", "inpaint_state_dict_shapes", "inpaint_weight_tensors",
           "inpaint_forward", "inpaint_input", "inpaint_condition", "scale_shift_act", "inpaint_tail", "mask_support_axis", "cv_mask_support", "inpaint_image",
           "inpaint_size"]
