"""Row f12: GPEN face enhancement, stage 1 — the GAN-prior generator, ``FullGenerator`` of swap_face_fine/gpen/face_model/gpen_model.py:628-690, in eval mode
between the tensor ends of ``FaceGAN`` (face_gan.py:49-62): ``gpen_forward``, ``gpen_image``.  Everything else of ``FaceEnhancement.process`` (the RetinaFace
detector, the 5-point warps, ParseNet, the RealESRNet pass, the paste mask, ``cv2.resize``) is rows f13 - f16; ``pipeline.gpen_face_enhancement`` chains them.

The network is a StyleGAN2 synthesis network behind a strided-convolution encoder, with one style per sample; its contractions run on kernels the library
has for the regional generator, in their single-region form (``nreg = 1``, no label map), the rest on csrc/gpen.hip.  The key-mirror modules, the stock
restatement of the layers, the weight preparation and the calls it shares with ``ops_inpaint`` are ``sg2net``'s:

    ecd0               e4s_gpen_stem: 1 x 1 convolution 3 -> C0, bias, leaky-relu * sqrt(2) in exact float32; from uint8 it applies img2tensor's roundings too
    ecd1 ..            e4s_upfirdn2d (4 x 4 FIR, pad (2, 2)), then e4s_conv2d_sb (3 x 3, stride 2, pad 0): sqrt(2) of the fused activation is folded into weight
                       and bias in float64 (leaky-relu is positively homogeneous), the PReLU epilogue with a 0.2 slope vector is then FusedLeakyReLU exactly
    final_linear, MLP  e4s_grouped_linear (groups = 1, act = 2) with EqualLinear's scale and lr_mul; PixelNorm between them is three stock tensor operations
    tables             every layer's style and demodulation tables in one batched call (``sg2net.style_tables``): the one latent is known before the first layer runs
    StyledConv         the modulated convolution writes planes [0, C) of the layer's [2C, h, w] buffer with the first C entries of the activation bias and no
                       additive noise; e4s_gpen_noise_half writes lrelu(noise.weight * f_r + bias[C:]) * sqrt(2) into planes [C, 2C), one launch for both layers
                       of a resolution.  The concatenation is never copied.
    ToRGB              e4s_region_torgb, which chains the skips through the FIR upsampling

Up layers.  Three entries compute a single-region up layer: the parity-composed form (``e4s_region_modconv3x3_sb(up = 1)``: 4 x the transposed convolution's
multiply-adds, but split-K over the input channels, so it fills the chip on a 4 x 4 map), the pair ``e4s_modconv_tconv_sb`` + ``e4s_blur_epilogue`` (1 x, no
split-K, a [cout, 2h + 1, 2w + 1] round trip) and ``e4s_modconv_up_fused_sb`` (1 x, one launch, no split-K: its grid is tiles x cout / 32).  A layer whose
input is at most ``UP_COMPOSED_MAX_WIDTH`` (32) wide takes the composed form: one sample at a time the 1 x entries run such a layer on 16 - 64 workgroups.
Measured on an MI355X at GPEN-BFR-512's shapes, batch 1 (tools/time_gpen.py --layers; the table is profiles/f12_time_gpen.txt, quoted in DESIGN.md row
f12): the composed form is 6 x faster at 4 x 4 and still ahead at 32 x 32, from 64 x 64 on the fused entry wins.  The two-launch pair is not used: it has
the fused entry's grid and a round trip more.  ``ARITH = "f32"`` takes the
composed exact-fp32 entry for every up layer.

``ARITH`` (module attribute): ``"sb"``, the default, runs the convolutions on the two-way split-bf16 entries, the synthesis path's arithmetic (bar: 1e-3 on
generated pixels); ``"f32"`` on the exact-fp32 entries ``e4s_region_modconv3x3`` / ``e4s_conv2d``.  The stem, the linear layers, the tables, ToRGB and the
glue are float32 in both.

The existing kernels write dense ``[bs, cout, h, w]`` outputs, so the samples of a batch run one after another on one sample's scratch, each exactly as a
batch-of-one call.  Forward only; no host synchronisation; the same inputs give the same bits; after one eager call (which prepares the weights) a call
captures in a graph."""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import netweights, sg2net
from ._lib import lib
from .ops import _p, _stream, grouped_linear
from .netweights import PreparedNet, _Net, _cuda_checked, _image_checked, _keys_shapes, _placed_checked, _tensor_checked, _validated, module_net, prepare
from .sg2net import SQRT2, Bias, EqualConv, EqualLinear, Fir, ModConv, flrelu, torch_modconv, upfirdn

ARITH = "sb"                                 # "sb" | "f32" (module attribute, no environment variable: tests and tools set it)
UP_COMPOSED_MAX_WIDTH = 32                   # up layers with an input at most this wide take the parity-composed, split-K form (measured: see the module text)
LR_MLP = 0.01


def gpen_channels(channel_multiplier: int = 2, narrow: float = 1):
    """Channels per resolution (gpen_model.py:642-653)."""
    c = {r: int(512 * narrow) for r in (4, 8, 16, 32)}
    c.update({64: int(256 * channel_multiplier * narrow), 128: int(128 * channel_multiplier * narrow), 256: int(64 * channel_multiplier * narrow),
              512: int(32 * channel_multiplier * narrow), 1024: int(16 * channel_multiplier * narrow), 2048: int(8 * channel_multiplier * narrow)})
    return c


# ------------------------------------------------------------------------------------------------ the module: the reference's keys, a stock-PyTorch forward
class _Noise(nn.Module):
    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(1))


class _StyledConv(nn.Module):
    def __init__(self, cin, cout, style_dim, up=False):
        super().__init__()
        self.conv = ModConv(cin, cout, 3, style_dim, 4.0 if up else None)
        self.noise = _Noise()
        self.activate = Bias(2 * cout)


class _ToRGB(nn.Module):
    def __init__(self, cin, style_dim, up=True):
        super().__init__()
        if up:
            self.upsample = Fir(4.0)
        self.conv = ModConv(cin, 3, 1, style_dim)
        self.bias = nn.Parameter(torch.zeros(1, 3, 1, 1))


class _Input(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.input = nn.Parameter(torch.randn(1, c, 4, 4))


class _Generator(nn.Module):
    def __init__(self, size, style_dim, n_mlp, ch):
        super().__init__()
        self.style = nn.Sequential(nn.Identity(), *[EqualLinear(style_dim, style_dim, lr_mul=LR_MLP) for _ in range(n_mlp)])    # (0: PixelNorm)
        self.input = _Input(ch[4])
        self.conv1 = _StyledConv(ch[4], ch[4], style_dim)
        self.to_rgb1 = _ToRGB(2 * ch[4], style_dim, up=False)
        self.convs, self.upsamples, self.to_rgbs = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        cin = ch[4]
        for i in range(3, int(math.log2(size)) + 1):
            cout = ch[2 ** i]
            self.convs.append(_StyledConv(2 * cin, cout, style_dim, up=True))
            self.convs.append(_StyledConv(2 * cout, cout, style_dim))
            self.to_rgbs.append(_ToRGB(2 * cout, style_dim))
            cin = cout


def _config_checked(size, style_dim, n_mlp, channel_multiplier, narrow):
    ok_int = lambda v: isinstance(v, int) and not isinstance(v, bool)      # noqa: E731
    if not ok_int(size) or size < 8 or size > 2048 or size & (size - 1):
        raise ValueError(f"GPEN: size is a power of two in 8..2048, got {size!r}")
    if not ok_int(style_dim) or style_dim < 1 or not ok_int(n_mlp) or n_mlp < 1 or not ok_int(channel_multiplier) or channel_multiplier < 1:
        raise ValueError(f"GPEN: style_dim, n_mlp and channel_multiplier are positive ints, got {style_dim!r}, {n_mlp!r}, {channel_multiplier!r}")
    ch = gpen_channels(channel_multiplier, narrow)
    if min(ch[2 ** i] for i in range(2, int(math.log2(size)) + 1)) < 1:
        raise ValueError(f"GPEN: narrow = {narrow!r} leaves a level without channels")
    return ch


class GPEN(nn.Module):
    """``FullGenerator(size, style_dim, n_mlp, channel_multiplier, narrow=narrow)`` of swap_face_fine/gpen/face_model/gpen_model.py with its ``state_dict`` keys,
    shapes and order (163 tensors at the default, the FIR buffers and ``generator.input.input`` included; ``GPEN-BFR-512.pth`` loads with ``strict=True``).
    ``forward`` is the plain PyTorch composition in eval mode — what the tests and the timing compare ``gpen_forward`` with; ``gpen_forward(x, module)`` runs
    the same weights on the HIP kernels.  It starts with random weights and ``gpen_forward`` refuses it until ``load_state_dict`` has filled it."""

    def __init__(self, size: int = 512, style_dim: int = 512, n_mlp: int = 8, channel_multiplier: int = 2, narrow: float = 1):
        super().__init__()
        ch = _config_checked(size, style_dim, n_mlp, channel_multiplier, narrow)
        self.size, self.style_dim, self.n_mlp, self.channel_multiplier, self.narrow = size, style_dim, n_mlp, channel_multiplier, narrow
        self.log_size = int(math.log2(size))
        self.n_latent = 2 * self.log_size - 2
        self.generator = _Generator(size, style_dim, n_mlp, ch)
        self.ecd0 = nn.Sequential(nn.Sequential(EqualConv(3, ch[size], 1), Bias(ch[size])))          # (a ConvLayer inside a Sequential)
        cin = ch[size]
        for i in range(self.log_size, 2, -1):
            cout = ch[2 ** (i - 1)]
            setattr(self, f"ecd{self.log_size - i + 1}", nn.Sequential(nn.Sequential(Fir(), EqualConv(cin, cout, 3), Bias(cout))))
            cin = cout
        self.final_linear = nn.Sequential(EqualLinear(16 * ch[4], style_dim))
        self.requires_grad_(False)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if "ecd0.0.0.weight" in state_dict and "generator.input.input" in state_dict:
            self._loaded = True
        return out

    def forward(self, x, return_latents: bool = False):
        if self.training:
            raise NotImplementedError("GPEN: training mode is not implemented; call .eval()")
        with torch.no_grad():
            image, latent = _torch_forward(dict(self.state_dict()), x, self.log_size)
        return image, (latent if return_latents else None)


def _torch_styled(sd, p, x, w, noise, up=False):
    y = torch_modconv(sd, p + ".conv", x, w, up, blur=sd[p + ".conv.blur.kernel"] if up else None)
    return flrelu(torch.cat((y, sd[p + ".noise.weight"] * noise), 1), sd[p + ".activate.bias"])


def _torch_forward(sd, x, log_size):
    feats = []
    W = sd["ecd0.0.0.weight"]
    x = flrelu(F.conv2d(x, W * (1 / math.sqrt(W.shape[1]))), sd["ecd0.0.1.bias"])
    feats.append(x)
    for i in range(1, log_size - 1):
        W = sd[f"ecd{i}.0.1.weight"]
        x = flrelu(F.conv2d(upfirdn(x, sd[f"ecd{i}.0.0.kernel"], 1, (2, 2)), W * (1 / math.sqrt(W.shape[1] * 9)), stride=2), sd[f"ecd{i}.0.2.bias"])
        feats.append(x)
    W = sd["final_linear.0.weight"]
    z = flrelu(F.linear(x.reshape(x.shape[0], -1), W * (1 / math.sqrt(W.shape[1]))), sd["final_linear.0.bias"])
    z = z * torch.rsqrt(torch.mean(z ** 2, dim=1, keepdim=True) + 1e-8)
    i = 1
    while f"generator.style.{i}.weight" in sd:
        W = sd[f"generator.style.{i}.weight"]
        z = flrelu(F.linear(z, W * ((1 / math.sqrt(W.shape[1])) * LR_MLP)), sd[f"generator.style.{i}.bias"] * LR_MLP)
        i += 1
    noise = [f for f in feats[::-1] for _ in (0, 1)][1:]
    g = "generator."
    out = sd[g + "input.input"].repeat(x.shape[0], 1, 1, 1)
    out = _torch_styled(sd, g + "conv1", out, z, noise[0])
    skip = torch_modconv(sd, g + "to_rgb1.conv", out, z, demodulate=False) + sd[g + "to_rgb1.bias"]
    for j in range(log_size - 2):
        out = _torch_styled(sd, f"{g}convs.{2 * j}", out, z, noise[1 + 2 * j], up=True)
        out = _torch_styled(sd, f"{g}convs.{2 * j + 1}", out, z, noise[2 + 2 * j])
        p = f"{g}to_rgbs.{j}"
        skip = torch_modconv(sd, p + ".conv", out, z, demodulate=False) + sd[p + ".bias"] + upfirdn(skip, sd[p + ".upsample.kernel"], 2, (2, 1))
    return skip, z[:, None].repeat(1, 2 * log_size - 2, 1)


# ------------------------------------------------------------------------------------------------ weights
def gpen_state_dict_shapes(size: int = 512, style_dim: int = 512, n_mlp: int = 8, channel_multiplier: int = 2, narrow: float = 1):
    """``{key: shape}`` of ``GPEN(size, style_dim, n_mlp, channel_multiplier, narrow).state_dict()``, in its order."""
    return dict(_keys_shapes(GPEN, size, style_dim, n_mlp, channel_multiplier, narrow))


def _gpen_variant(name, sd):
    """(size, style_dim, n_mlp, channel_multiplier, narrow) read off the keys and shapes of ``sd``."""
    for probe in ("ecd0.0.0.weight", "generator.input.input", "final_linear.0.weight"):
        t = sd.get(probe)
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise KeyError(f"{name}: the weights lack '{probe}': expected the keys of FullGenerator (ops.gpen_state_dict_shapes())")
    levels = 0
    while f"ecd{levels}.0.{0 if levels == 0 else 1}.weight" in sd:
        levels += 1
    n_mlp = 0
    while f"generator.style.{n_mlp + 1}.weight" in sd:
        n_mlp += 1
    size = 2 ** (levels + 1)
    c4, c_size = int(sd["generator.input.input"].shape[1]), int(sd["ecd0.0.0.weight"].shape[0])
    narrow = c4 / 512
    base = {64: 256, 128: 128, 256: 64, 512: 32, 1024: 16, 2048: 8}.get(size)
    cm = max(1, round(c_size / (base * narrow))) if base and narrow > 0 else 2
    if levels < 2 or n_mlp < 1 or c4 < 1:
        raise KeyError(f"{name}: the weights do not describe a FullGenerator ({levels} encoder levels, {n_mlp} style layers)")
    return size, int(sd["final_linear.0.weight"].shape[0]), n_mlp, cm, narrow


def _gpen_shapes(variant):
    return gpen_state_dict_shapes(*variant)


def _net_of(weights):
    """The description ``_validated`` checks ``weights`` against.  A ``GPEN`` module hands over the configuration it was built with; only a mapping has it
    read off its keys and shapes (``_gpen_variant``), which recovers ``narrow`` and ``channel_multiplier`` up to what ``int()`` left of them."""
    if not isinstance(weights, GPEN):
        return _GPEN_NET
    return module_net(_GPEN_NET, (weights.size, weights.style_dim, weights.n_mlp, weights.channel_multiplier, weights.narrow))


_GPEN_NET = _Net("FullGenerator", _gpen_shapes, ("module.",), False, ("ecd0.0.0.weight",), _gpen_variant,
                 "the native path is the eval-mode forward", ())


def gpen_weight_tensors(weights, name: str = "gpen_forward"):
    """The tensors of the network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _net_of(weights))[2]


def check_loaded(weights):
    """``weights`` itself; raises if it is a module whose weights were never loaded (an enhancement from initial parameters would be silently wrong)."""
    netweights.check_loaded(None, weights, "the GPEN weights")
    return weights


def _weights_checked(name, weights):
    """``_validated``'s result for ``weights``, refused first if they are a module that never loaded any."""
    check_loaded(weights)
    return _validated(name, weights, _net_of(weights))


class PreparedGPEN(PreparedNet):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage or the arithmetic changes.  ``stem``: ecd0's weight with
    its scale, ``[C0, 3]``, and bias; ``enc``: per level (FIR, slabs or K-major fp32 weight, bias, slope vector) with sqrt(2) folded into weight and bias in
    float64; ``final`` and ``mlp``: the EqualLinear weights as they are (scale and lr_mul are call arguments); per modulated convolution its split-bf16 slabs
    (or K-major fp32 weight), ``wsq`` table, modulation weights, noise weight and activation bias; per ToRGB its ``k = 1`` weight."""

    __slots__ = ()
    _entry = "gpen_forward"

    def _net(self, weights):
        return _net_of(weights)

    def _settings(self):
        return ARITH, UP_COMPOSED_MAX_WIDTH

    def _build(self, sd, variant, dev):
        size, sdim, n_mlp, _, _ = variant
        log_size = int(math.log2(size))
        sb = ARITH == "sb"

        def enc_level(i):
            return dict(sg2net.prep_conv3x3(sd[f"ecd{i}.0.1.weight"], sd[f"ecd{i}.0.2.bias"], SQRT2, sb, True), fir=sd[f"ecd{i}.0.0.kernel"])

        def styled(p, up, w_in):
            W = sd[p + ".conv.weight"]
            composed = up and sg2net.use_composed(ARITH, UP_COMPOSED_MAX_WIDTH, w_in)
            blur = sd[p + ".conv.blur.kernel"] if up else None
            wt, wsq = sg2net.prep_styled(W, blur, composed, sb)
            return dict(wt=wt, wsq=wsq, mw=sd[p + ".conv.modulation.weight"], mb=sd[p + ".conv.modulation.bias"], nw=sd[p + ".noise.weight"],
                        bias=sd[p + ".activate.bias"], blur=blur, up=up, composed=composed, cin=W.shape[2], cout=W.shape[1])

        def rgb(p, up):
            W = sd[p + ".conv.weight"]
            return dict(wt=sg2net.prep_rgb(W), mw=sd[p + ".conv.modulation.weight"], mb=sd[p + ".conv.modulation.bias"], bias=sd[p + ".bias"].reshape(3).contiguous(),
                        upk=sd[p + ".upsample.kernel"] if up else None, cin=W.shape[2])

        W0 = sd["ecd0.0.0.weight"]
        g = "generator."
        convs, rgbs = [styled(g + "conv1", False, 4)], [rgb(g + "to_rgb1", False)]
        for j in range(log_size - 2):
            convs += [styled(f"{g}convs.{2 * j}", True, 4 << j), styled(f"{g}convs.{2 * j + 1}", False, 8 << j)]
            rgbs.append(rgb(f"{g}to_rgbs.{j}", True))
        return dict(size=size, sdim=sdim, log_size=log_size, sb=sb,
                    stem=((W0 * (1 / math.sqrt(3))).reshape(W0.shape[0], 3).contiguous(), sd["ecd0.0.1.bias"]),
                    enc=[enc_level(i) for i in range(1, log_size - 1)],
                    final=(sd["final_linear.0.weight"], sd["final_linear.0.bias"]),
                    mlp=[(sd[f"{g}style.{i}.weight"], sd[f"{g}style.{i}.bias"]) for i in range(1, n_mlp + 1)],
                    const=sd[g + "input.input"], convs=convs, rgbs=rgbs)


# ------------------------------------------------------------------------------------------------ the forward pass
def _scratch(P, dev):
    """One sample's buffers, made once per call: the encoder's features (the decoder's noise), one blurred map sized for the largest level (``blurs``: each
    level's view of it), every decoder layer's [2C, h, w] output, the ToRGB chain, the style / demodulation tables and the two style vectors the linear layers
    alternate between."""
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)               # noqa: E731
    size = P["size"]
    C0 = P["stem"][0].shape[0]
    feats, blurred = [new(1, C0, size, size)], []
    r = size
    for L in P["enc"]:
        blurred.append((1, L["cin"], r + 1, r + 1))
        r //= 2
        feats.append(new(1, L["cout"], r, r))
    blur = new(max(math.prod(shape) for shape in blurred))
    outs = []
    r = 4
    for L in P["convs"]:
        if L["up"]:
            r *= 2
        outs.append(new(1, 2 * L["cout"], r, r))
    n_s = sum(L["cin"] for L in P["convs"]) + sum(L["cin"] for L in P["rgbs"])
    n_d = sum(L["cout"] for L in P["convs"])
    return dict(feats=feats, blurs=[blur[:math.prod(shape)].view(shape) for shape in blurred], outs=outs,
                rgb=[new(1, 3, 4 << j, 4 << j) for j in range(len(P["rgbs"]))], s=new(n_s), d=new(n_d), z=[new(1, 1, P["sdim"]), new(1, 1, P["sdim"])])


def _tables(P, S, latent):
    """Every layer's (s, d) from the one ``latent [1, 1, sdim]``; returns [(s, d)] for the convolutions and [s] for the ToRGBs."""
    layers = P["convs"] + P["rgbs"]
    return sg2net.style_tables(layers, [(latent.data_ptr(), latent.stride(0), latent.stride(1))] * len(layers), 1, P["sdim"], S["s"], S["d"])


def _modconv(P, L, x, out, s, d, h, st):
    """The layer's modulated convolution on one sample into ``out`` (planes [0, C) of its buffer) with the first C activation-bias entries, leaky-relu * sqrt(2),
    and no additive noise."""
    sg2net.modconv(L, x, out, s, d, sb=P["sb"], blur=L["blur"], bias=L["bias"], act=1, bs=1, h=h, st=st)


def _noise_half(f, layers, outs):
    """planes [C, 2C) of one or two layers' buffers from the encoder feature ``f [1, C, h, w]``."""
    C, h, w = f.shape[1:]
    hw = h * w
    a, b = layers[0], (layers[1] if len(layers) > 1 else None)
    lib().call("e4s_gpen_noise_half", _p(outs[0][:, C:]), _p(outs[1][:, C:]) if b else None, _p(f), _p(a["nw"]), _p(b["nw"]) if b else None, _p(a["bias"][C:]),
               _p(b["bias"][C:]) if b else None, 1, C, hw, 2 * C * hw, _stream())


def _gpen_sample(P, S, x, x_u8, out_f, latent_row):
    """The network on one sample: ``x [1, 3, size, size]`` float32 or ``x_u8 [1, size, size, 3]``; the image goes to ``out_f [1, 3, size, size]``, the style
    vector to ``latent_row [1, 1, sdim]``."""
    st = _stream()
    size = P["size"]
    feats = S["feats"]
    lib().call("e4s_gpen_stem", _p(feats[0]), _p(x), _p(x_u8), _p(P["stem"][0]), _p(P["stem"][1]), 1, feats[0].shape[1], size, size, st)
    r = size
    for L, src, dst, blur in zip(P["enc"], feats[:-1], feats[1:], S["blurs"]):
        sg2net.conv3x3(L, src, dst, 1, r, P["sb"], st, L["fir"], blur)
        r //= 2
    f4 = feats[-1]
    za, zb = S["z"]
    W, b = P["final"]
    grouped_linear(f4.view(1, 1, -1), [W], [b], scale=1 / math.sqrt(W.shape[1]), bias_mul=1.0, act=2, out=za)
    torch.mul(za, torch.rsqrt(torch.mean(za * za, dim=2, keepdim=True) + 1e-8), out=zb)                 # PixelNorm
    cur, nxt = zb, za
    for i, (W, b) in enumerate(P["mlp"]):
        dst = latent_row if i == len(P["mlp"]) - 1 else nxt
        grouped_linear(cur, [W], [b], scale=(1 / math.sqrt(W.shape[1])) * LR_MLP, bias_mul=LR_MLP, act=2, out=dst)
        cur, nxt = dst, cur
    conv_t, rgb_t = _tables(P, S, latent_row)
    convs, outs, rgbs = P["convs"], S["outs"], P["rgbs"]
    noise = feats[::-1]                                                                                 # f4, f8, ..., f_size
    _modconv(P, convs[0], P["const"], outs[0][:, :convs[0]["cout"]], *conv_t[0], 4, st)
    _noise_half(noise[0], convs[:1], outs[:1])
    n_rgb = len(rgbs)

    def torgb(j, x, skip, h):
        dst = out_f if j == n_rgb - 1 else S["rgb"][j]
        sg2net.torgb(rgbs[j], x, rgb_t[j], skip, rgbs[j]["upk"], dst, 1, h, st)
        return dst

    skip = torgb(0, outs[0], None, 4)
    h = 4
    for j in range(1, n_rgb):
        a, b = 2 * j - 1, 2 * j
        _modconv(P, convs[a], outs[a - 1], outs[a][:, :convs[a]["cout"]], *conv_t[a], h, st)
        h *= 2
        _noise_half(noise[j], convs[a:b + 1], outs[a:b + 1])
        _modconv(P, convs[b], outs[a], outs[b][:, :convs[b]["cout"]], *conv_t[b], h, st)
        skip = torgb(j, outs[b], skip, h)


def _gpen_run(P, x, x_u8, want_latent):
    src = x if x is not None else x_u8
    bs, dev = src.shape[0], src.device
    size, sdim, n_latent = P["size"], P["sdim"], 2 * P["log_size"] - 2
    out = torch.empty((bs, 3, size, size), dtype=torch.float32, device=dev)
    lat = torch.empty((bs, 1, sdim), dtype=torch.float32, device=dev)
    S = _scratch(P, dev)
    for b in range(bs):
        _gpen_sample(P, S, None if x is None else x[b:b + 1], None if x_u8 is None else x_u8[b:b + 1], out[b:b + 1], lat[b:b + 1])
    return out, (lat.repeat(1, n_latent, 1) if want_latent else None)


def _gpen_checked_all(name, weights, x=None, img_u8=None):
    checked = _weights_checked(name, weights)
    size = checked[1][0]
    t, nm, H, W, c = _image_checked(name, x, img_u8, "a float32 [bs, 3, size, size] image", "a uint8 [bs, size, size, 3] RGB image")
    if (c, H, W) != (3, size, size):
        expected = f"[bs, 3, {size}, {size}]" if x is not None else f"[bs, {size}, {size}, 3] (resizing to the network's size is the caller's)"
        raise ValueError(f"{name}: {nm} is {tuple(t.shape)}: the network's size is {size}, expected {expected}")
    _placed_checked(name, nm, t, checked[2])
    sg2net.arith_checked(name, "ops_gpen", ARITH)
    return checked


def gpen_forward(x: torch.Tensor, weights, return_latents: bool = False):
    """``FullGenerator.forward(x)`` (gpen_model.py:671-690) in eval mode on the device: ``(image, latent or None)`` with the float32 image
    ``[bs, 3, size, size]`` and the latent ``[bs, n_latent, style_dim]``, from a float32 ``x [bs, 3, size, size]``.  ``weights``: a module with the network's
    keys (``GPEN``, the drop-in ``FullGenerator``) or a mapping such as ``torch.load('GPEN-BFR-512.pth')``; the configuration is read off the keys and shapes.
    A module's prepared weights are cached per parameter version; a mapping is prepared on every call.  Refused: a CPU tensor, another dtype, a module in
    training mode, a module that never loaded weights, an image of another size.  Every argument is checked before any launch."""
    name = "gpen_forward"
    checked = _gpen_checked_all(name, weights, x=x)
    if x.shape[0] == 0:
        size, sdim = checked[1][0], checked[1][1]
        n_latent = 2 * int(math.log2(size)) - 2
        return x.new_empty((0, 3, size, size)), (x.new_empty((0, n_latent, sdim)) if return_latents else None)
    with torch.no_grad():
        return _gpen_run(prepare(PreparedGPEN, weights, checked), x.detach().contiguous(), None, return_latents)


def gpen_image(img_u8: torch.Tensor, weights) -> torch.Tensor:
    """``FaceGAN.process`` behind its ``cv2.resize`` and without its BGR flips: uint8 ``[bs, size, size, 3]`` RGB to uint8 of the same shape, as three fused
    steps: the stem kernel applies ``img2tensor`` (``/ 255``, ``(x - 0.5) / 0.5``), the network, and ``e4s_gpen_to_u8`` (``* 0.5 + 0.5``, the clip, ``* 255``,
    the truncation).  An image of another size raises ``ValueError``: the resize is the caller's (the reference's is cv2's fixed-point bilinear)."""
    name = "gpen_image"
    checked = _gpen_checked_all(name, weights, img_u8=img_u8)
    bs, size = img_u8.shape[0], checked[1][0]
    out = torch.empty((bs, size, size, 3), dtype=torch.uint8, device=img_u8.device)
    if bs == 0:
        return out
    with torch.no_grad():
        r, _ = _gpen_run(prepare(PreparedGPEN, weights, checked), None, img_u8.contiguous(), False)
        lib().call("e4s_gpen_to_u8", _p(out), _p(r), bs, size, size, _stream())
    return out


def gpen_to_u8(x: torch.Tensor) -> torch.Tensor:
    """``FaceGAN.tensor2img`` without its flip (``e4s_gpen_to_u8``): float32 ``[bs, 3, H, W]`` to uint8 ``[bs, H, W, 3]``."""
    _tensor_checked("gpen_to_u8", "x", x, torch.float32, 4, "a float32 [bs, 3, H, W] image")
    if x.shape[1] != 3 or x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError(f"gpen_to_u8: expected a float32 [bs, 3, H, W] image, got {tuple(x.shape)}")
    _cuda_checked("gpen_to_u8", x=x)
    x = x.contiguous()
    out = torch.empty((x.shape[0], x.shape[2], x.shape[3], 3), dtype=torch.uint8, device=x.device)
    lib().call("e4s_gpen_to_u8", _p(out), _p(x), x.shape[0], x.shape[2], x.shape[3], _stream())
    return out


__all__ = ["GPEN", "PreparedGPEN", "gpen_channels", "gpen_state_dict_shapes", "gpen_weight_tensors", "gpen_forward", "gpen_image", "gpen_to_u8"]
