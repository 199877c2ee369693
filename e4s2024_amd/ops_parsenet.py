"""Row f13: GPEN face enhancement, stage 2 — the face mask's network, ``ParseNet`` of swap_face_fine/gpen/face_parse/parse_model.py:21-75 with the
``ConvLayer`` and ``ResidualBlock`` of blocks.py:72-125, in eval mode between the tensor ends of ``FaceParse`` (face_parsing.py:39-79): ``parsenet_forward``,
``parsenet_mask``, ``parsenet_mask_from_tensor``.  ``FaceEnhancement.process`` runs it at 512 x 512 on every enhanced face (face_enhancement.py:89); its
19-class argmax through the 0 / 255 table ``MASK_COLORMAP`` is the mask that decides where the enhanced face is pasted.  Scope: ``norm_type='bn'``,
``relu_type='LeakyReLU'``, any sizes, widths and depths, any input whose sides keep every feature map at least 2 x 2.

Every ``ConvLayer`` is reflection pad 1 (behind a nearest x 2 in the decoder), a 3 x 3 convolution, an eval BatchNorm or a bias, and LeakyReLU 0.2 or nothing.
The convolutions run on ``conv.hip``'s three-way split-bf16 kernel (``e4s_conv2d_sb3``: fp32-class, the argmax must not move) with ``pad = 0`` on planes that
csrc/parsenet.hip wrote:

    encoder.0          e4s_parsenet_stem: 3 -> C0 in exact float32, the reflection in its index arithmetic; from uint8 it applies FaceParse.img2tensor too
    a ConvLayer        e4s_parsenet_pad (u = 1, or 2 for scale='up'), then e4s_conv2d_sb3 with ks = 3, stride 1 or 2, pad 0; BatchNorm folded into weight and bias
                       in float64 (``lossnet.bn_fold`` / ``prep_fwd``), LeakyReLU as the PReLU epilogue with a 0.2 slope vector
    a ResidualBlock    ``conv1`` and the shortcut convolution read the SAME padded buffer (scale='down': shortcut stride 2, conv1 stride 1, conv2 stride 2;
                       scale='up': both read the u = 2 buffer); ``conv2`` takes the shortcut's output, or in a body block the block's own input, as ``residual``
    feat + body(feat)  the ``add`` operand of the pad pass behind it: never a pass of its own
    the two heads      one padded buffer; with the image wanted one 22-output convolution on concatenated weights (the 19 logits first), else the 19-output one
    the mask           e4s_bilinear_argmax at equal size with MASK_COLORMAP as its table: argmax + table (include/e4s_hip.h says why)

The whole batch goes through each launch.  Forward only; no host synchronisation; the same inputs give the same bits; after one eager call (which prepares the
weights) a call captures in a graph."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import lib
from .lossnet import bn_fold, conv_sb, prep_fwd
from .ops import _p, _stream
from .netweights import EVAL_ONLY, PreparedNet, _Net, _image_checked, _keys_shapes, _placed_checked, _validated, bn_shapes, check_loaded, module_net, prepare

SLOPE = 0.2                                  # ReluLayer's LeakyReLU (blocks.py:58)
# FaceParse.MASK_COLORMAP (face_parsing.py:30): background, hat (14) and cloth (18) are 0, every other class 255
MASK_COLORMAP = (0, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 0, 255, 255, 255, 0)


def img2tensor_table() -> np.ndarray:
    """``FaceParse.img2tensor`` on every uint8 level: numpy's float64 ``v / 255. * 2 - 1``, rounded once to float32 (``.float()``)."""
    return (np.arange(256, dtype=np.uint8) / 255. * 2 - 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the module: the reference's keys, a stock-PyTorch forward
class _Norm(nn.Module):
    """``NormLayer(c, norm_type='bn')``: its ``norm``."""

    def __init__(self, c):
        super().__init__()
        self.norm = nn.BatchNorm2d(c, affine=True)

    def forward(self, x):
        return self.norm(x)


class _ConvLayer(nn.Module):
    """``ConvLayer(cin, cout, 3, scale, norm_type, relu_type)``: ``conv2d`` (without bias under a BatchNorm) and ``norm`` when there is one."""

    def __init__(self, cin, cout, scale="none", bn=False, act=False):
        super().__init__()
        self.scale, self.act = scale, act
        self.conv2d = nn.Conv2d(cin, cout, 3, 2 if scale == "down" else 1, bias=not bn)
        if bn:
            self.norm = _Norm(cout)

    def forward(self, x):
        if self.scale == "up":
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        x = self.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"))
        if hasattr(self, "norm"):
            x = self.norm(x)
        return F.leaky_relu(x, SLOPE) if self.act else x


class _ResidualBlock(nn.Module):
    """``ResidualBlock(cin, cout, relu_type, 'bn', scale)``: a shortcut convolution unless the block keeps size and width."""

    def __init__(self, cin, cout, scale="none"):
        super().__init__()
        if scale != "none" or cin != cout:
            self.shortcut_func = _ConvLayer(cin, cout, scale)
        first, second = {"down": ("none", "down"), "up": ("up", "none"), "none": ("none", "none")}[scale]
        self.conv1 = _ConvLayer(cin, cout, first, bn=True, act=True)
        self.conv2 = _ConvLayer(cout, cout, second, bn=True)

    def forward(self, x):
        identity = self.shortcut_func(x) if hasattr(self, "shortcut_func") else x
        return identity + self.conv2(self.conv1(x))


def parsenet_structure(in_size=512, out_size=512, min_feat_size=32, base_ch=64, parsing_ch=19, res_depth=10, ch_range=(32, 256)):
    """The constructor arithmetic of parse_model.py:36-67 as ``(C0, blocks, head channels, parsing_ch)``, ``blocks`` a tuple of (group, scale, cin, cout) with
    group 'encoder' (index from 1), 'body' or 'decoder': what the keys and shapes of the network follow from."""
    ok_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)          # noqa: E731
    if not all(ok_int(v) for v in (in_size, out_size, min_feat_size, base_ch, parsing_ch, res_depth)) or len(tuple(ch_range)) != 2:
        raise ValueError("ParseNet: in_size, out_size, min_feat_size, base_ch, parsing_ch and res_depth are ints and ch_range a pair")
    min_ch, max_ch = (int(v) for v in ch_range)
    if min(in_size, out_size, min_feat_size, base_ch, parsing_ch, min_ch) < 1 or max_ch < min_ch or res_depth < 0:
        raise ValueError(f"ParseNet: sizes, widths and parsing_ch are positive, res_depth >= 0 and ch_range ascending, got {in_size}, {out_size}, "
                         f"{min_feat_size}, {base_ch}, {parsing_ch}, {res_depth}, {tuple(ch_range)!r}")
    clip = lambda c: max(min_ch, min(c, max_ch))                                            # noqa: E731
    min_feat_size = min(in_size, min_feat_size)
    if out_size < min_feat_size:
        raise ValueError(f"ParseNet: out_size {out_size} is below the smallest feature size {min_feat_size}")
    down_steps, up_steps = int(np.log2(in_size // min_feat_size)), int(np.log2(out_size // min_feat_size))
    blocks, head = [], base_ch
    for _ in range(down_steps):
        blocks.append(("encoder", "down", clip(head), clip(head * 2)))
        head *= 2
    blocks += [("body", "none", clip(head), clip(head))] * res_depth
    for _ in range(up_steps):
        blocks.append(("decoder", "up", clip(head), clip(head // 2)))
        head //= 2
    return int(base_ch), tuple(blocks), clip(head), int(parsing_ch)


def _checked_types(relu_type, norm_type):
    if not isinstance(norm_type, str) or norm_type.lower() != "bn":
        raise ValueError(f"ParseNet: norm_type {norm_type!r} is not implemented: the native network is norm_type='bn'")
    if not isinstance(relu_type, str) or relu_type.lower() != "leakyrelu":
        raise ValueError(f"ParseNet: relu_type {relu_type!r} is not implemented: the native network is relu_type='LeakyReLU'")


class ParseNet(nn.Module):
    """``ParseNet(in_size, out_size, min_feat_size, base_ch, parsing_ch, res_depth, relu_type, norm_type, ch_range)`` of
    swap_face_fine/gpen/face_parse/parse_model.py with its ``state_dict`` keys, shapes and order; the defaults are what ``FaceParse`` builds (238 tensors,
    ``num_batches_tracked`` included; ``ParseNet-latest.pth`` loads with ``strict=True``).  ``forward`` is the plain PyTorch composition in eval mode, returning
    ``(out_mask, out_img)`` — what the tests and the timing compare ``parsenet_forward`` with; ``parsenet_forward(x, module)`` runs the same weights on the HIP
    kernels.  It starts with random weights and the native entries refuse it until ``load_state_dict`` has filled it."""

    def __init__(self, in_size=512, out_size=512, min_feat_size=32, base_ch=64, parsing_ch=19, res_depth=10, relu_type="LeakyReLU", norm_type="bn",
                 ch_range=(32, 256)):
        super().__init__()
        _checked_types(relu_type, norm_type)
        self.structure = parsenet_structure(in_size, out_size, min_feat_size, base_ch, parsing_ch, res_depth, tuple(ch_range))
        self.in_size, self.out_size, self.res_depth = in_size, out_size, res_depth
        c0, blocks, head, ncls = self.structure
        group = lambda g: [_ResidualBlock(cin, cout, scale) for gg, scale, cin, cout in blocks if gg == g]      # noqa: E731
        self.encoder = nn.Sequential(_ConvLayer(3, c0), *group("encoder"))
        self.body = nn.Sequential(*group("body"))
        self.decoder = nn.Sequential(*group("decoder"))
        self.out_img_conv = _ConvLayer(head, 3)
        self.out_mask_conv = _ConvLayer(head, ncls)
        self.requires_grad_(False)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if "encoder.0.conv2d.weight" in state_dict and "out_mask_conv.conv2d.weight" in state_dict:
            self._loaded = True
        return out

    def forward(self, x):
        if self.training:
            raise NotImplementedError("ParseNet: training mode is not implemented; call .eval()")
        with torch.no_grad():
            feat = self.encoder(x)
            x = self.decoder(feat + self.body(feat))
            out_img = self.out_img_conv(x)
            return self.out_mask_conv(x), out_img


# ------------------------------------------------------------------------------------------------ weights
def _conv_shapes(out, p, cin, cout, bn):
    out[p + ".conv2d.weight"] = (cout, cin, 3, 3)
    if not bn:
        out[p + ".conv2d.bias"] = (cout,)
        return
    bn_shapes(out, p + ".norm.norm", cout)


def _block_prefixes(blocks):
    """[(key prefix, scale, cin, cout, has a shortcut convolution)] in key order."""
    out, n = [], {"encoder": 1, "body": 0, "decoder": 0}
    for g, scale, cin, cout in blocks:
        out.append((f"{g}.{n[g]}", scale, cin, cout, scale != "none" or cin != cout))
        n[g] += 1
    return out


def parsenet_structure_shapes(structure):
    """``{key: shape}`` of the network with ``structure`` (``parsenet_structure``), in ``state_dict`` order."""
    c0, blocks, head, ncls = structure
    out = {}
    _conv_shapes(out, "encoder.0", 3, c0, False)
    for p, _, cin, cout, shortcut in _block_prefixes(blocks):
        if shortcut:
            _conv_shapes(out, p + ".shortcut_func", cin, cout, False)
        _conv_shapes(out, p + ".conv1", cin, cout, True)
        _conv_shapes(out, p + ".conv2", cout, cout, True)
    _conv_shapes(out, "out_img_conv", head, 3, False)
    _conv_shapes(out, "out_mask_conv", head, ncls, False)
    return out


def parsenet_state_dict_shapes(in_size=512, out_size=512, min_feat_size=32, base_ch=64, parsing_ch=19, res_depth=10, ch_range=(32, 256)):
    """``{key: shape}`` of ``ParseNet(...).state_dict()``, in its order."""
    return dict(_keys_shapes(ParseNet, in_size, out_size, min_feat_size, base_ch, parsing_ch, res_depth, "LeakyReLU", "bn", tuple(ch_range)))


def _structure_of_keys(name, sd):
    """The structure read off the keys and shapes of a mapping (a module of ``ParseNet`` hands over its own)."""
    def shape(key):
        t = sd.get(key)
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise KeyError(f"{name}: the weights lack '{key}': expected the keys of ParseNet (ops.parsenet_state_dict_shapes())")
        return t.shape

    c0 = int(shape("encoder.0.conv2d.weight")[0])
    blocks = []
    for g, scale, first in (("encoder", "down", 1), ("body", "none", 0), ("decoder", "up", 0)):
        i = first
        while f"{g}.{i}.conv1.conv2d.weight" in sd:
            cout, cin = shape(f"{g}.{i}.conv1.conv2d.weight")[:2]
            blocks.append((g, scale, int(cin), int(cout)))
            i += 1
    w = shape("out_mask_conv.conv2d.weight")
    return c0, tuple(blocks), int(w[1]), int(w[0])


_PARSENET_NET = _Net("ParseNet", parsenet_structure_shapes, ("module.",), False, ("encoder.0.conv2d.weight",), _structure_of_keys, EVAL_ONLY,
                     ("num_batches_tracked",))


def _net_of(weights):
    """The description ``_validated`` checks ``weights`` against: a ``ParseNet`` module is held to the structure it was built with."""
    return module_net(_PARSENET_NET, weights.structure) if isinstance(weights, ParseNet) else _PARSENET_NET


def parsenet_weight_tensors(weights, name: str = "parsenet_forward"):
    """The float tensors of the network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _net_of(weights))[2]


class PreparedParseNet(PreparedNet):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage.  ``stem``: encoder.0's weight ``[C0, 27]`` and bias as
    they are; per block the three-way split slabs and float32 biases of ``conv1`` / ``conv2`` with the eval BatchNorm folded in float64 and of the shortcut
    convolution, and the 0.2 slope vector; ``head19`` / ``head22``: ``out_mask_conv`` alone and with ``out_img_conv`` behind it; ``lut``: img2tensor's 256
    values; ``cmap``: MASK_COLORMAP as uint8."""

    __slots__ = ()
    _entry = "parsenet_forward"

    def _net(self, weights):
        return _net_of(weights)

    def _build(self, sd, structure, dev):
        c0, blocks, _, ncls = structure

        def plain(p):
            return prep_fwd(sd[p + ".conv2d.weight"], None, sd[p + ".conv2d.bias"].double())

        def normed(p):
            return prep_fwd(sd[p + ".conv2d.weight"], *bn_fold(sd, p + ".norm.norm"))

        layers = [dict(group=p.split(".")[0], scale=scale, cout=cout, sc=plain(p + ".shortcut_func") if shortcut else None, c1=normed(p + ".conv1"),
                       c2=normed(p + ".conv2"), slope=torch.full((cout,), SLOPE, dtype=torch.float32, device=dev))
                  for p, scale, _, cout, shortcut in _block_prefixes(blocks)]
        wm, bm = sd["out_mask_conv.conv2d.weight"], sd["out_mask_conv.conv2d.bias"]
        wi, bi = sd["out_img_conv.conv2d.weight"], sd["out_img_conv.conv2d.bias"]
        return dict(c0=c0, ncls=ncls, stem=(sd["encoder.0.conv2d.weight"].reshape(c0, 27).contiguous(), sd["encoder.0.conv2d.bias"]), blocks=layers,
                    head19=prep_fwd(wm, None, bm.double()), head22=prep_fwd(torch.cat((wm, wi)), None, torch.cat((bm, bi)).double()),
                    lut=torch.from_numpy(img2tensor_table()).to(dev),
                    cmap=torch.tensor([MASK_COLORMAP[c] if c < len(MASK_COLORMAP) else 255 for c in range(ncls)], dtype=torch.uint8).to(dev))


# ------------------------------------------------------------------------------------------------ the forward pass
def _pad(x, add=None, u=1):
    """``e4s_parsenet_pad``: the reflection-padded (and, with ``u = 2``, nearest-upsampled) planes of ``x + add``."""
    bs, c, h, w = x.shape
    out = torch.empty((bs, c, u * h + 2, u * w + 2), dtype=torch.float32, device=x.device)
    lib().call("e4s_parsenet_pad", _p(out), _p(x), _p(add), bs * c, h, w, u, _stream())
    return out


def _run(P, x, x_u8, bgr, with_image):
    """(the 19 logits, the image or None) of a float ``x [bs, 3, H, W]`` or a uint8 ``x_u8 [bs, H, W, 3]``."""
    src = x if x is not None else x_u8
    bs, (H, W) = src.shape[0], (src.shape[2:] if x is not None else src.shape[1:3])
    feat = torch.empty((bs, P["c0"], H, W), dtype=torch.float32, device=src.device)
    lib().call("e4s_parsenet_stem", _p(feat), _p(x), _p(x_u8), _p(P["lut"]), 1 if bgr else 0, _p(P["stem"][0]), _p(P["stem"][1]), bs, P["c0"], H, W, _stream())

    def block(L, cur, add=None):
        """A ResidualBlock on ``cur + add``: conv1 and the shortcut convolution read one padded buffer; conv2 adds the shortcut (or the block's input)."""
        s2 = 2 if L["scale"] == "down" else 1
        p = _pad(cur, add, 2 if L["scale"] == "up" else 1)
        identity = conv_sb(p, *L["sc"], k=3, stride=s2, pad=0) if L["sc"] is not None else cur
        r = conv_sb(p, *L["c1"], k=3, stride=1, pad=0, slope=L["slope"])
        return conv_sb(_pad(r), *L["c2"], k=3, stride=s2, pad=0, residual=identity)

    groups = {g: [L for L in P["blocks"] if L["group"] == g] for g in ("encoder", "body", "decoder")}
    for L in groups["encoder"]:
        feat = block(L, feat)
    cur = feat
    for L in groups["body"]:
        cur = block(L, cur)
    add = feat                                           # feat + body(feat) rides on the next pad pass: the first decoder block's, or the heads'
    for L in groups["decoder"]:
        cur, add = block(L, cur, add), None
    p = _pad(cur, add)
    if not with_image:
        return conv_sb(p, *P["head19"], k=3, pad=0), None
    both = conv_sb(p, *P["head22"], k=3, pad=0)
    return both[:, :P["ncls"]], both[:, P["ncls"]:]


def parsenet_output_size(structure, H: int, W: int):
    """(H', W') of the network's outputs for an H x W input, or None when a feature map on the way falls below 2 x 2 (the smallest reflection)."""
    for _, scale, _, _ in structure[1]:
        if min(H, W) < 2:
            return None
        if scale == "down":
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        elif scale == "up":
            H, W = 2 * H, 2 * W
    return (H, W) if min(H, W) >= 2 else None


def _checked_all(name, weights, x=None, img_u8=None, sized=False):
    """Everything that can be refused, before any launch: (checked weights, output size)."""
    check_loaded(name, weights, "the ParseNet weights")
    checked = _validated(name, weights, _net_of(weights))
    t, nm, H, W, c = _image_checked(name, x, img_u8, "a float32 [bs, 3, H, W] image", "a uint8 [bs, S, S, 3] image")
    if c != 3:
        raise ValueError(f"{name}: {nm} is {tuple(t.shape)}: expected three colour channels")
    in_size = getattr(weights, "in_size", None)
    if sized and in_size is not None and (H, W) != (in_size, in_size):
        raise ValueError(f"{name}: {nm} is {tuple(t.shape)}: the network's in_size is {in_size}, expected {in_size} x {in_size} "
                         "(resizing to the network's size is the caller's)")
    out_hw = parsenet_output_size(checked[1], int(H), int(W))
    if out_hw is None or max(out_hw) > 16384 or max(H, W) > 16384:
        raise ValueError(f"{name}: {nm} is {H} x {W}: every feature map of the network must stay at least 2 x 2 (and no side above 16384)")
    _placed_checked(name, nm, t, checked[2])
    return checked, out_hw


def parsenet_forward(x: torch.Tensor, weights, with_image: bool = False):
    """``ParseNet.forward(x)`` (parse_model.py:69-75) in eval mode on the device: ``(out_mask [bs, parsing_ch, H', W'], out_img [bs, 3, H', W'] or None)`` from
    a float32 ``x [bs, 3, H, W]``; the image head runs only ``with_image`` (the two are then views of one ``[bs, parsing_ch + 3, H', W']`` tensor, and the
    logits have the bits of the call without it).  ``weights``: a module with the network's keys (``ParseNet``, the drop-in) or the mapping ``torch.load``
    returns; a mapping's structure is read off its keys and shapes.  A module's prepared weights are cached per parameter version; a mapping is prepared on
    every call.  Refused: a CPU tensor, another dtype, a module in training mode, a module that never loaded weights, an input that lets a feature map fall
    below 2 x 2.  Every argument is checked before any launch."""
    name = "parsenet_forward"
    checked, (oh, ow) = _checked_all(name, weights, x=x)
    if x.shape[0] == 0:
        return x.new_empty((0, checked[1][3], oh, ow)), (x.new_empty((0, 3, oh, ow)) if with_image else None)
    with torch.no_grad():
        return _run(prepare(PreparedParseNet, weights, checked), x.detach().contiguous(), None, False, with_image)


def _mask_of(P, logits):
    bs, ncls, h, w = logits.shape
    out = torch.empty((bs, h, w), dtype=torch.uint8, device=logits.device)
    lib().call("e4s_bilinear_argmax", _p(out), _p(logits), _p(P["cmap"]), bs, ncls, h, w, h, w, _stream())
    return out


def parsenet_mask(img_u8: torch.Tensor, weights, bgr: bool = True) -> torch.Tensor:
    """``FaceParse.process`` (face_parsing.py:39-45) behind its ``cv2.resize``, for a batch on the device: uint8 ``[bs, S, S, 3]`` faces (BGR as the reference
    takes them, or RGB with ``bgr=False``) with ``S`` the module's ``in_size`` to the uint8 masks ``[bs, S', S']`` of 0 / 255, as three fused steps: the stem
    kernel applies ``img2tensor``, the network without its image head, and argmax + ``MASK_COLORMAP`` in one launch.  An image of another size raises
    ``ValueError`` naming the size: the resize is the caller's."""
    name = "parsenet_mask"
    checked, (oh, ow) = _checked_all(name, weights, img_u8=img_u8, sized=True)
    if img_u8.shape[0] == 0:
        return torch.empty((0, oh, ow), dtype=torch.uint8, device=img_u8.device)
    with torch.no_grad():
        P = prepare(PreparedParseNet, weights, checked)
        return _mask_of(P, _run(P, None, img_u8.contiguous(), bool(bgr), False)[0])


def parsenet_mask_from_tensor(imt: torch.Tensor, weights) -> torch.Tensor:
    """``FaceParse.process_tensor`` (face_parsing.py:47-57) for an input already at ``in_size`` (its nearest ``F.interpolate`` is then the identity): float32
    ``[bs, 3, S, S]`` BGR in [0, 1] to int64 ``[1, bs, S', S']`` of 0 / 255.  ``flip(1) * 2 - 1`` is stock PyTorch, each operation rounded on its own."""
    name = "parsenet_mask_from_tensor"
    checked, (oh, ow) = _checked_all(name, weights, x=imt, sized=True)
    if imt.shape[0] == 0:
        return torch.empty((1, 0, oh, ow), dtype=torch.int64, device=imt.device)
    with torch.no_grad():
        P = prepare(PreparedParseNet, weights, checked)
        x = (imt.detach().flip(1) * 2 - 1).contiguous()
        return _mask_of(P, _run(P, x, None, False, False)[0]).to(torch.int64).unsqueeze(0)


__all__ = ["ParseNet", "PreparedParseNet", "MASK_COLORMAP", "img2tensor_table", "parsenet_structure", "parsenet_structure_shapes", "parsenet_state_dict_shapes",
           "parsenet_weight_tensors", "parsenet_output_size", "parsenet_forward", "parsenet_mask", "parsenet_mask_from_tensor"]
