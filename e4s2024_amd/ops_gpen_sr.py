"""Row f16: GPEN face enhancement, stage 5 — the RealESRNet pass of ``FaceEnhancement.process`` (swap_face_fine/gpen/sr_model/real_esrnet.py:8-60 around
``RRDBNet(3, 3, scale, num_feat=32, num_block=23, num_grow_ch=32)`` of sr_model/rrdbnet_arch.py:64-116) and the ``cv2.resize`` of the frame to the
super-resolved size (face_enhancement.py:66), forward only: ``gpen_sr_forward``, ``gpen_sr_image``, ``cv_resize_linear``.

This is row f11's network (``ops.RRDBNet``: ``num_feat=64``, scale 4, another checkpoint) with the feature width and the scale as parameters: at scale 2 / 1
a ``pixel_unshuffle`` by 2 / 4 stands in front of ``conv_first``, which then has 12 / 48 input channels.  The scheme is ``_rrdb_sample``'s with ``num_feat`` a
parameter: a dense block's concatenations are never formed, its convolutions read the head of a ``num_feat + 128``-plane slab and write their 32 planes right
behind it; conv5 carries the block's ``* 0.2`` (folded in float64) and takes the block's input as its residual.  The convolutions run on csrc/conv.hip's
three-way split-bf16 kernel through ``lossnet.conv_sb``, the glue on csrc/rrdb.hip (``e4s_esr_scale_add``, ``e4s_esr_up2``), the two ends of
``RealESRNet.process`` and the resize on csrc/gpen_sr.hip:

    e4s_gsr_input             uint8 -> v / 255, the channel flip, the bottom / right reflect pad to a multiple of r and the pixel-unshuffle by r, one pass
    e4s_gsr_tail              conv_last in exact float32, clamp(0, 1), * 255.0, round half to even, the crop, the flip back, uint8
    e4s_cv_resize_linear_u8   cv2.resize at INTER_LINEAR in OpenCV's fixed-point arithmetic (pinned by tests/gpen_sr_model.py, never run against OpenCV)

The samples of a batch run one after another on one sample's scratch, each exactly as a batch-of-one call.  No host synchronisation; the same inputs give the
same bits; after one eager call (which prepares the weights) a call captures in a graph."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lossnet
from ._lib import lib
from .lossnet import conv_sb, prep_fwd, weights_key
from .ops import _Prepared, _c, _p, _stream
from .ops_recolor import _Net, _cuda_checked, _devices_checked, _keys_shapes, _tensor_checked, _validated

GPEN_SR_FEATS = (32, 64)                     # num_feat: 32 as RealESRNet builds it, 64 as the published x4 checkpoints have it
GPEN_SR_SCALES = (1, 2, 4)
GPEN_SR_GROW = 32                            # num_grow_ch, the only value the reference builds
GPEN_SR_SLOPE = 0.2
GPEN_SR_MAX_SIDE = 16384
_UNSHUFFLE = {4: 1, 2: 2, 1: 4}              # scale -> r of pixel_unshuffle, which is also mod_scale of RealESRNet.process
_SCALE_OF_CIN = {3 * r * r: s for s, r in _UNSHUFFLE.items()}
_PREFIXES = ("params_ema.", "params.")


class _RDB(nn.Module):
    """``ResidualDenseBlock(num_feat, 32)`` under the reference's parameter names."""

    def __init__(self, num_feat):
        super().__init__()
        for k in range(1, 6):
            setattr(self, f"conv{k}", nn.Conv2d(num_feat + (k - 1) * GPEN_SR_GROW, GPEN_SR_GROW if k < 5 else num_feat, 3, 1, 1))

    def forward(self, x):
        xs = [x]
        for k in range(1, 5):
            xs.append(F.leaky_relu(getattr(self, f"conv{k}")(torch.cat(xs, 1)), GPEN_SR_SLOPE))
        return self.conv5(torch.cat(xs, 1)) * 0.2 + x


class _RRDB(nn.Module):
    def __init__(self, num_feat):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = _RDB(num_feat), _RDB(num_feat), _RDB(num_feat)

    def forward(self, x):
        return self.rdb3(self.rdb2(self.rdb1(x))) * 0.2 + x


def _config_checked(name, num_block, num_feat, scale):
    if isinstance(num_block, bool) or not isinstance(num_block, int) or num_block < 1:
        raise ValueError(f"{name}: num_block is a positive int, got {num_block!r}")
    if num_feat not in GPEN_SR_FEATS:
        raise ValueError(f"{name}: num_feat is one of {GPEN_SR_FEATS}, got {num_feat!r}")
    if scale not in GPEN_SR_SCALES:
        raise ValueError(f"{name}: scale is one of {GPEN_SR_SCALES}, got {scale!r}")


class GpenSRNet(nn.Module):
    """``RRDBNet(3, 3, scale, num_feat, num_block, 32)`` of swap_face_fine/gpen/sr_model/rrdbnet_arch.py with its ``state_dict`` keys and shapes (a
    ``realesrnet_x2.pth``'s ``params_ema`` loads with ``strict=True``): 702 tensors at 23 blocks.  ``forward`` is the plain PyTorch composition — what the tests
    and the timing compare ``gpen_sr_forward`` with; ``gpen_sr_forward(x, module)`` runs the same weights on the HIP kernels."""

    def __init__(self, num_block: int = 23, num_feat: int = 32, scale: int = 2):
        super().__init__()
        _config_checked("GpenSRNet", num_block, num_feat, scale)
        self.num_block, self.num_feat, self.scale = num_block, num_feat, scale
        r = _UNSHUFFLE[scale]
        self.conv_first = nn.Conv2d(3 * r * r, num_feat, 3, 1, 1)
        self.body = nn.Sequential(*[_RRDB(num_feat) for _ in range(num_block)])
        self.conv_body = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_hr = nn.Conv2d(num_feat, num_feat, 3, 1, 1)
        self.conv_last = nn.Conv2d(num_feat, 3, 3, 1, 1)

    def forward(self, x):
        r = _UNSHUFFLE[self.scale]
        feat = self.conv_first(F.pixel_unshuffle(x, r) if r > 1 else x)       # (arch_util.pixel_unshuffle's channel order: c r r + dy r + dx)
        feat = feat + self.conv_body(self.body(feat))
        feat = F.leaky_relu(self.conv_up1(F.interpolate(feat, scale_factor=2, mode="nearest")), GPEN_SR_SLOPE)
        feat = F.leaky_relu(self.conv_up2(F.interpolate(feat, scale_factor=2, mode="nearest")), GPEN_SR_SLOPE)
        return self.conv_last(F.leaky_relu(self.conv_hr(feat), GPEN_SR_SLOPE))


def gpen_sr_state_dict_shapes(num_block: int = 23, num_feat: int = 32, scale: int = 2):
    """``{key: shape}`` of ``GpenSRNet(num_block, num_feat, scale).state_dict()``, in its order."""
    _config_checked("gpen_sr_state_dict_shapes", num_block, num_feat, scale)
    return dict(_keys_shapes(GpenSRNet, num_block, num_feat, scale))


def _gsr_shapes(variant):
    return gpen_sr_state_dict_shapes(*variant)


def _gsr_variant(name, sd):
    """(num_block, num_feat, scale) read off the keys and shapes of ``sd``: a mapping tells the scales apart through conv_first's input channels alone."""
    for probe in ("conv_first.weight", "body.0.rdb1.conv1.weight"):
        if probe not in sd:
            raise KeyError(f"{name}: the weights lack '{probe}': expected the keys of RRDBNet (ops.gpen_sr_state_dict_shapes())")
    first = sd["conv_first.weight"]
    shape = tuple(getattr(first, "shape", ()))
    if len(shape) != 4 or shape[0] not in GPEN_SR_FEATS or shape[1] not in _SCALE_OF_CIN or shape[2:] != (3, 3):
        raise ValueError(f"{name}: 'conv_first.weight' is {getattr(first, 'dtype', type(first).__name__)} {shape}, expected float32 (num_feat, 3 | 12 | 48, 3, 3) "
                         f"with num_feat one of {GPEN_SR_FEATS}")
    num_block = 0
    while f"body.{num_block}.rdb1.conv1.weight" in sd:
        num_block += 1
    return num_block, int(shape[0]), _SCALE_OF_CIN[shape[1]]


# a mapping may be the checkpoint itself, with the network under ``params_ema`` or ``params``
_GSR_NET = _Net("RRDBNet", _gsr_shapes, _PREFIXES, True, ("conv_first.weight",), _gsr_variant, None, ())


def gpen_sr_weight_tensors(weights, name: str = "gpen_sr_forward"):
    """The tensors of the network in key order, their shapes checked: what ``weights_key`` watches."""
    return _validated(name, weights, _GSR_NET)[2]


class PreparedGpenSRNet(_Prepared):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage.  ``first``, ``conv_body``, ``up1``, ``up2``, ``hr`` and
    per block three dense blocks of five convolutions, all as three-way split slabs with their biases; ``conv5`` of a dense block carries the block's ``* 0.2``
    in weight and bias (folded in float64), so that ``x5 * 0.2 + x`` is the convolution's residual epilogue; ``last`` conv_last's float32 weight and bias for
    the exact kernel; ``slope_feat`` / ``slope_grow`` the LeakyReLU as a PReLU slope vector."""

    __slots__ = ()

    def get(self, weights, checked=None):
        sd, (num_block, num_feat, scale), ts = checked if checked is not None else _validated("gpen_sr_forward", weights, _GSR_NET)
        key = weights_key(ts) + (ts[0].device,)
        hit = self._lookup(key)
        if hit is not None:
            return hit
        sd = {k: _c(sd[k].detach(), k) for k in gpen_sr_state_dict_shapes(num_block, num_feat, scale)}
        dev = ts[0].device

        def conv(name, fold=None):
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            if fold is None:
                return prep_fwd(w, None, b)
            return prep_fwd(w, torch.full((w.shape[0],), fold, dtype=torch.float64, device=dev), b.double() * fold)

        with torch.no_grad():
            body = [[[conv(f"body.{i}.rdb{r}.conv{k}", 0.2 if k == 5 else None) for k in range(1, 6)] for r in (1, 2, 3)] for i in range(num_block)]
            P = dict(num_block=num_block, num_feat=num_feat, scale=scale, first=conv("conv_first"), body=body, conv_body=conv("conv_body"),
                     up1=conv("conv_up1"), up2=conv("conv_up2"), hr=conv("conv_hr"),
                     last=(sd["conv_last.weight"].contiguous(), sd["conv_last.bias"].contiguous()),
                     slope_feat=torch.full((num_feat,), GPEN_SR_SLOPE, dtype=torch.float32, device=dev),
                     slope_grow=torch.full((GPEN_SR_GROW,), GPEN_SR_SLOPE, dtype=torch.float32, device=dev))
        return self._publish(key, P)


def _gsr_sample(P, x, out_f, out_u8, crop, bgr, reads, writes, feat0, ups):
    """The network behind its unshuffle on one sample ``x [1, 3 r r, h, w]``: ``ops_recolor._rrdb_sample`` with ``num_feat`` planes at a slab's head.  Dense
    block 1 of an RRDB goes slab 0 -> 1, block 2 goes 1 -> 2, block 3 goes 2 -> 1, and ``e4s_esr_scale_add`` puts ``head(1) * 0.2 + head(0)`` back into the head
    of slab 0.  ``crop``: (Ho, Wo) of the uint8 image."""
    _, _, h, w = x.shape
    C = P["num_feat"]
    st = _stream()
    head0, head1 = reads[0][0], reads[1][0]
    conv_sb(x, *P["first"], k=3, out=feat0)
    head0.copy_(feat0)
    for block in P["body"]:
        for rdb, (src, dst) in zip(block, ((0, 1), (1, 2), (2, 1))):
            R, W = reads[src], writes[src]
            for k in range(4):
                conv_sb(R[k], *rdb[k], k=3, slope=P["slope_grow"], out=W[k])
            conv_sb(R[4], *rdb[4], k=3, residual=R[0], out=reads[dst][0])
        lib().call("e4s_esr_scale_add", _p(head0), _p(head1), _p(head0), C, h * w, st)
    feat = conv_sb(head0, *P["conv_body"], k=3, residual=feat0, out=head1)                    # feat + conv_body(body(feat))
    for name, (up, out) in zip(("up1", "up2"), ups):
        lib().call("e4s_esr_up2", _p(up), _p(feat), C, h, w, st)
        h, w = 2 * h, 2 * w
        feat = conv_sb(up, *P[name], k=3, slope=P["slope_feat"], out=out)
    hr = conv_sb(feat, *P["hr"], k=3, slope=P["slope_feat"], out=ups[1][0])                   # over conv_up2's input, which is free by then
    lib().call("e4s_gsr_tail", _p(out_u8), _p(out_f), _p(hr), _p(P["last"][0]), _p(P["last"][1]), 1, C, h, w, crop[0], crop[1], int(bgr), st)


def _gsr_run(x, P, want_float, crop=None, bgr=False):
    """(float32 [bs, 3, 4h, 4w] or None, uint8 [bs, Ho, Wo, 3] or None) of the unshuffled ``x [bs, 3 r r, h, w]``, sample after sample on one sample's scratch,
    made once.  ``crop`` None: no uint8 image is wanted (the tail kernel writes one sample's worth of it as scratch)."""
    bs, _, h, w = x.shape
    C, G = P["num_feat"], GPEN_SR_GROW
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)             # noqa: E731
    out_f = new(bs, 3, 4 * h, 4 * w) if want_float else None
    Ho, Wo = (4 * h, 4 * w) if crop is None else crop
    out_u8 = torch.empty((bs if crop is not None else 1, Ho, Wo, 3), dtype=torch.uint8, device=x.device)
    slabs = [new(1, C + 4 * G, h, w) for _ in range(3)]
    reads = [[S[:, :C + k * G] for k in range(5)] for S in slabs]                             # convolution k of a dense block reads the first C + 32 k planes ...
    writes = [[S[:, C + k * G:C + (k + 1) * G] for k in range(4)] for S in slabs]             # ... and (k < 4) writes the 32 planes behind them
    feat0 = new(1, C, h, w)
    ups = [(new(1, C, 2 * h, 2 * w), new(1, C, 2 * h, 2 * w)), (new(1, C, 4 * h, 4 * w), new(1, C, 4 * h, 4 * w))]
    for b in range(bs):
        _gsr_sample(P, x[b:b + 1], out_f[b] if want_float else None, out_u8[b if crop is not None else 0], (Ho, Wo), bgr, reads, writes, feat0, ups)
    return out_f, (out_u8 if crop is not None else None)


def gpen_sr_forward(x: torch.Tensor, weights) -> torch.Tensor:
    """``RRDBNet.forward`` (sr_model/rrdbnet_arch.py:102-116) in eval mode on the device: float32 ``[bs, 3, 4h / r, 4w / r]`` from a float32 ``[bs, 3, h, w]``
    image, ``r`` = 1, 2, 4 at scale 4, 2, 1 — the input scaled by ``scale``.  ``weights``: a module with the network's keys (``GpenSRNet``, the drop-in
    ``RRDBNet``) or a mapping, bare or the checkpoint with ``params_ema`` / ``params``; the block count, ``num_feat`` (32 or 64) and the scale (conv_first's
    3, 12 or 48 input channels) are read off the keys and shapes.  Refused: ``h`` or ``w`` not divisible by ``r`` (the reference's pixel_unshuffle asserts the
    same), an output side over 16384.  The pixel-unshuffle of a float input is a strided copy by PyTorch (``gpen_sr_image`` has it fused into its input
    kernel).  A module's prepared weights are cached per parameter version; a mapping is prepared on every call.  Every convolution runs on the three-way
    split-bf16 kernel except conv_last, which is exact float32 (``e4s_gsr_tail``).  The samples of a batch run one after another on scratch that does not grow
    with ``bs``.  Forward only, no gradient.  Every argument is checked before any launch."""
    name = "gpen_sr_forward"
    checked = _validated(name, weights, _GSR_NET)
    scale = checked[1][2]
    r = _UNSHUFFLE[scale]
    _tensor_checked(name, "x", x, torch.float32, 4, "a float32 [bs, 3, h, w] image")
    bs, c3, h, w = x.shape
    if c3 != 3 or h < 1 or w < 1:
        raise ValueError(f"{name}: x: expected a float32 [bs, 3, h, w] image with h, w >= 1, got {tuple(x.shape)}")
    if h % r or w % r:
        raise ValueError(f"{name}: x is {h} x {w}: at scale {scale} the network unshuffles by {r}, which both sides must be divisible by")
    if scale * h > GPEN_SR_MAX_SIDE or scale * w > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: x is {h} x {w}: the x{scale} output may be {GPEN_SR_MAX_SIDE} x {GPEN_SR_MAX_SIDE} at the most")
    _devices_checked(name, "x", x, checked[2])
    _cuda_checked(name, x=x)
    if bs == 0:
        return torch.empty((0, 3, scale * h, scale * w), dtype=torch.float32, device=x.device)
    with torch.no_grad():
        x = x.detach()
        if r > 1:
            x = x.reshape(bs, 3, h // r, r, w // r, r).permute(0, 1, 3, 5, 2, 4).reshape(bs, 3 * r * r, h // r, w // r)
        return _gsr_run(x.contiguous(), lossnet.prepare(PreparedGpenSRNet, weights, checked), True)[0]


def gpen_sr_output_size(H: int, W: int, scale: int):
    """((Ho, Wo), (ph, pw)) of ``RealESRNet.process`` on an ``H x W`` image: the pad to a multiple of mod_scale, and ``Ho = scale (H + ph) - ph`` — the
    reference crops ``ph`` pixels of the OUTPUT, not ``scale * ph`` (real_esrnet.py:50-52), so an odd ``H`` at scale 2 gives ``2 H + 1``."""
    r = _UNSHUFFLE[scale]
    ph, pw = -H % r, -W % r
    return (scale * (H + ph) - ph, scale * (W + pw) - pw), (ph, pw)


def _image_checked(name, nm, img_u8):
    _tensor_checked(name, nm, img_u8, torch.uint8, 4, "a uint8 [bs, H, W, 3] image")
    bs, H, W, c3 = img_u8.shape
    if c3 != 3 or H < 1 or W < 1 or H > GPEN_SR_MAX_SIDE or W > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: {nm}: expected a uint8 [bs, H, W, 3] image with 1 <= H, W <= {GPEN_SR_MAX_SIDE}, got {tuple(img_u8.shape)}")
    return bs, H, W


def gpen_sr_image(img_u8: torch.Tensor, weights, bgr: bool = True) -> torch.Tensor:
    """``RealESRNet.process`` (sr_model/real_esrnet.py:26-60) for a batch on the device, as three steps: ``e4s_gsr_input`` (``/ 255``, the channel flip, the
    reflect pad to a multiple of mod_scale, the pixel-unshuffle), the network, ``e4s_gsr_tail`` (conv_last, the crop, ``clamp(0, 1)``, the flip back,
    ``(x * 255).round()``).  uint8 ``[bs, H, W, 3]`` (BGR as the reference takes it; ``bgr=False``: RGB in and out) to uint8 ``[bs, Ho, Wo, 3]`` with
    ``(Ho, Wo) = gpen_sr_output_size(H, W, scale)[0]``.  Refused with ``ValueError``: ``H <= ph`` or ``W <= pw`` (PyTorch's reflect pad raises there, in front of the
    reference's ``try``), an output side over 16384.  ``weights`` as ``gpen_sr_forward`` takes them."""
    name = "gpen_sr_image"
    checked = _validated(name, weights, _GSR_NET)
    scale = checked[1][2]
    bs, H, W = _image_checked(name, "img_u8", img_u8)
    (Ho, Wo), (ph, pw) = gpen_sr_output_size(H, W, scale)
    if H <= ph or W <= pw:
        raise ValueError(f"{name}: img_u8 is {H} x {W}: the reflect pad of {ph} x {pw} to a multiple of {_UNSHUFFLE[scale]} needs more rows / columns than that")
    if scale * (H + ph) > GPEN_SR_MAX_SIDE or scale * (W + pw) > GPEN_SR_MAX_SIDE:
        raise ValueError(f"{name}: img_u8 is {H} x {W}: the x{scale} output may be {GPEN_SR_MAX_SIDE} x {GPEN_SR_MAX_SIDE} at the most")
    _devices_checked(name, "img_u8", img_u8, checked[2])
    _cuda_checked(name, img_u8=img_u8)
    if bs == 0:
        return torch.empty((0, Ho, Wo, 3), dtype=torch.uint8, device=img_u8.device)
    r = _UNSHUFFLE[scale]
    with torch.no_grad():
        x = torch.empty((bs, 3 * r * r, (H + ph) // r, (W + pw) // r), dtype=torch.float32, device=img_u8.device)
        lib().call("e4s_gsr_input", _p(x), _p(img_u8.contiguous()), bs, H, W, r, int(bool(bgr)), _stream())
        return _gsr_run(x, lossnet.prepare(PreparedGpenSRNet, weights, checked), False, (Ho, Wo), bool(bgr))[1]


def cv_resize_linear(img_u8: torch.Tensor, dsize) -> torch.Tensor:
    """``cv2.resize(img, (Wo, Ho))`` at its default ``INTER_LINEAR`` for a batch on the device (``e4s_cv_resize_linear_u8``): uint8 ``[bs, H, W, 3]`` to uint8
    ``[bs, Ho, Wo, 3]``, ``dsize = (Wo, Ho)`` in cv2's order.  OpenCV's portable fixed-point arithmetic as tests/gpen_sr_model.py restates it; cv2 itself has
    never been run against it.  Refused: the exact 2 : 1 downscale of both sides, which OpenCV routes to ``INTER_AREA``."""
    name = "cv_resize_linear"
    bs, H, W = _image_checked(name, "img_u8", img_u8)
    try:
        Wo, Ho = dsize
    except (TypeError, ValueError):
        raise ValueError(f"{name}: dsize is a pair (Wo, Ho) of ints in 1..{GPEN_SR_MAX_SIDE}, got {dsize!r}") from None
    for v in (Wo, Ho):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= GPEN_SR_MAX_SIDE:
            raise ValueError(f"{name}: dsize is a pair (Wo, Ho) of ints in 1..{GPEN_SR_MAX_SIDE}, got {dsize!r}")
    if H == 2 * Ho and W == 2 * Wo:
        raise ValueError(f"{name}: {H} x {W} to {Ho} x {Wo} is the exact 2 : 1 downscale, which cv2 routes to INTER_AREA: not offered")
    _cuda_checked(name, img_u8=img_u8)
    out = torch.empty((bs, Ho, Wo, 3), dtype=torch.uint8, device=img_u8.device)
    lib().call("e4s_cv_resize_linear_u8", _p(out), _p(img_u8.contiguous()), bs, H, W, Ho, Wo, _stream())
    return out


__all__ = ["GPEN_SR_FEATS", "GPEN_SR_SCALES", "GpenSRNet", "PreparedGpenSRNet", "gpen_sr_state_dict_shapes", "gpen_sr_weight_tensors", "gpen_sr_output_size",
           "gpen_sr_forward", "gpen_sr_image", "cv_resize_linear"]
