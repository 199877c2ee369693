"""The RRDB network that rows f11 and f16 share: ``RRDBNet(3, 3, scale, num_feat, num_block, 32)`` of basicsr's rrdbnet_arch (the Real-ESRGAN step of the
recolouring, ``ops_recolor``: ``num_feat=64`` at scale 4) and of swap_face_fine/gpen/sr_model/rrdbnet_arch.py:64-116 (the RealESRNet pass of GPEN, ``ops_gpen_sr``:
the width and the scale read off the checkpoint).  The two differ in the ends around the network alone; here are the mirror module, the description of its
weights, their prepared form and the forward on the device, once.  At scale 2 / 1 a ``pixel_unshuffle`` by 2 / 4 stands in front of ``conv_first``, which then
has 12 / 48 input channels; the callers hand ``_run`` the unshuffled input.

A dense block's concatenations are never formed: its convolutions read the head of a ``num_feat + 128``-plane slab and write their 32 planes right behind it;
conv5 carries the block's ``* 0.2`` (folded in float64) and takes the block's input as its residual.  The convolutions run on csrc/conv.hip's three-way
split-bf16 kernel through ``lossnet.conv_sb``, the glue and the exact-float32 conv_last on csrc/rrdb.hip.  The samples of a batch run one after another on one
sample's scratch, each exactly as a batch-of-one call.  No host synchronisation; the same inputs give the same bits; after one eager call (which prepares the
weights) a call captures in a graph."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import lib
from .lossnet import conv_sb, prep_fwd
from .netweights import PreparedNet, _Net, _keys_shapes
from .ops import _p, _stream

GPEN_SR_FEATS = (32, 64)                     # num_feat: 32 as RealESRNet builds it, 64 as the published x4 checkpoints (RealESRGAN_x4plus.pth among them) have it
GPEN_SR_SCALES = (1, 2, 4)
RRDB_GROW = 32                               # num_grow_ch, the only value the references build
RRDB_SLOPE = 0.2
_UNSHUFFLE = {4: 1, 2: 2, 1: 4}              # scale -> r of pixel_unshuffle, which is also mod_scale of RealESRNet.process
_SCALE_OF_CIN = {3 * r * r: s for s, r in _UNSHUFFLE.items()}
_PREFIXES = ("params_ema.", "params.")       # a mapping may be the checkpoint itself, with the network under ``params_ema`` or ``params``


class _RDB(nn.Module):
    """``ResidualDenseBlock(num_feat, 32)`` under the references' parameter names."""

    def __init__(self, num_feat):
        super().__init__()
        for k in range(1, 6):
            setattr(self, f"conv{k}", nn.Conv2d(num_feat + (k - 1) * RRDB_GROW, RRDB_GROW if k < 5 else num_feat, 3, 1, 1))

    def forward(self, x):
        xs = [x]
        for k in range(1, 5):
            xs.append(F.leaky_relu(getattr(self, f"conv{k}")(torch.cat(xs, 1)), RRDB_SLOPE))
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
    and the timing compare ``gpen_sr_forward`` with; ``gpen_sr_forward(x, module)`` runs the same weights on the HIP kernels.  ``ops.RRDBNet(n)`` is this
    module at ``(n, 64, 4)``."""

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
        feat = F.leaky_relu(self.conv_up1(F.interpolate(feat, scale_factor=2, mode="nearest")), RRDB_SLOPE)
        feat = F.leaky_relu(self.conv_up2(F.interpolate(feat, scale_factor=2, mode="nearest")), RRDB_SLOPE)
        return self.conv_last(F.leaky_relu(self.conv_hr(feat), RRDB_SLOPE))


def gpen_sr_state_dict_shapes(num_block: int = 23, num_feat: int = 32, scale: int = 2):
    """``{key: shape}`` of ``GpenSRNet(num_block, num_feat, scale).state_dict()``, in its order."""
    _config_checked("gpen_sr_state_dict_shapes", num_block, num_feat, scale)
    return dict(_keys_shapes(GpenSRNet, num_block, num_feat, scale))


def _gsr_shapes(variant):
    return gpen_sr_state_dict_shapes(*variant)


def _blocks(name, sd, shapes="gpen_sr_state_dict_shapes"):
    """The block count read off the keys of ``sd``; ``shapes``: the public shapes function the message for a missing probe key points to."""
    for probe in ("conv_first.weight", "body.0.rdb1.conv1.weight"):
        if probe not in sd:
            raise KeyError(f"{name}: the weights lack '{probe}': expected the keys of RRDBNet (ops.{shapes}())")
    num_block = 0
    while f"body.{num_block}.rdb1.conv1.weight" in sd:
        num_block += 1
    return num_block


def _gsr_variant(name, sd):
    """(num_block, num_feat, scale) read off the keys and shapes of ``sd``: a mapping tells the scales apart through conv_first's input channels alone."""
    num_block = _blocks(name, sd)
    first = sd["conv_first.weight"]
    shape = tuple(getattr(first, "shape", ()))
    if len(shape) != 4 or shape[0] not in GPEN_SR_FEATS or shape[1] not in _SCALE_OF_CIN or shape[2:] != (3, 3):
        raise ValueError(f"{name}: 'conv_first.weight' is {getattr(first, 'dtype', type(first).__name__)} {shape}, expected float32 (num_feat, 3 | 12 | 48, 3, 3) "
                         f"with num_feat one of {GPEN_SR_FEATS}")
    return num_block, int(shape[0]), _SCALE_OF_CIN[shape[1]]


_GSR_NET = _Net("RRDBNet", _gsr_shapes, _PREFIXES, True, ("conv_first.weight",), _gsr_variant, None, ())


class _PreparedRRDB(PreparedNet):
    """The kernels' copies of the network's weights, rebuilt when a tensor changes version or storage.  ``first``, ``conv_body``, ``up1``, ``up2``, ``hr`` and
    per block three dense blocks of five convolutions, all as three-way split slabs with their biases; ``conv5`` of a dense block carries the block's ``* 0.2``
    in weight and bias (folded in float64), so that ``x5 * 0.2 + x`` is the convolution's residual epilogue; ``last`` conv_last's float32 weight and bias for
    the exact kernel; ``slope_feat`` / ``slope_grow`` the LeakyReLU as a PReLU slope vector.  A subclass names its public entry and its ``_Net``, whose variant
    is (num_block, num_feat, scale) or, for the network at width 64 and scale 4 alone, the block count."""

    __slots__ = ()

    def _build(self, sd, variant, dev):
        num_block, num_feat, scale = variant if isinstance(variant, tuple) else (variant, 64, 4)

        def conv(name, fold=None):
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            if fold is None:
                return prep_fwd(w, None, b)
            return prep_fwd(w, torch.full((w.shape[0],), fold, dtype=torch.float64, device=dev), b.double() * fold)

        body = [[[conv(f"body.{i}.rdb{r}.conv{k}", 0.2 if k == 5 else None) for k in range(1, 6)] for r in (1, 2, 3)] for i in range(num_block)]
        return dict(num_block=num_block, num_feat=num_feat, scale=scale, first=conv("conv_first"), body=body, conv_body=conv("conv_body"),
                    up1=conv("conv_up1"), up2=conv("conv_up2"), hr=conv("conv_hr"),
                    last=(sd["conv_last.weight"].contiguous(), sd["conv_last.bias"].contiguous()),
                    slope_feat=torch.full((num_feat,), RRDB_SLOPE, dtype=torch.float32, device=dev),
                    slope_grow=torch.full((RRDB_GROW,), RRDB_SLOPE, dtype=torch.float32, device=dev))


def _sample(P, x, out_f, out_u8, tail, reads, writes, feat0, ups):
    """The network behind its unshuffle on one sample ``x [1, 3 r r, h, w]``.  ``reads`` / ``writes``: the views of three ``[1, num_feat + 128, h, w]`` slabs
    (``_run``); a dense block reads the head of one (x, x1 ..) and each of its first four convolutions writes its 32 planes right behind what it read, so no
    concatenation is formed; conv5 writes the head of the NEXT slab with this slab's head as its residual.  An RRDB's input (the head of slab 0) outlives its
    three dense blocks: block 1 goes 0 -> 1, block 2 goes 1 -> 2, block 3 goes 2 -> 1, and ``e4s_esr_scale_add`` puts ``head(1) * 0.2 + head(0)`` back into
    the head of slab 0.  ``ups``: per upsampling the pair (nearest x2, convolution output) of ``[1, num_feat, 2h, 2w]`` and ``[1, num_feat, 4h, 4w]`` buffers.
    ``tail``: the caller's last kernel as (entry point, the arguments between batch size and (H, W), the arguments behind them)."""
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
    entry, before, after = tail
    lib().call(entry, _p(out_u8), _p(out_f), _p(hr), _p(P["last"][0]), _p(P["last"][1]), 1, *before, h, w, *after, st)


def _run(x, P, want_float, u8_hw, tail):
    """(float32 [bs, 3, 4h, 4w] or None, uint8 [bs, *u8_hw, 3] or None) of the unshuffled ``x [bs, 3 r r, h, w]``, sample after sample on one sample's scratch,
    made once.  ``u8_hw`` None: no uint8 image is wanted (the tail kernel writes one sample's worth of it, uncropped, as scratch).  ``tail``: as ``_sample``
    takes it."""
    bs, _, h, w = x.shape
    C, G = P["num_feat"], RRDB_GROW
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)             # noqa: E731
    out_f = new(bs, 3, 4 * h, 4 * w) if want_float else None
    out_u8 = torch.empty((bs, *u8_hw, 3) if u8_hw else (1, 4 * h, 4 * w, 3), dtype=torch.uint8, device=x.device)
    slabs = [new(1, C + 4 * G, h, w) for _ in range(3)]
    reads = [[S[:, :C + k * G] for k in range(5)] for S in slabs]                             # convolution k of a dense block reads the first C + 32 k planes ...
    writes = [[S[:, C + k * G:C + (k + 1) * G] for k in range(4)] for S in slabs]             # ... and (k < 4) writes the 32 planes behind them
    feat0 = new(1, C, h, w)
    ups = [(new(1, C, 2 * h, 2 * w), new(1, C, 2 * h, 2 * w)), (new(1, C, 4 * h, 4 * w), new(1, C, 4 * h, 4 * w))]
    for b in range(bs):
        _sample(P, x[b:b + 1], out_f[b] if want_float else None, out_u8[b if u8_hw else 0], tail, reads, writes, feat0, ups)
    return out_f, (out_u8 if u8_hw else None)
