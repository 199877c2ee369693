"""A plain CPU model of the f16 + 2 x MX-fp6 arithmetic,  a w ~ a1 w1 + fp6(a1) fp6(w - w1) + fp6(a - a1) fp6(w1),  as csrc/modconv_mx.hip (with its tile,
modconv_mx_tile.h), csrc/modconv_mx4.hip and csrc/conv_mx3.hip compute it: the scalar rules (f16 rounding, block exponents, the e2m3 conversion), the block
map of every kernel (which values share a scale), byte readers and writers of the prepared-weight layouts 1, 3, 5, 4 and 7 and of the prepared-operand map, the
emulation of a layer from the model's own operands with the three terms summed in float64 (``emulate``), its fp32-accumulated forms, the counted bar, and the
single-change mutants the bar is held against.  No GPU and no library import.  The float64 references, the epilogue and the case machinery are those of
tests/modconv_model.py and tests/conv_model.py.

Block maps (read from the sources):
  modconv_mx.hip / modconv_mx4.hip   a block = the 3 taps of one kernel row x the 8 channels of one K half of a 16-channel chunk = 24 values (positions
                                     8 t + e of 32, 24..31 zero), for the weights per (parity, co) and for the activations per OUTPUT pixel; the masked loop takes
                                     the block exponent from the fp32 maximum of |a|, the plain-convolution loop from the f16 bits of max |a1|.
  conv_mx3.hip                       activations: one PATCH pixel's 32 channels of a chunk, one scale for all nine taps that read the pixel;
                                     weights: (co, tap, the chunk's 32 channels); stride 2 (layout 5) orders its tap pairs (0,2) (6,8) (3,5) (1,7) (4,-).
  modconv_upblock_mx.hip             activations as conv_mx3.hip's, of x s[r] with r the block's one region; weights (co, transposed-conv tap, 32 channels) times the
                                     layer's scale, not blur-composed, in tap pairs that share an accumulator parity (layout 7); the blur follows on the fp32 pre-blur map.
The fused single-region ToRGB and the split-plane output of the masked kernel follow from the emulated activation (``emulate_rgb``, ``emulate_split_planes``)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import conv_model as CM
import modconv_model as MM
from conv_model import cdiv, maxdiff, randn      # noqa: F401

MX_LAYER_TOL = 2e-4          # tests/test_gpu_mx.py: the f16 + fp6 layer against float64, of the output scale
U = 2.0 ** -24
CKS = 16                     # channels per chunk of modconv_mx.hip
CK3 = 32                     # ... of conv_mx3.hip
F16_LIMIT = 65520.0          # the smallest magnitude f16 rounds to infinity (the tie between 65504 and 2^16)
S2TAP = ((0, 2), (6, 8), (3, 5), (1, 7), (4, 9))      # conv_mx3.hip, stride 2: unit u, K half d -> tap (9: none)


# ================================================================================================ scalar rules
def f16(a):
    """Round to nearest even into f16 (numpy converts float32 and float64 directly, one rounding)."""
    return np.asarray(a).astype(np.float16)


def f16_trunc(a):
    """f16 by truncation (a mutant's rule)."""
    a = np.asarray(a, dtype=np.float64)
    h = a.astype(np.float16)
    bits = h.view(np.uint16).copy()
    over = np.abs(h.astype(np.float64)) > np.abs(a)
    bits = np.where(over, bits - 1, bits).astype(np.uint16)        # one step towards zero: the magnitude bits order like integers
    return bits.view(np.float16)


def fl32(a):
    return np.asarray(a).astype(np.float32)


def exp_field32(m):
    """Biased exponent field of an fp32 value."""
    return ((np.ascontiguousarray(m, dtype=np.float32).view(np.uint32) >> 23) & 0xff).astype(np.int64)


def exp_field16(h):
    """fp32-biased exponent of an f16 value as the plain-convolution loops take it from the bits: the field, 0 counted as 1, + 112."""
    e16 = ((np.ascontiguousarray(h, dtype=np.float16).view(np.uint16) >> 10) & 31).astype(np.int64)
    return np.where(e16 == 0, 1, e16) + 112


def e1_rule(ex):
    """Block scale 2^(E - 2) of a value set whose largest magnitude has the biased exponent ``ex``: the maximum lands in [4, 8) of e2m3."""
    ex = np.asarray(ex, dtype=np.int64)
    return np.where(ex > 3, ex - 2, 1)


def e2_rule(ex, off=13):
    """Block scale 2^(E - 13) of the activation residuals (|a - a1| <= 2^(E - 11))."""
    ex = np.asarray(ex, dtype=np.int64)
    return np.where(ex > off + 1, ex - off, 1)


def stored_w_e2(e2):
    """The weight residual went through f16 scaled by 2^12: its stored scale is e2 - 12, floored at 0."""
    e2 = np.asarray(e2, dtype=np.int64)
    return np.where(e2 > 12, e2 - 12, 0)


def guard(a):
    """Does a modulated / normalised activation leave the f16 range?  |a| >= 65520 (``amax >= 65520.f``; the f16 exponent field 31 of a1 in the ``ENC`` loops)."""
    return np.abs(np.asarray(a, dtype=np.float64)) >= F16_LIMIT


# ------------------------------------------------------------------------------------------------ e2m3 under a power-of-two scale (OCP MX v1.0)
E2M3 = np.array([m / 8.0 for m in range(8)] + [(1 + m / 8.0) * 2.0 ** (e - 1) for e in (1, 2, 3) for m in range(8)])      # code & 31 -> magnitude


def e2m3_value(codes):
    codes = np.asarray(codes).astype(np.int64)
    return np.where(codes & 32, -1.0, 1.0) * E2M3[codes & 31]


def fp6_value(codes, e):
    """The value an fp6 operand stands for under the E8M0 scale byte ``e``."""
    return np.ldexp(e2m3_value(codes), np.asarray(e, dtype=np.int64) - 127)


def quant_e2m3(v, e, rounding="rne", overflow="sat"):
    """Codes (uint8, bit 5 = sign, bits 4:3 exponent, bits 2:0 mantissa) of ``v`` / 2^(e - 127): round to nearest even onto the e2m3 grid (steps of 1/8 below
    2 — subnormals kept —, 1/4 below 4, 1/2 below 8), saturating at +-7.5; the sign of a zero is kept.  ``rounding`` "trunc" / "away" and ``overflow`` "wrap"
    (the exponent field overflows into nothing) are the mutants' rules."""
    v = np.asarray(v, dtype=np.float64)
    t = np.ldexp(v, 127 - np.asarray(e, dtype=np.int64))
    mag = np.abs(t)
    step = np.where(mag < 2, 0.125, np.where(mag < 4, 0.25, 0.5))
    n = mag / step
    n = {"rne": np.rint, "trunc": np.floor, "away": lambda q: np.floor(q + 0.5)}[rounding](n)
    q = n * step
    if overflow == "sat":
        q = np.minimum(q, 7.5)
    fr, xp = np.frexp(np.maximum(q, 1.0))                # q = fr 2^xp, fr in [0.5, 1)
    ef = xp                                              # exponent field of a normal: floor(log2 q) + 1
    man = np.rint((q / np.ldexp(1.0, ef - 1) - 1.0) * 8).astype(np.int64)
    code = np.where(q < 1, np.rint(q * 8).astype(np.int64), (ef.astype(np.int64) << 3) | man)
    code = code & 31
    return (code | np.where(np.signbit(v), 32, 0)).astype(np.uint8)


def pack_codes(codes):
    """32 six-bit codes ``[..., 32]`` -> 24 bytes ``[..., 24]``: code i in bits 6 i .. 6 i + 5, little-endian (``v_cvt_scalef32_pk32_fp6_f16``)."""
    bits = np.unpackbits(np.ascontiguousarray(codes, dtype=np.uint8)[..., None], axis=-1, bitorder="little")[..., :6]
    return np.packbits(bits.reshape(codes.shape[:-1] + (192,)), axis=-1, bitorder="little")


def unpack_codes(b):
    bits = np.unpackbits(np.ascontiguousarray(b, dtype=np.uint8), axis=-1, bitorder="little").reshape(b.shape[:-1] + (32, 6))
    return np.packbits(bits, axis=-1, bitorder="little")[..., 0]


# ================================================================================================ blocks of 32 values
def encode_weight_blocks(V, rounding="rne", overflow="sat", forget12=False):
    """Blocks ``[..., 32]`` of fp32 weights (zeros where a position holds nothing) as the prep kernels make them: w1 = f16(w), the residual
    f16((w - w1) 4096), converted under 2^(E - 2) of the largest |w1| and of the largest fp32 |(w - w1) 4096|; the residual's stored scale takes the 2^12 back out."""
    V = fl32(V)
    w1 = f16(V)
    r32 = fl32((V - w1.astype(np.float32)) * np.float32(4096.0))       # (w - w1 is exact in fp32)
    r = f16(r32)
    e1 = e1_rule(exp_field32(np.abs(w1.astype(np.float32)).max(-1)))
    e2 = e1_rule(exp_field32(np.abs(r32).max(-1)))                     # the largest fp32 residual, BEFORE its f16 rounding: one that rounds up to 2^(E + 1) saturates at 7.5
    c0 = quant_e2m3(w1.astype(np.float64), e1[..., None], rounding, overflow)
    c1 = quant_e2m3(r.astype(np.float64), e2[..., None], rounding, overflow)
    sc = np.stack([e1, e2 if forget12 else stored_w_e2(e2)], -1).astype(np.uint8)
    return dict(w1=w1.view(np.uint16), c0=c0, c1=c1, sc=sc)


def block_values(blk):
    """(w1, fp6(w1), fp6(w - w1)) of weight blocks, or (a1, fp6(a1), fp6(a - a1)) of activation blocks, as float64 ``[..., 32]``."""
    w1 = np.ascontiguousarray(blk["w1"]).view(np.float16).astype(np.float64)
    return w1, fp6_value(blk["c0"], blk["sc"][..., 0:1]), fp6_value(blk["c1"], blk["sc"][..., 1:2])


def encode_act_pixels(a, rounding="rne", overflow="sat"):
    """``encode32`` of conv_mx3.hip on blocks ``[..., 32]`` of fp32 activations: a1 = f16(a), the residual f16(a - a1) (the difference is exact in fp32), the
    scales 2^(E - 2) / 2^(E - 13) from the f16 bits of the largest |a1|.  A zero pixel gets the scale bytes (111, 100)."""
    a = fl32(a)
    a1 = f16(a)
    r = f16(a - a1.astype(np.float32))
    ex = exp_field16(np.abs(a1).max(-1))
    e1, e2 = e1_rule(ex), e2_rule(ex)
    c0 = quant_e2m3(a1.astype(np.float64), e1[..., None], rounding, overflow)
    c1 = quant_e2m3(r.astype(np.float64), e2[..., None], rounding, overflow)
    return dict(w1=a1.view(np.uint16), c0=c0, c1=c1, sc=np.stack([e1, e2], -1).astype(np.uint8))


# ================================================================================================ block maps and byte layouts of the prepared weights
# layout -> (output channels per tile, 16-byte f16 segments per block, order of the f16 part, bytes of the scale section)
LAYOUTS = {1: (128, 3, "seg_half", 1024), 4: (64, 3, "seg_half", 1024), 3: (128, 4, "half_seg", 1024), 5: (128, 4, "half_seg", 1024), 7: (64, 4, "half_seg", 1024)}


def block_index(layout, npar, cout, cin):
    """The block map of a prepared-weight layout: int64 ``[slot dims..., K half 2, co TN, 32]`` = index of every block position into the dense weight
    ``[npar, cout, cin, 9]`` flattened, -1 where the position holds nothing (positions 24..31, channel and output-channel tails, tap 9).
    Slot dims: 1: (parity, chunk, co tile, kernel row); 4: (chunk, 64-co tile, kernel row, parity); 3 / 5 / 7: (chunk, co tile, unit) — 7 (modconv_upblock_mx.hip:
    the transposed-conv taps times the layer's scale, NOT blur-composed, 64-co tiles) pairs its taps as the stride-2 form does: (0,2) (6,8) (3,5) (1,7) (4,-)."""
    tn = LAYOUTS[layout][0]
    ntile = cdiv(cout, tn)
    if layout in (1, 4):
        nchunk = cdiv(cin, CKS)
        dims = (npar, nchunk, ntile, 3) if layout == 1 else (nchunk, ntile, 3, npar)
        g = np.indices(dims + (2, tn, 32))
        if layout == 1:
            par, chunk, tile, row = g[0], g[1], g[2], g[3]
        else:
            chunk, tile, row, par = g[0], g[1], g[2], g[3]
        half, n, p = g[4], g[5], g[6]
        ci = chunk * CKS + half * 8 + (p & 7)
        tap = row * 3 + (p >> 3)
        live = (p < 24) & (ci < cin)
    else:
        assert npar == 1 and cin % CK3 == 0
        nchunk = cin // CK3
        g = np.indices((nchunk, ntile, 5, 2, tn, 32))
        chunk, tile, unit, half, n, p = g
        par = np.zeros_like(p)
        ci = chunk * CK3 + p
        tap = (2 * unit + half) if layout == 3 else np.asarray(S2TAP)[unit, half]          # (ux_tap_ky / ux_tap_kx of layout 7 give the same pairs)
        live = tap < 9
    co = tile * tn + n
    live = live & (co < cout)
    idx = ((par * cout + co) * cin + ci) * 9 + tap
    return np.where(live, idx, -1)


def to_blocks(dense, idx):
    """Dense ``[npar, cout, cin, 9]`` -> blocks (zeros where ``idx`` is -1)."""
    flat = np.concatenate([np.asarray(dense).reshape(-1), np.zeros(1, dtype=np.asarray(dense).dtype)])
    return flat[idx]


def from_blocks(vals, idx, shape):
    """Block values ``[..., 32]`` (or one value per block ``[...]``) back on the dense grid."""
    vals = np.asarray(vals)
    if vals.ndim == idx.ndim - 1:
        vals = np.broadcast_to(vals[..., None], idx.shape)
    out = np.zeros(int(np.prod(shape)) + 1, dtype=vals.dtype)
    out[idx.reshape(-1)] = vals.reshape(-1)
    return out[:-1].reshape(shape)


def weight_bytes_of(blk, layout):
    """Blocks ``[slots..., 2, TN, ...]`` -> the bytes of the prepared tensor.  A slot: f16 part (layouts 1 / 4: [tap][half][co] x 16 B; 3 / 5: [half][K-step, k half]
    [co] x 16 B) | first 16 code bytes [term][half][co] | last 8 [term][half][co] | scales [half][co] x 4 B (byte 0: fp6(w1), byte 1: fp6(w - w1)), zero-padded."""
    tn, nseg, order, scb = LAYOUTS[layout]
    w1 = blk["w1"]
    S = w1.shape[:-3]
    ns = len(S)
    seg = w1[..., : 8 * nseg].reshape(S + (2, tn, nseg, 8))
    seg = np.moveaxis(seg, ns + 2, ns) if order == "seg_half" else np.moveaxis(seg, ns + 2, ns + 1)        # -> [seg][half][co] / [half][seg][co]
    w1b = np.ascontiguousarray(seg).astype("<u2").view(np.uint8).reshape(S + (-1,))
    cb = pack_codes(np.stack([blk["c0"], blk["c1"]], ns))                                                  # [slots, term, half, co, 24]
    sc = np.zeros(S + (2, tn, 4), dtype=np.uint8)
    sc[..., 0:2] = blk["sc"]
    scs = sc.reshape(S + (-1,))
    pad = np.zeros(S + (scb - scs.shape[-1],), dtype=np.uint8)
    return np.concatenate([w1b, np.ascontiguousarray(cb[..., :16]).reshape(S + (-1,)), np.ascontiguousarray(cb[..., 16:]).reshape(S + (-1,)), scs, pad], -1).reshape(-1)


def slot_dims(layout, npar, cout, cin):
    tn = LAYOUTS[layout][0]
    ntile = cdiv(cout, tn)
    if layout == 1:
        return (npar, cdiv(cin, CKS), ntile, 3)
    if layout == 4:
        return (cdiv(cin, CKS), ntile, 3, npar)
    return (cin // CK3, ntile, 5)


def read_weight_bytes(b, layout, npar, cout, cin):
    """The inverse of ``weight_bytes_of``: w1 halves (uint16), fp6 codes and E8M0 bytes per block position; positions the layout does not store read as 0."""
    tn, nseg, order, scb = LAYOUTS[layout]
    S = slot_dims(layout, npar, cout, cin)
    ns = len(S)
    n_w1, n_lo, n_hi = nseg * 2 * tn * 16, 2 * 2 * tn * 16, 2 * 2 * tn * 8
    b = np.asarray(b, dtype=np.uint8).reshape(S + (n_w1 + n_lo + n_hi + scb,))
    seg = np.ascontiguousarray(b[..., :n_w1]).view("<u2").reshape(S + ((nseg, 2, tn, 8) if order == "seg_half" else (2, nseg, tn, 8)))
    seg = np.moveaxis(seg, ns, ns + 2) if order == "seg_half" else np.moveaxis(seg, ns + 1, ns + 2)        # -> [half][co][seg][8]
    w1 = np.zeros(S + (2, tn, 32), dtype=np.uint16)
    w1[..., : 8 * nseg] = seg.reshape(S + (2, tn, 8 * nseg))
    lo = b[..., n_w1:n_w1 + n_lo].reshape(S + (2, 2, tn, 16))
    hi = b[..., n_w1 + n_lo:n_w1 + n_lo + n_hi].reshape(S + (2, 2, tn, 8))
    codes = unpack_codes(np.concatenate([lo, hi], -1))
    sc = b[..., n_w1 + n_lo + n_hi:n_w1 + n_lo + n_hi + 2 * tn * 4].reshape(S + (2, tn, 4))
    return dict(w1=w1, c0=np.take(codes, 0, ns), c1=np.take(codes, 1, ns), sc=np.ascontiguousarray(sc[..., 0:2]))


def dense_weight32(W, layout, blur=None, scale=None):
    """The fp32 weight the prep kernel splits, ``[npar, cout, cin, 9]``: a ModulatedConv2d weight times the equalised-lr scale (``scale`` None: 1 / sqrt(9 cin) in
    fp32), up layers blur-composed per parity in the kernel's FMA order; a plain convolution weight as it is (``scale`` 1)."""
    W = W.float()
    cin = W.shape[1]
    sc = torch.tensor(MM.scale32(cin) if scale is None else np.float32(scale))
    wf = MM.compose32(W, blur) if blur is not None else W.flatten(2)[None]
    return (wf * sc).numpy()


def model_weights(W, layout, blur=None, scale=None, **mut):
    """(blocks, block map) of the model for a weight: what ``PreparedMx.get`` must hold, byte for byte (``weight_bytes_of``)."""
    wf = dense_weight32(W, layout, blur, scale)
    idx = block_index(layout, wf.shape[0], wf.shape[1], wf.shape[2])
    return encode_weight_blocks(to_blocks(wf, idx), **mut), idx, wf.shape


def dense_terms(blk, idx, shape):
    """(w1, fp6(w1), fp6(w - w1)) on the dense grid, float64 tensors."""
    return tuple(torch.from_numpy(from_blocks(v, idx, shape)) for v in block_values(blk))


# ------------------------------------------------------------------------------------------------ the prepared-operand map
PREPB = 116


def read_operand_map(data, bs, c, h, w):
    """``ops.MxOperandMap.data`` (float32 ``[bs, c / 32, 29 h w]``, any tensor or array of those bytes) -> blocks per (image, 32-channel block, pixel in the
    map's own pixel order): per block 64 hw B of f16 ([slot 4][pixel] x 16 B), two code sets ([pixel] x 16 B each), their tails ([pixel] x (8 + 8) B), scales
    ([pixel] x 4 B: byte 0 for fp6(a1), byte 1 for fp6(a - a1))."""
    hw = h * w
    raw = data.detach().cpu().contiguous().numpy() if isinstance(data, torch.Tensor) else np.ascontiguousarray(data)
    b = raw.view(np.uint8).reshape(bs, c // 32, PREPB * hw)
    a1 = np.ascontiguousarray(b[..., : 64 * hw]).view("<u2").reshape(bs, c // 32, 4, hw, 8)
    a1 = np.moveaxis(a1, 2, 3).reshape(bs, c // 32, hw, 32)
    lo = b[..., 64 * hw:96 * hw].reshape(bs, c // 32, 2, hw, 16)
    hi = b[..., 96 * hw:112 * hw].reshape(bs, c // 32, hw, 2, 8)
    codes = unpack_codes(np.concatenate([lo, np.moveaxis(hi, 3, 2)], -1))
    sc = b[..., 112 * hw:].reshape(bs, c // 32, hw, 4)
    return dict(w1=np.ascontiguousarray(a1), c0=codes[:, :, 0], c1=codes[:, :, 1], sc=np.ascontiguousarray(sc[..., 0:2])), np.ascontiguousarray(sc[..., 2:4])


def operand_map_bytes(blk):
    """The writer of the same layout (bytes 2 and 3 of a scale word: zero)."""
    bs, nb, hw = blk["w1"].shape[:3]
    a1 = np.moveaxis(blk["w1"].reshape(bs, nb, hw, 4, 8), 3, 2)
    cb = pack_codes(np.stack([blk["c0"], blk["c1"]], 2))                   # [bs, nb, term, hw, 24]
    sc = np.zeros((bs, nb, hw, 4), dtype=np.uint8)
    sc[..., 0:2] = blk["sc"]
    parts = [np.ascontiguousarray(a1).astype("<u2").view(np.uint8).reshape(bs, nb, -1), np.ascontiguousarray(cb[..., :16]).reshape(bs, nb, -1),
             np.ascontiguousarray(np.moveaxis(cb[..., 16:], 2, 3)).reshape(bs, nb, -1), sc.reshape(bs, nb, -1)]
    return np.concatenate(parts, -1)


def model_operand_map(act, phased=False):
    """Blocks of a map ``[bs, c, h, w]`` of fp32 activations in the pixel order of the map (``phased``: the four phase planes (py, px) one after the other)."""
    bs, c, h, w = act.shape
    a = act.float()
    if phased:
        a = torch.stack([a[:, :, py::2, px::2] for py in (0, 1) for px in (0, 1)], 2)
    a = a.reshape(bs, c // 32, 32, h * w).permute(0, 1, 3, 2).contiguous().numpy()
    return encode_act_pixels(a)


# ================================================================================================ the operation
def _unfold(x, stride=1):
    """``[bs, cin, h, w]`` -> ``[bs, cin, 9, ho, wo]``: the nine zero-padded taps of every output pixel."""
    h, w = x.shape[2:]
    ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.stack([xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(3) for kx in range(3)], 2)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _row_blocks(a, group="row"):
    """Largest |value| of every block of ``a [P, bs, cin, 9, h, w]``, broadcast back: ``row`` = (chunk, K half, kernel row) = 8 channels x 3 taps; the mutants'
    ``tap`` = 8 channels of one tap, ``halves`` = the 16 channels of the chunk x 3 taps."""
    P, bs, cin, _, h, w = a.shape
    v = np.abs(a).reshape(P, bs, cin // CKS, 2, 8, 3, 3, h, w)
    axes = {"row": (4, 6), "tap": (4,), "halves": (3, 4, 6)}[group]
    return np.broadcast_to(v.max(axes, keepdims=True), v.shape).reshape(a.shape)


def _masked_acts(c, rm, resid="fma", a1_rule="rne", group="row", e1_shift=0, e2_off=13, rounding="rne", overflow="sat", none_row0=False):
    """The masked loop's operands on the unfolded grid ``[P, bs, cin, 9, h, w]`` (P: 1, or the four parities of a composed up layer): a = fl32(x s) with s the
    modulation of the OUTPUT pixel's region (zeros without one), a1 = f16(a), the residual f16(fma(x, s, -a1)) — the product not rounded before the
    subtraction, the difference rounded to fp32 and then to f16 (v_fma_mix) —, block exponents from the fp32 maximum of |a| over the row's 24 values."""
    x, s = c["x"].float(), c["s"].float()
    xu = MM._unfold(x).double()
    sp = MM._gather(s, rm.clamp(min=0) if none_row0 else rm).double()
    sps = [sp[:, :, None, (p >> 1)::2, (p & 1)::2] for p in range(4)] if c["up"] else [sp[:, :, None]]
    prod = torch.stack([xu * q for q in sps]).numpy()                 # exact: 24 x 24 bits
    a = fl32(prod)
    a1 = (f16 if a1_rule == "rne" else f16_trunc)(a)
    a1d = a1.astype(np.float64)
    r = f16(fl32((prod if resid == "fma" else a.astype(np.float64)) - a1d))
    ex = exp_field32(_row_blocks(a, group))
    e1, e2 = e1_rule(ex) + e1_shift, e2_rule(ex, e2_off)
    f1 = fp6_value(quant_e2m3(a1d, e1, rounding, overflow), e1)
    f2 = fp6_value(quant_e2m3(r.astype(np.float64), e2, rounding, overflow), e2)
    return dict(a=a, a1=a1d, f1=f1, f2=f2)


def norm32(x, in_norm, form):
    """The plain-convolution loops' normalised input in fp32 (float64 array out): ``form`` "sub" = fl32(fl32(x - mean) rstd) (modconv_mx_tile.h), "fma" =
    fl32(fma(x, rstd, fl32(-mean rstd))) (conv_mx3.hip); without statistics x itself."""
    xd = _np(x).astype(np.float64)
    if in_norm is None:
        return fl32(xd)
    m, r = (_np(t).astype(np.float64)[:, :, None, None] for t in in_norm)
    if form == "sub":
        return fl32(fl32(xd - m).astype(np.float64) * r)
    return fl32(xd * r + fl32(-m * r).astype(np.float64))


def _enc_acts(c, kernel, stride, group="row", e1_shift=0, e2_off=13, rounding="rne", overflow="sat", a1_rule="rne", norm_after_f16=False):
    """The plain-convolution operands on the unfolded grid ``[1, bs, cin, 9, ho, wo]``.  ``conv_mx`` (the one-phase kernel): blocks as the masked loop's, the
    exponent from the f16 bits of max |a1|; ``conv_mx3``: every input pixel's 32 channels of a chunk converted once, whichever tap reads it."""
    x = c["x"]
    if norm_after_f16:
        x = torch.from_numpy(f16(_np(x)).astype(np.float32))
    a = norm32(x, c["in_norm"], "sub" if kernel == "conv_mx" else "fma")
    a1 = (f16 if a1_rule == "rne" else f16_trunc)(a)
    a1d = a1.astype(np.float64)
    r = f16(fl32(a.astype(np.float64) - a1d))
    unf = lambda v: _unfold(torch.from_numpy(np.ascontiguousarray(v)), stride)[None].numpy()      # noqa: E731
    if kernel == "conv_mx":
        ua1, ur = unf(a1d), unf(r.astype(np.float64))
        ex = exp_field16(f16(_row_blocks(ua1, group)))
        e1, e2 = e1_rule(ex) + e1_shift, e2_rule(ex, e2_off)
        return dict(a=unf(a.astype(np.float64)), a1=ua1, f1=fp6_value(quant_e2m3(ua1, e1, rounding, overflow), e1), f2=fp6_value(quant_e2m3(ur, e2, rounding, overflow), e2))
    bs, cin, h, w = a.shape
    blk = np.abs(a1d).reshape(bs, cin // CK3, CK3, h, w)
    if group == "window":        # mutant: the scale of an OUTPUT pixel's 3 x 3 window instead of the patch pixel's own
        m = torch.from_numpy(blk.max(2))
        m = F.max_pool2d(m, 3, 1, 1).numpy()
    elif group == "k16":         # mutant: a scale per 16-channel K step
        m = np.broadcast_to(blk.reshape(bs, cin // 16, 16, h, w).max(2, keepdims=True), (bs, cin // 16, 16, h, w)).reshape(bs, cin, h, w)
    else:
        m = blk.max(2)
    if group != "k16":
        m = np.broadcast_to(m[:, :, None], blk.shape).reshape(bs, cin, h, w)
    ex = exp_field16(f16(m))
    e1, e2 = e1_rule(ex) + e1_shift, e2_rule(ex, e2_off)
    f1 = fp6_value(quant_e2m3(a1d, e1, rounding, overflow), e1)
    f2 = fp6_value(quant_e2m3(r.astype(np.float64), e2, rounding, overflow), e2)
    return dict(a=unf(a.astype(np.float64)), a1=unf(a1d), f1=unf(f1), f2=unf(f2))


def _kmask(cin, chunk_of, lose):
    """1 / 0 per (channel, tap): what a partial loss of a correction term keeps.  ``lose``: ("chunk", -1) the last chunk, ("row", 2), ("half", 1)."""
    m = torch.ones(cin, 9, dtype=torch.float64)
    kind, which = lose
    if kind == "chunk":
        nch = cin // chunk_of
        m[(which % nch) * chunk_of:(which % nch + 1) * chunk_of] = 0
    elif kind == "row":
        m[:, 3 * which:3 * which + 3] = 0
    elif kind == "half":
        ci = torch.arange(cin)
        m[(ci % 16) // 8 == which] = 0
    elif kind == "all":
        m.zero_()
    return m


def _sum(c, wd, xa):
    """sum_{ci, tap} of weight ``[P, cout, cin, 9]`` times activation ``[P, bs, cin, 9, h, w]`` in float64 -> ``[bs, cout, ho, wo]`` (parities interleaved)."""
    xa = torch.from_numpy(np.ascontiguousarray(xa)) if not isinstance(xa, torch.Tensor) else xa
    P = wd.shape[0]
    ys = [torch.einsum("ock,bckhw->bohw", wd[p], xa[p]) for p in range(P)]
    if P == 1:
        return ys[0]
    bs, co, h, w = ys[0].shape
    out = torch.empty((bs, co, 2 * h, 2 * w), dtype=torch.float64)
    for p in range(4):
        out[:, :, (p >> 1)::2, (p & 1)::2] = ys[p]
    return out


KERNELS = ("modconv_mx", "mx4", "conv_mx", "conv_mx3", "conv_mx3_s2", "upblock")
# fp32 additions on an accumulator's chain per chunk, every MFMA's K counted in full: modconv_mx / mx4 / conv_mx — a 16-channel chunk is three kernel rows of
# three f16 MFMAs (K = 16) and two fp6 MFMAs (K = 64): 3 (3 x 16 + 2 x 64) = 528; conv_mx3 — a 32-channel chunk is five units of four (the last: two) f16 MFMAs
# (K = 16) and two fp6 MFMAs (K = 64): 4 (64 + 128) + (32 + 128) = 928.
# upblock — a 32-channel chunk adds to the accumulator of pre-blur parity (0, 0) two units of four f16 MFMAs and two fp6 MFMAs, 2 (64 + 128) = 384 (the other
# parities take one unit each); the pre-blur value is stored as fp32 (1), the blur is a chain of 16 FMAs, then the masked epilogue.
D_CHUNK = {"modconv_mx": 528, "mx4": 528, "conv_mx": 528, "conv_mx3": 928, "conv_mx3_s2": 928, "upblock": 384}
D_EPILOGUE = {"modconv_mx": 5, "mx4": 5, "conv_mx": 1, "conv_mx3": 1, "conv_mx3_s2": 1, "upblock": 1 + 16 + 5}      # demodulation, noise, bias, leaky slope, gain / the PReLU slope


def mx_ksplit(c):
    """K slices of the launch ``ops.region_modconv3x3(mx=...)`` makes (``launch_modconv_mx``: one workgroup per CU, split until one round of the chip is full)."""
    if c.get("rgb") is not None or c.get("uni_blocks"):          # the fused ToRGB needs the whole sum in one workgroup; a layer that shares its map with the block kernel gives up its K split
        return 1
    ho, wo = MM.out_hw(c)
    out_floats = c["bs"] * c["cout"] * ho * wo
    ws = 16 * out_floats if out_floats <= MM.SPLITK_MAX_OUT_FLOATS else 0
    base = cdiv(c["w"], 32) * cdiv(c["h"], 8) * (4 if c["up"] else 1) * cdiv(c["cout"], 128) * c["bs"]
    nchunk, k = cdiv(c["cin"], CKS), 1
    if ws and base < 384:
        while k < 16 and base * k * 2 <= 256 and k * 2 <= nchunk and k * 2 * out_floats <= ws:
            k *= 2
    return k


def chain_length(c, kernel):
    """D of the bar: the additions of one output's longest accumulator chain, the split-K sum and the epilogue's roundings."""
    if kernel in ("modconv_mx", "mx4"):
        k = 1 if kernel == "mx4" else mx_ksplit(c)
        return D_CHUNK[kernel] * cdiv(cdiv(c["cin"], CKS), k) + k + D_EPILOGUE[kernel]
    return D_CHUNK[kernel] * (c["cin"] // (CKS if kernel == "conv_mx" else CK3)) + D_EPILOGUE[kernel]


def _emulate_upblock(c, lose1=None, lose2=None, swap_pairs=False, forget12=False, resid="fma", a1_rule="rne", e1_shift=0, e2_off=13, rounding="rne", overflow="sat", **unused):
    """The region-uniform block kernel (csrc/modconv_upblock_mx.hip) on a map whose 16 x 16 output blocks carry one region each: per region r the single-region
    layer on x s[r] — every patch pixel's 32 channels of a chunk converted once (a1 = f16(fl32(x s)), the residual f16(fma(x, s, -a1)), the scales from the f16
    bits of max |a1|), the transposed-conv taps of layout 7, the pre-blur map rounded to fp32, the blur — selected block by block."""
    assert c["up"]
    rm = MM.region_map(c)
    blk, idx, shape = model_weights(c["W"], 7, forget12=forget12, rounding=rounding, overflow=overflow)
    w1, q0, q1 = (t[0].reshape(shape[1], shape[2], 3, 3) for t in dense_terms(blk, idx, shape))
    cin = shape[2]
    k1 = _kmask(cin, CK3, lose1).reshape(cin, 3, 3) if lose1 else 1.0
    k2 = _kmask(cin, CK3, lose2).reshape(cin, 3, 3) if lose2 else 1.0
    x = c["x"].double().numpy()
    bs, _, h, w = x.shape
    out_raw = torch.zeros((bs, shape[1], 2 * h, 2 * w), dtype=torch.float64)
    out_mag = torch.zeros_like(out_raw)
    tconv = lambda a, wt: F.conv_transpose2d(torch.from_numpy(np.ascontiguousarray(a)), wt.transpose(0, 1).contiguous(), stride=2)      # noqa: E731
    ovf = False
    for r in range(c["nreg"]):
        sel = (rm == r)[:, None]
        if not sel.any():
            continue
        prod = x * c["s"][:, r].double().numpy()[:, :, None, None]
        a = fl32(prod)
        ovf = ovf or bool(guard(a).any())
        a1 = (f16 if a1_rule == "rne" else f16_trunc)(a)
        a1d = a1.astype(np.float64)
        res = f16(fl32((prod if resid == "fma" else a.astype(np.float64)) - a1d)).astype(np.float64)
        m = np.abs(a1d).reshape(bs, cin // CK3, CK3, h, w).max(2, keepdims=True)
        ex = exp_field16(f16(np.broadcast_to(m, (bs, cin // CK3, CK3, h, w)).reshape(a.shape)))
        e1, e2 = e1_rule(ex) + e1_shift, e2_rule(ex, e2_off)
        f1 = fp6_value(quant_e2m3(a1d, e1, rounding, overflow), e1)
        f2 = fp6_value(quant_e2m3(res, e2, rounding, overflow), e2)
        if swap_pairs:
            f1, f2 = f2, f1
        z = tconv(a1d, w1) + tconv(f1, q1 * k1) + tconv(f2, q0 * k2)
        zm = tconv(np.abs(a1d), w1.abs()) + tconv(np.abs(f1), (q1 * k1).abs()) + tconv(np.abs(f2), (q0 * k2).abs())
        out_raw = out_raw + MM._blur64(c, z.float().double()) * sel
        out_mag = out_mag + MM.O.upfirdn2d(zm, c["blur"].double().abs(), pad=(1, 1)) * sel
    out = MM._epilogue(c, out_raw, rm)
    mg = out_mag * (MM._gather(c["d"].double().abs(), rm) if c["d"] is not None else (rm >= 0)[:, None].double())
    if c["noise"] is not None:
        mg = mg + (c["noise_weight"].double() * c["noise"].double().reshape(c["noise"].shape[0], 1, *out_raw.shape[2:])).abs()
    if c["bias"] is not None:
        mg = mg + c["bias"].double().abs()[None, :, None, None]
    if c["act"]:
        mg = mg * MM.SQRT2
    D = chain_length(c, "upblock")
    return dict(out=out, bar=D * U * mg, guard=ovf, D=D, raw=out_raw)


# every mutant: name -> (family it applies to: "mod" / "enc" / "both", keywords of ``emulate``)
MUTANTS = {
    "fp6(a - a1) fp6(w1) lost": ("both", dict(lose2=("all", 0))),
    "fp6(a1) fp6(w - w1) lost": ("both", dict(lose1=("all", 0))),
    "fp6(a - a1) fp6(w1) lost in the last chunk": ("both", dict(lose2=("chunk", -1))),
    "fp6(a1) fp6(w - w1) lost in the last chunk": ("both", dict(lose1=("chunk", -1))),
    "fp6(a - a1) fp6(w1) lost in kernel row 2": ("both", dict(lose2=("row", 2))),
    "fp6(a1) fp6(w - w1) lost in kernel row 2": ("both", dict(lose1=("row", 2))),
    "fp6(a - a1) fp6(w1) lost in K half 1": ("both", dict(lose2=("half", 1))),
    "fp6(a1) fp6(w - w1) lost in K half 1": ("both", dict(lose1=("half", 1))),
    "fp6 operand sets paired the wrong way round": ("both", dict(swap_pairs=True)),
    "activation block exponent one too large": ("both", dict(e1_shift=1)),
    "activation block exponent one too small": ("both", dict(e1_shift=-1)),
    "activation residual scale E - 12": ("both", dict(e2_off=12)),
    "weight residual's -12 forgotten": ("both", dict(forget12=True)),
    "scale per tap (8 values) instead of per row (24)": ("mod", dict(group="tap")),
    "scale shared by the two K halves": ("mod", dict(group="halves")),
    "conv_mx3: scale of the output pixel's window instead of the patch pixel's": ("mx3", dict(group="window")),
    "conv_mx3: scale per 16-channel K step instead of per pixel": ("mx3", dict(group="k16")),
    "fp6 conversion truncates": ("both", dict(rounding="trunc")),
    "fp6 conversion rounds half away": ("both", dict(rounding="away")),
    "fp6 conversion wraps instead of saturating": ("both", dict(overflow="wrap")),
    "a1 by truncation": ("both", dict(a1_rule="trunc")),
    "residual from the rounded product": ("mod", dict(resid="rounded")),
    "region-less pixel modulated by row 0": ("mod", dict(none_row0=True)),
    "in-norm applied after the f16 rounding": ("enc", dict(norm_after_f16=True)),
    "stride-2 tap order of layout 5 read as layout 3": ("s2", dict(weight_layout=3)),
}
# Notes on the list.  The issue's "conv_mx3's scale taken per tap instead of per pixel" is replaced by the two conv_mx3 entries above: a scale per (patch pixel, tap)
# is a scale over the same 32 channels, i.e. the rule itself, so the two ways a wrong block can differ from it are taken instead — wider (the 3 x 3 window of the output
# pixel) and narrower (one 16-channel K step).  "a1 by truncation" shows only where x s falls between two f16 values whose residual cannot take the difference back:
# between f16 subnormals (the masked case, whose modulation 0.25 puts the subnormal band there; the encoder case normalised by rstd 0.5 likewise); elsewhere the
# residual f16(a - a1) restores the sum and the mutant stays below a bar, and the designed encoder / block-kernel inputs without such a factor are f16-exact, where
# truncation IS the rounding.  "region-less pixel modulated by row 0" cannot show in the output — the epilogue multiplies that pixel's sum by zero — but it shows in
# the range guard: ``regionless_guard_case`` puts +-65520 where every output pixel that reads it is region-less, and the counter must not move.
# Mutants no constructible case separates by two bars, with the reason (tests/test_mx_model_cpu.py prints the measured ratio of each):
NOT_SEPARABLE = {
    "residual from the rounded product": "fl32(x s) - a1 and fma(x, s, -a1) differ by at most half an fp32 ulp of the product, 2^-25 |a|, which moves the f16 residual only "
                                         "across a tie: one fp32 rounding per product where the bar allows D of them (measured 0.07 bars on the Gaussian case, 0 where x s is exact)",
}
# (the channel tail of a ragged cin: every launcher requires cin % 16 == 0 (conv_mx3: % 32), so no kernel run can show it; the prep kernels accept any cin and
#  tests/test_gpu_mx_arith.py compares their bytes at cin = 40 with the model's, zero positions included)


def emulate(c, kernel, lose1=None, lose2=None, swap_pairs=False, forget12=False, weight_layout=None, **mut):
    """What ``kernel`` computes for case ``c`` with exact (float64) accumulation: the three terms from the model's own operands — the weights decoded from the
    model's blocks of the kernel's prepared layout, the activations converted block by block — summed, then the kernel's epilogue.  Returns a dict: ``out`` the
    output, ``bar`` the counted bar per output (``chain_length`` x 2^-24 x the sum of the magnitudes of every term product, through the epilogue), ``guard``
    whether the range guard must trip, ``D``.  The keywords are the mutants of ``MUTANTS``."""
    assert kernel in KERNELS
    if kernel == "upblock":
        return _emulate_upblock(c, lose1, lose2, swap_pairs, forget12, **mut)
    wmut = {k: mut[k] for k in ("rounding", "overflow") if k in mut}
    if kernel in ("modconv_mx", "mx4"):
        rm = MM.region_map(c)
        layout = 4 if kernel == "mx4" else 1
        blk, idx, shape = model_weights(c["W"], layout, c["blur"] if c["up"] else None, forget12=forget12, **wmut)
        acts = _masked_acts(c, rm, **mut)
        chunk_of = CKS
    else:
        stride = 2 if kernel == "conv_mx3_s2" else 1
        layout = weight_layout or {"conv_mx": 1, "conv_mx3": 3, "conv_mx3_s2": 5}[kernel]
        blk, idx, shape = model_weights(c["W"], layout, None, 1.0, forget12=forget12, **wmut)
        if weight_layout is not None:          # the bytes of one layout read through the block map of another
            idx = block_index({"conv_mx3_s2": 5, "conv_mx3": 3}[kernel], 1, shape[1], shape[2])
        acts = _enc_acts(c, kernel, stride, **mut)
        chunk_of = CKS if kernel == "conv_mx" else CK3
    w1, q0, q1 = dense_terms(blk, idx, shape)
    cin = shape[2]
    k1 = _kmask(cin, chunk_of, lose1)[None, None, :, :, None, None].numpy() if lose1 else 1.0
    k2 = _kmask(cin, chunk_of, lose2)[None, None, :, :, None, None].numpy() if lose2 else 1.0
    f1, f2 = (acts["f2"], acts["f1"]) if swap_pairs else (acts["f1"], acts["f2"])
    raw = _sum(c, w1, acts["a1"]) + _sum(c, q1, f1 * k1) + _sum(c, q0, f2 * k2)
    mag = _sum(c, w1.abs(), np.abs(acts["a1"])) + _sum(c, q1.abs(), np.abs(f1 * k1)) + _sum(c, q0.abs(), np.abs(f2 * k2))
    D = chain_length(c, kernel)
    if kernel in ("modconv_mx", "mx4"):
        out = MM._epilogue(c, raw, rm)
        m = mag * (MM._gather(c["d"].double().abs(), rm) if c["d"] is not None else (rm >= 0)[:, None].double())
        if c["noise"] is not None:
            m = m + (c["noise_weight"].double() * c["noise"].double().reshape(c["noise"].shape[0], 1, *raw.shape[2:])).abs()
        if c["bias"] is not None:
            m = m + c["bias"].double().abs()[None, :, None, None]
        if c["act"]:
            m = m * MM.SQRT2
    else:
        out = CM._epilogue(raw, None, None, False, c["prelu"])
        m = mag * (c["prelu"].double().abs().clamp(min=1.0)[None, :, None, None] if c["prelu"] is not None else 1.0)
    return dict(out=out, bar=D * U * m, guard=bool(guard(acts["a"]).any()), D=D, raw=raw)


def emulate_rgb(c, emu):
    """The fused single-region ToRGB on the emulated activation: the image in float64 and its counted bar — the activation's bar through |w s| / sqrt(cout), plus
    the roundings of the 1x1 sum itself: cout additions, the weight's scale and modulation, the product, the bias, and the 16 taps and the sum of the skip."""
    r = c["rgb"]
    img = MM.to_rgb64(c, emu["out"])
    wabs = (r["w"].double()[None] * (1.0 / math.sqrt(c["cout"])) * r["s"].double()[:, None, :]).abs()          # [bs, 3, cout]
    mag = torch.einsum("boc,bchw->bohw", wabs, emu["out"].abs()) + r["bias"].double().abs().reshape(1, 3, 1, 1)
    if r["skip"] is not None:
        mag = mag + MM.O.upfirdn2d(r["skip"].double().abs(), r["upk"].double().abs(), up=2, down=1, pad=(2, 1))
    D = c["cout"] + 4 + (17 if r["skip"] is not None else 0)
    return dict(out=img, bar=torch.einsum("boc,bchw->bohw", wabs, emu["bar"].expand_as(emu["out"])) + D * U * mag, D=D)


def emulate_split_planes(c, emu):
    """The split-plane output on the emulated activation: act s_next in fp32 as two bf16 terms.  Bar: the activation's through |s_next|, one rounding of the
    product, and 2^-16 of the value for the two-term bf16 form."""
    sn = c["sn"].double()[:, :, None, None]
    v = emu["out"] * sn
    return dict(out=v, bar=emu["bar"].expand_as(v) * sn.abs() + (U + 2.0 ** -16) * v.abs(), D=emu["D"] + 1)


def bars_off(value, emu):
    """The largest |value - emulation| in bars (an output whose bar is 0 — no non-zero product reaches it — must be matched exactly)."""
    err = (value.detach().double().cpu() - emu["out"]).abs()
    bar = emu["bar"].expand_as(err)
    ratio = torch.where(bar > 0, err / bar.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return ratio.max().item()


def reference64(c, kernel):
    """float64 of the exact layer on the fp32 inputs the kernel gets."""
    if kernel in ("modconv_mx", "mx4", "upblock"):
        return MM.reference64(c)
    return CM.reference(c["x"], c["W"], stride=2 if kernel == "conv_mx3_s2" else 1, pad=1, in_norm=c["in_norm"], prelu=c["prelu"])


def layer_error(value, c, kernel):
    """max |value - float64| as a fraction of the layer's output scale (the measure ``MX_LAYER_TOL`` bounds)."""
    ref = reference64(c, kernel)
    return maxdiff(value, ref) / max(1.0, ref.abs().max().item()) if kernel in ("modconv_mx", "mx4", "upblock") else maxdiff(value, ref) / ref.abs().max().item()


# ------------------------------------------------------------------------------------------------ fp32 accumulation
def emulate32(c, kernel, order):
    """``emulate`` with ONE fp32 accumulator per output taking every product singly (the harshest reading of an MFMA's undocumented internal order), in three
    orders: ``ascending`` (term by term, channel by channel, tap by tap), ``loop`` (as the K loop runs: per chunk and kernel row / unit the f16 products, then the
    two fp6 terms) and ``pairwise`` (a balanced tree); then the epilogue in float64.  Same-resolution and plain cases only."""
    assert not c.get("up")
    if kernel in ("modconv_mx", "mx4"):
        rm = MM.region_map(c)
        blk, idx, shape = model_weights(c["W"], 1)
        acts = _masked_acts(c, rm)
        chunk_of, stride = CKS, 1
    else:
        stride = 2 if kernel == "conv_mx3_s2" else 1
        blk, idx, shape = model_weights(c["W"], {"conv_mx": 1, "conv_mx3": 3, "conv_mx3_s2": 5}[kernel], None, 1.0)
        acts = _enc_acts(c, kernel, stride)
        chunk_of = CKS if kernel == "conv_mx" else CK3
    w1, q0, q1 = (t[0] for t in dense_terms(blk, idx, shape))
    cin = shape[2]
    terms = [(w1, torch.from_numpy(acts["a1"][0])), (q1, torch.from_numpy(acts["f1"][0])), (q0, torch.from_numpy(acts["f2"][0]))]
    keys = []          # (term, channel, tap) in the order of addition
    if order == "loop":
        groups = [range(3 * r, 3 * r + 3) for r in range(3)] if chunk_of == CKS else [(2 * u, 2 * u + 1) if u < 4 else (8,) for u in range(5)]
        for ch in range(cin // chunk_of):
            for taps in groups:
                for t in range(3):
                    keys += [(t, ci, tap) for tap in taps for ci in range(ch * chunk_of, (ch + 1) * chunk_of)]
    else:
        keys = [(t, ci, tap) for t in range(3) for ci in range(cin) for tap in range(9)]

    def prod(k):
        t, ci, tap = k
        return (terms[t][0][:, ci, tap][None, :, None, None] * terms[t][1][:, ci, tap][:, None]).float()      # one rounding of an exact product: below the bar's count

    if order == "pairwise":
        level = [prod(k) for k in keys]
        while len(level) > 1:
            level = [(level[i] + level[i + 1]) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
        acc = level[0]
    else:
        acc = torch.zeros_like(prod(keys[0]))
        for k in keys:
            acc = acc + prod(k)
    raw = acc.double()
    if kernel in ("modconv_mx", "mx4"):
        return MM._epilogue(c, raw, rm)
    return CM._epilogue(raw, None, None, False, c["prelu"])


# ================================================================================================ the cases
def _mrow(id, bs, cin, cout, h, w, nreg, lh, lw, up=False, noise=1, act=True):
    return MM._row("mx_" + id, bs, cin, cout, h, w, nreg=nreg, lh=lh, lw=lw, up=up, noise=noise, act=act)


# masked layers at the smallest shapes the kernel accepts (width >= 32, cout >= 128, cin % 16 == 0): one chunk / three / four chunks (the last: split over K
# slices), one co tile and a tail tile, a map of exactly one tile row and a ragged one, labels at another resolution with a region-less corner, all 16 table rows
MOD_ROWS = [
    _mrow("c16_co128_32x32", 1, 16, 128, 32, 32, 3, 32, 32),
    _mrow("c48_co136_40x36", 1, 48, 136, 40, 36, 12, 13, 21, noise=2),
    _mrow("c64_co128_32x32_r16", 2, 64, 128, 32, 32, 16, 64, 64, noise=2),
    _mrow("c16_co136_40x36_noact", 1, 16, 136, 40, 36, 5, 80, 72, noise=0, act=False),
]
# composed up layer (the kernel wants an input width >= 32: 16 x 32 -> 32 x 64) and the four-parity launch (cin 32, cout 128, 32 -> 64)
# the fused single-region ToRGB (every output channel in one workgroup tile: cout = 128, same resolution), plain and with the skip image, and the split-plane output
RGB_ROWS = [MM._row("mx_rgb_plain_c16_co128_9x36", 1, 16, 128, 9, 36, nreg=3, lh=13, lw=21, rgb="plain"),
            MM._row("mx_rgb_skip_c32_co128_10x40", 2, 32, 128, 10, 40, nreg=12, lh=13, lw=21, rgb="skip", noise=2),
            MM._row("mx_sp_c16_co128_9x36", 1, 16, 128, 9, 36, nreg=3, lh=13, lw=21, rgb="plain", s_next=True)]
UP_ROWS = [_mrow("up_c16_co128_16x32", 1, 16, 128, 16, 32, 3, 13, 21, up=True)]
MX4_ROWS = [_mrow("up4_c32_co128_32x32", 1, 32, 128, 32, 32, 5, 16, 16, up=True)]
# the block kernel: every 16 x 16 output block of the 64 x 64 output under one region (cells of 16 label pixels at the output resolution), one and two chunks
UPBLOCK_ROWS = [_mrow("upblk_c32_co128_32x32", 1, 32, 128, 32, 32, 5, 64, 64, up=True), _mrow("upblk_c64_co136_32x32", 2, 64, 136, 32, 32, 12, 64, 64, up=True, noise=2)]
#            id                 bs cin cout  h   w  stride
ENC_ROWS = [("s1_c32_co128_7x45", 1, 32, 128, 7, 45, 1),
            ("s1_c96_co136_40x36", 2, 96, 136, 40, 36, 1),
            ("s2_c32_co136_14x90", 1, 32, 136, 14, 90, 2),
            ("s2_c64_co128_16x24", 2, 64, 128, 16, 24, 2)]
_CASES = {}


def mod_case(row):
    c = MM.case(row)
    if row["id"].startswith("mx_upblk") and "cells16" not in c:
        g = torch.Generator().manual_seed(row["cin"] + 16)
        cells = torch.randint(0, row["nreg"], (row["bs"], row["lh"] // 16, row["lw"] // 16), generator=g).to(torch.uint8)
        c["labels"] = cells.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
        c["cells16"] = True
    return c


def enc_case(row, norm_prelu):
    """Seeded Gaussian inputs of one encoder row: x of mean 0.5 and spread 2, weights of the layer's scale, the sample's own statistics, PReLU slopes in [0, 0.5)."""
    id, bs, cin, cout, h, w, stride = row
    key = (id, norm_prelu)
    if key not in _CASES:
        x = randn(id + "x", (bs, cin, h, w), 2.0) + 0.5
        W = randn(id + "W", (cout, cin, 3, 3)) / math.sqrt(cin * 9.0)
        _CASES[key] = dict(id=f"mx_enc_{id}_{'norm_prelu' if norm_prelu else 'plain'}", bs=bs, cin=cin, cout=cout, h=h, w=w, stride=stride, x=x, W=W,
                           in_norm=CM.host_stats(x) if norm_prelu else None, prelu=(randn(id + "p", (cout,)).abs() * 0.25).clamp(max=0.5) if norm_prelu else None)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ designed inputs
# One activation pattern per band of four map rows (a block of the masked loop — three neighbouring pixels of a row x 8 channels — then holds one pattern), per K
# half of 8 channels, in units of the block scale 2^(E - 2) with E = 0: channel 0 of a half is the "setter" that fixes the block exponent; weight classes with a
# zero on the setter make the small values the whole output.
_T = 2.0 ** -13
BANDS = [
    ("zero", [0, 0, 0, 0, 0, 0, 0, 0]),                                               # an all-zero block: exponent floor, every code 0
    ("max_pow2_ties_up", [4.0, 0.1875, 0.4375, 0.6875, 0.1875, 0.4375, 0.6875, 0.1875]),          # maximum exactly 2^E; ties that RNE rounds up (truncation differs)
    ("ties_down", [4.0, 0.0625, 0.3125, 0.5625, 0.0625, 0.3125, 0.5625, 0.0625]),                 # ties that RNE rounds down (half-away differs)
    ("saturating", [7.99609375, 7.75, 3.0, 1.5, 7.75, 6.0, 2.0, 7.875]),                         # just under 2^(E + 1): the largest elements saturate at 7.5
    ("smallest_codes", [4.0, 0.125, 0.625, 0.125, 0.625, 0.125, 0.625, 0.125]),                  # exact now, lost or moved when the scale is one too large
    ("residual", [4.0 * (1 + 461 * 2.0 ** -20)] * 8),                                            # a1 = 4, a - a1 = 0.45 f16 ulp, all of one sign
    ("small_residual", [4.0] + [0.5 * (1 + _T)] * 7),                                            # a - a1 = 2^-16 of the setter: code 0.125 under 2^(E - 13), nothing under 2^(E - 12)
    ("negative_ties", [-4.0, -0.1875, -0.4375, -0.6875, -0.0625, -0.3125, -0.5625, -0.0]),       # oddness, a negative zero
    ("f16_subnormal", [1000 * 2.0 ** -22, 700 * 2.0 ** -22, 3 * 2.0 ** -22, 2.0 ** -22, 513 * 2.0 ** -22, 0, 2.0 ** -22, 999 * 2.0 ** -22]),    # x 2^-2: f16 subnormals
    ("edge_65519", [65519.0 * 4, 4.0, 8.0, 16.0, 30000.0 * 4, 1.0, 2.0, 3.0]),                   # x 2^-2: 65519 rounds to 65504, the guard must NOT trip
]
#   weight classes by co % 8 (before the layer's scale, which the model applies as the kernel does)
W_UNIT_RES = 1 + 461 * 2.0 ** -20        # f16(w) = 1, w - w1 = 0.45 f16 ulp


def designed_x(bs, cin, h, w, chunks=None, colstep=False, group=16):
    """The banded activation map ``[bs, cin, h, w]`` (x 2^-2: the patterns are written in units of the block scale at E = 0).  ``chunks``: the 16-channel chunks
    that carry the patterns (the others are zero); ``colstep``: every third column and the second half of every ``group`` channels scaled by 2^-4 (blocks whose
    taps / K halves / K steps differ in range)."""
    x = torch.zeros(bs, cin, h, w, dtype=torch.float64)
    for y in range(h):
        pat = torch.tensor(BANDS[(y // 4) % len(BANDS)][1], dtype=torch.float64) * 0.25
        x[:, :, y, :] = pat.repeat(cin // 8)[None, :, None]
    if chunks is not None:
        keep = torch.zeros(cin, dtype=torch.float64)
        for ch in chunks:
            keep[ch * 16:(ch + 1) * 16] = 1
        x = x * keep[None, :, None, None]
    if colstep:
        col = torch.where(torch.arange(w) % 3 == 1, 2.0 ** -4, 1.0).double()
        half = torch.where((torch.arange(cin) % group) >= group // 2, 2.0 ** -4, 1.0).double()
        x = x * col[None, None, None, :] * half[None, :, None, None]
    return x.float()


def designed_w(cout, cin, colstep=False, group=16):
    """Weight classes by co % 8: 0 all ones; 1 ones, zero on the setter channels; 2 / 3 the same with a residual of 0.45 f16 ulp on every weight (w - w1 of one
    sign); 4 Gaussian; 5 class 3 x 2^-14 (w1 an f16 subnormal: the residual's f16 detour); 6 class 3 negated; 7 class 3 on the left tap column only."""
    W = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    setter = (torch.arange(cin) % 8 == 0)
    g = randn("mx_designed_w", (cout, cin, 3, 3)).double()
    for co in range(cout):
        k = co % 8
        if k in (0, 1):
            W[co] = 1.0
        elif k == 4:
            W[co] = g[co]
        else:
            W[co] = W_UNIT_RES
        if k in (1, 3, 5, 6, 7):
            W[co, setter] = 0
        if k == 5:
            W[co] *= 2.0 ** -14
        if k == 6:
            W[co] = -W[co]
        if k == 7:
            W[co, :, :, 1:] = 0
            if colstep:
                W[co, (torch.arange(cin) % group) < group // 2] = 0
    return W.float()


def designed_mod_case(id, cin, chunks=None, colstep=False, cout=128, h=40, w=32):
    """A masked same-resolution case on the designed inputs: modulation rows that are powers of two (x s exact: the patterns survive), labels i.i.d. with a
    region-less corner, the weights pre-divided by the layer's fp32 scale so that fl32(W scale) is the class value to one fp32 rounding."""
    key = ("designed", id)
    if key in _CASES:
        return _CASES[key]
    row = MM._row("mx_designed_" + id, 1, cin, cout, h, w, nreg=4, lh=h, lw=w, noise=0, act=False)
    c = dict(row)
    c["x"] = designed_x(1, cin, h, w, chunks, colstep)
    sc = float(MM.scale32(cin))
    c["W"] = (designed_w(cout, cin, colstep).double() / sc).float()
    c["s"] = torch.tensor([1.0, 0.25, 0.5, 1.0])[None, :, None].expand(1, 4, cin).contiguous()
    c["nreg"] = 4
    c["d"] = None
    g = torch.Generator().manual_seed(cin * 131 + 7)
    lab = torch.randint(0, 4, (1, h, w), generator=g).to(torch.uint8)
    lab[:, : h // 8, : w // 4] = MM.LABEL_NONE
    c["labels"] = lab
    c["noise"], c["noise_weight"], c["bias"], c["blur"], c["sn"], c["rgb"] = None, torch.tensor([0.0]), None, MM.blur_kernel(), None, None
    _CASES[key] = c
    return c


def designed_upblock_case(id="c32", cin=32, chunks=None, cout=128, h=32, w=32):
    """The designed inputs through the block kernel: an up layer whose 16 x 16 output blocks carry one region each (modulation rows that are powers of two)."""
    key = ("designed_up", id)
    if key in _CASES:
        return _CASES[key]
    c = dict(designed_mod_case("upsrc_" + id, cin, chunks, False, cout, h, w))
    c.update(id="mx_designed_upblk_" + id, up=True, route="conv", lh=2 * h, lw=2 * w)
    g = torch.Generator().manual_seed(cin + 99)
    cells = torch.randint(0, 4, (1, 2 * h // 16, 2 * w // 16), generator=g).to(torch.uint8)
    c["labels"] = cells.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    c["d"] = torch.ones(1, 4, cout)
    _CASES[key] = c
    return c


def regionless_guard_case(value):
    """+-``value`` at one pixel whose whole 3 x 3 output neighbourhood has no region (rows 0 .. 9 of the map), 0.5 elsewhere, every modulation row 1: the
    modulated activation of every output pixel that reads the large value is 0, so the range guard must stay down — and moves if row 0 stood in for 'no region'."""
    c = dict(designed_mod_case("c16", 16))
    x = torch.full_like(c["x"], 0.5)
    x[0, 5, 4, 16] = value
    lab = torch.zeros_like(c["labels"])
    lab[:, :10] = MM.LABEL_NONE
    return dict(c, id="mx_regionless_guard", x=x, labels=lab, s=torch.ones_like(c["s"]))


def designed_enc_case(id, cin, stride=1, chunks=None, cout=128, h=40, w=32, norm=False, colstep=False):
    """The same inputs through a plain convolution (weights as they are); ``norm``: statistics (mean 0, rstd a power of two) that keep the patterns exact."""
    key = ("designed_enc", id)
    if key in _CASES:
        return _CASES[key]
    x = designed_x(1, cin, h, w, chunks, colstep, 32)
    in_norm = (torch.zeros(1, cin), torch.full((1, cin), 0.5)) if norm else None
    _CASES[key] = dict(id="mx_designed_enc_" + id, bs=1, cin=cin, cout=cout, h=h, w=w, stride=stride, x=x, W=designed_w(cout, cin, colstep, 32), in_norm=in_norm, prelu=None)
    return _CASES[key]
