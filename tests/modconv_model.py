"""A plain CPU model of the split-bf16 modulated convolution (csrc/modconv_sb.hip, csrc/modconv_upfused.hip): the float64 reference of the layer on the fp32
inputs the kernel gets (``reference64``), the kernel's arithmetic with float64 accumulation (``emulate``) and with fp32 accumulation in its K order
(``emulate32``), the mutants the parity bars are held against, a mirror of the three launchers' dispatch rules (``select_kernel`` / ``all_instantiations``)
and the case tables tests/test_modconv_model_cpu.py and tests/test_gpu_modconv_variants.py share.  No GPU and no library import.

The layer:  out[b, co, p] = act( d[b, r(p), co] * sum_{ci, tap} W[co, ci, tap] * scale * (x * s[b, r(p)])[ci, q(p, tap)] + noise_weight * noise[b, p] + bias[co] )
with r(p) the region of the OUTPUT pixel (label map sampled 'nearest' at the output size, label 255 = no region = a zero sum) and, for up layers, the
stride-2 transposed convolution followed by the 4x4 blur with pad (1, 1).

Routes: ``"conv"`` = ``ops.region_modconv3x3`` (same resolution, or ``up`` on blur-composed parity weights), ``"tconv"`` = ``ops.modconv_up_single`` with
``ops.UP_FUSED = False`` (transposed conv into a pre-blur map + blur epilogue), ``"fused"`` = the one-launch up kernel, ``"fused_sp"`` = the same on split
planes (input pre-modulated and pre-split, output multiplied by the next layer's modulation and split)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from conv_model import cdiv, maxdiff, randn, split_terms      # noqa: F401  (re-exported for the two test files)
from oracle import e4s_oracle as O

CKS = 16                       # input channels per K chunk
MAX_REGIONS = 16
LABEL_NONE = 255
SQRT2 = math.sqrt(2.0)
LAYER_TOL = 2e-4               # tests/test_gpu_synthesis.py: the split-bf16 layer against the fp32 oracle, times max(1, |ref|)
RGB_TOL = 3e-5                 # ... and the fp32 ToRGB
PRODUCTS = {2: ((0, 0), (0, 1), (1, 0)), 3: ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))}      # (weight term, activation term), in the kernel's MFMA order

# every mutant: name -> (keyword of ``reference64`` / ``emulate``, kind).  ``arith`` mutants are single lost products of the emulation, held to ``fp32_class_bar``
# against the emulation; the others are held to the layer bar against the float64 reference.
MUTANTS = {
    "lo*hi dropped": (dict(drop=(1, 0)), "arith"),
    "hi*lo dropped": (dict(drop=(0, 1)), "arith"),
    "lo plane of the last channel zeroed": (dict(zero_lo_channel=-1), "arith"),
    "region of the input pixel": (dict(region="input"), "index"),
    "labels sampled with round": (dict(label_round=True), "index"),
    "label 255 counted as region 0": (dict(none_is_zero=True), "index"),
    "d of the wrong region": (dict(d_shift=1), "index"),
    "up: region of the position": (dict(region="position"), "index"),
    "up: blur not flipped": (dict(blur_flip=False), "index"),
    "up: blur pad (2, 0)": (dict(blur_pad=(2, 0)), "index"),
    "up: parities swapped": (dict(swap_parity=True), "index"),
    "noise batch stride 0": (dict(noise_stride0=True), "index"),
    "noise weight after the activation": (dict(noise_after_act=True), "index"),
    "leaky slope 0.01": (dict(slope=0.01), "index"),
    "sqrt(2) gain missing": (dict(gain=1.0), "index"),
    "last K chunk lost": (dict(lose_last_chunk=True), "index"),
    "right boundary tap clamped": (dict(clamp_right=True), "index"),
    "ToRGB skip pad (1, 2)": (dict(skip_pad=(1, 2)), "index"),
    "split planes without s_next": (dict(no_s_next=True), "index"),
}


# ------------------------------------------------------------------------------------------------ label sampling
def nearest_src(n_out, n_in, rounded=False):
    """Source index of every destination index as ``nearest_src`` of csrc/common.h computes it: floor(float(dst) * float(n_in / n_out)) in fp32, clamped."""
    scale = np.float32(n_in) / np.float32(n_out)
    t = np.arange(n_out, dtype=np.float32) * scale
    idx = (np.floor(t + np.float32(0.5)) if rounded else np.floor(t)).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, n_in - 1))


def region_map(c, label_round=False, none_is_zero=False, region="output"):
    """Region of every output pixel ``[bs, ho, wo]`` (int64, -1 = none)."""
    ho, wo = out_hw(c)
    if c["labels"] is None:
        return torch.zeros((c["bs"], ho, wo), dtype=torch.int64)
    lab = c["labels"].long()
    iy, ix = nearest_src(ho, lab.shape[1], label_round), nearest_src(wo, lab.shape[2], label_round)
    rm = lab[:, iy][:, :, ix]
    if region == "position":          # up layer: all four outputs of a position take the region of its first one
        rm = rm[:, ::2, ::2].repeat_interleave(2, 1).repeat_interleave(2, 2)
    if none_is_zero:
        rm = torch.where(rm == LABEL_NONE, torch.zeros_like(rm), rm)
    return torch.where(rm < c["nreg"], rm, torch.full_like(rm, -1))


def out_hw(c):
    return (2 * c["h"], 2 * c["w"]) if c["up"] else (c["h"], c["w"])


def _gather(table, rm, shift=0):
    """table ``[bs, nreg, C]`` at the region of every pixel -> ``[bs, C, H, W]``, zero where the pixel has no region."""
    nreg = table.shape[1]
    idx = ((rm.clamp(min=0) + shift) % nreg)
    g = torch.gather(table, 1, idx.flatten(1)[:, :, None].expand(-1, -1, table.shape[2]))            # [bs, HW, C]
    g = g * (rm >= 0).flatten(1)[:, :, None].to(table.dtype)
    return g.transpose(1, 2).reshape(table.shape[0], table.shape[2], rm.shape[1], rm.shape[2])


# ------------------------------------------------------------------------------------------------ the epilogue and the fused pieces
def _epilogue(c, raw, rm, dtype=torch.float64, d_shift=0, noise_stride0=False, noise_after_act=False, slope=0.2, gain=SQRT2):
    v = raw.to(dtype)
    if c["d"] is not None:
        v = v * _gather(c["d"].to(dtype), rm, d_shift)
    else:
        v = v * (rm >= 0)[:, None].to(dtype)
    nz = None
    if c["noise"] is not None:
        n = c["noise"].to(dtype).reshape(c["noise"].shape[0], 1, *raw.shape[2:])
        if noise_stride0:
            n = n[:1]
        nz = c["noise_weight"].to(dtype) * n
        if not noise_after_act:
            v = v + nz
    if c["bias"] is not None:
        v = v + c["bias"].to(dtype)[None, :, None, None]
    if c["act"]:
        v = torch.where(v > 0, v, v * slope) * gain
    if nz is not None and noise_after_act:
        v = v + nz
    return v


def to_rgb64(c, act, skip_pad=(2, 1)):
    """The fused single-region ToRGB on an activation ``[bs, cout, h, w]`` in float64: 1x1 modulated (no demodulation), bias, optional skip through
    ``upfirdn2d(up=2, pad=(2, 1))``."""
    r = c["rgb"]
    wmod = r["w"].double()[None] * (1.0 / math.sqrt(c["cout"])) * r["s"].double()[:, None, :]          # [bs, 3, cout]
    y = torch.einsum("boc,bchw->bohw", wmod, act.double()) + r["bias"].double().reshape(1, 3, 1, 1)
    if r["skip"] is not None:
        y = y + O.upfirdn2d(r["skip"].double(), r["upk"].double(), up=2, down=1, pad=skip_pad)
    return y


def split_planes_value(c, act, no_s_next=False, exact=False):
    """What the split-plane output holds, as hi + lo: ``act * s_next`` rounded to fp32 and split into two bf16 terms (``exact``: the float64 product)."""
    sn = c["sn"].double()[:, :, None, None]
    v = act.double() * (1.0 if no_s_next else sn)
    if exact:
        return v
    hi, lo = split_terms(v.float(), 2, torch.bfloat16)
    return (hi + lo).double()


def to_blocked(t):
    """``[bs, C, H, W]`` -> channel-blocked ``[bs, C/8, H, W, 8]``."""
    b, ch, h, w = t.shape
    return t.reshape(b, ch // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


def from_blocked(t):
    b, cb, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(b, cb * 8, h, w)


def split_product(x, s):
    """[hi, lo] of x * s where the multiplication stands inside the split (the masked kernels' activation operand, ``e4s_to_split_planes``): hi = bf16(fl32(x * s));
    the compiler contracts the residual ``x * s - hi`` into one FMA, so lo = bf16(fl32(x * s - hi)) sees the UNROUNDED product.  The two differ where the fp32
    residual is a tie of the bf16 rounding, one element in sixty — a bf16 ulp of lo each, together one to two bars of ``fp32_class_bar``.  (The single-region
    kernels select between the product and a zero before they split: no contraction, ``split_terms`` of the rounded product.)"""
    t = x.double() * s.double()                       # exact: 24 + 24 bits
    hi = t.float().bfloat16().float()
    lo = (t - hi.double()).float().bfloat16().float()
    return [hi, lo]


def split_planes_of(x, s):
    """int16 split planes ``[2, bs, C/8, H, W, 8]`` of x * s, as ``ops.to_split_planes`` makes them."""
    hi, lo = split_product(x.float(), s.float().reshape(x.shape[0], -1)[:, :, None, None])
    return torch.stack([to_blocked(hi).bfloat16().view(torch.int16), to_blocked(lo).bfloat16().view(torch.int16)])


# ------------------------------------------------------------------------------------------------ the float64 reference
def _scale64(c):
    return 1.0 / math.sqrt(c["cin"] * 9)


def reference64(c, dtype=torch.float64, region="output", label_round=False, none_is_zero=False, d_shift=0, blur_flip=True, blur_pad=(1, 1), swap_parity=False,
                lose_last_chunk=False, clamp_right=False, raw_only=False, **epi):
    """The layer with plain ``F.conv2d`` / ``F.conv_transpose2d`` + ``upfirdn2d`` per region, in ``dtype`` (float32: the stock evaluation a bar must let pass).
    The keywords are the mutants of ``MUTANTS``."""
    rm = region_map(c, label_round, none_is_zero, "position" if region == "position" else "output")
    x, s = c["x"].to(dtype), c["s"].to(dtype)
    W = c["W"].to(dtype) * _scale64(c)
    if lose_last_chunk:
        W = W.clone()
        W[:, CKS * (cdiv(c["cin"], CKS) - 1):] = 0
    ho, wo = out_hw(c)

    def conv(xs):
        if c["up"]:
            z = F.conv_transpose2d(xs, W.transpose(0, 1), stride=2)                                         # [bs, cout, 2h+1, 2w+1]
            k = c["blur"].to(dtype)
            return O.upfirdn2d(z, k if blur_flip else torch.flip(k, [0, 1]), pad=blur_pad)
        if clamp_right:
            xp = F.pad(xs, (1, 0, 1, 1))
            return F.conv2d(torch.cat([xp, xp[..., -1:]], -1), W)
        return F.conv2d(xs, W, padding=1)

    if region == "input":             # the modulation follows the INPUT pixel (same-resolution layers)
        assert not c["up"]
        raw = conv(x * _gather(s, rm))
    else:
        raw = torch.zeros((c["bs"], c["cout"], ho, wo), dtype=dtype)
        for r in range(c["nreg"]):
            sel = (rm == r)[:, None]
            if sel.any():
                raw = raw + conv(x * s[:, r, :, None, None]) * sel.to(dtype)
    if swap_parity:
        raw = _swap_parity(raw)
    return raw if raw_only else _epilogue(c, raw, rm, dtype, d_shift, **epi)


def stock32(c):
    return reference64(c, dtype=torch.float32)


def _swap_parity(raw):
    """out[2y + a, 2x + b] = raw[2y + b, 2x + a]."""
    out = torch.empty_like(raw)
    for a in (0, 1):
        for b in (0, 1):
            out[..., a::2, b::2] = raw[..., b::2, a::2]
    return out


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic
def scale32(cin):
    """``1.0f / sqrtf((float)cin * 9.f)`` of the launchers."""
    return np.float32(1.0) / np.sqrt(np.float32(cin) * np.float32(9.0))


def compose32(W, blur):
    """The blur-composed parity weights ``[4, cout, cin, 9]`` of an up layer in the fp32 order of ``prep_weights_sb_kernel`` (before the scale): a chain of FMAs."""
    W, blur = W.float(), blur.float()
    out = torch.zeros((4,) + tuple(W.shape[:2]) + (9,), dtype=torch.float32)
    for par in range(4):
        a, b = par >> 1, par & 1
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            v = torch.zeros(W.shape[:2], dtype=torch.float32)
            for ky in range(3):
                ty = ky + 2 * dy + 1 - a
                if ty < 0 or ty > 3:
                    continue
                for kx in range(3):
                    tx = kx + 2 * dx + 1 - b
                    if tx < 0 or tx > 3:
                        continue
                    v = (v.double() + blur[3 - ty, 3 - tx].double() * W[:, :, ky, kx].double()).float()          # v += blur * w compiles to one FMA
            out[par, :, :, tap] = v
    return out


def _unfold(x):
    """``[bs, cin, h, w]`` -> ``[bs, cin, 9, h, w]``: the nine zero-padded taps of every pixel."""
    h, w = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.stack([xp[:, :, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 2)


def _operands(c, nterms, rm, lose_last_chunk=False):
    """(weight terms, activation terms) of the route, each term an fp32 tensor holding bf16 values.
    conv:  weights ``[npar, cout, cin, 9]``, activations ``[npar, bs, cin, 9, h, w]`` = fl32(x[tap] * s[region of the output pixel]);
    tconv / fused: weights ``[cout, cin, 3, 3]``, activations ``[bs, cin, h, w]`` = fl32(x * s)."""
    sc = torch.tensor(scale32(c["cin"]))
    x, s = c["x"].float(), c["s"].float()
    if c["route"] == "conv":
        wf = (compose32(c["W"], c["blur"]) if c["up"] else c["W"].float().flatten(2)[None]) * sc
        xu = _unfold(x)
        sp = _gather(s, rm)                                                                # [bs, cin, ho, wo]
        sps = [sp[:, :, None, (p >> 1)::2, (p & 1)::2] for p in range(4)] if c["up"] else [sp[:, :, None]]
        if c["masked"] and nterms == 2:
            parts = [split_product(xu, q) for q in sps]
            xt = [torch.stack([p[k] for p in parts]) for k in range(2)]
        else:
            xt = split_terms(torch.stack([xu * q for q in sps]), nterms, torch.bfloat16)
    else:
        wf = c["W"].float() * sc
        if c["route"] == "fused_sp" and nterms == 2:         # the planes ``ops.to_split_planes`` hands the kernel
            xt = split_product(x, s[:, 0, :, None, None])
        else:
            xt = split_terms(x * s[:, 0, :, None, None], nterms, torch.bfloat16)
    if lose_last_chunk:
        wf = wf.clone()
        if c["route"] == "conv":
            wf[:, :, CKS * (cdiv(c["cin"], CKS) - 1):] = 0
        else:
            wf[:, CKS * (cdiv(c["cin"], CKS) - 1):] = 0
    return split_terms(wf, nterms, torch.bfloat16), xt


def _product(c, wa, xb, ch=None, tap=None):
    """One product plane in float64, before the blur of the tconv routes: the conv route gives the raw sums ``[bs, cout, ho, wo]``, the tconv routes the
    pre-blur map ``[bs, cout, 2h+1, 2w+1]``.  ``ch`` / ``tap``: one K chunk and one tap only."""
    cs = slice(None) if ch is None else slice(ch * CKS, (ch + 1) * CKS)
    if c["route"] == "conv":
        ts = slice(None) if tap is None else slice(tap, tap + 1)
        ho, wo = out_hw(c)
        out = torch.empty((c["bs"], c["cout"], ho, wo), dtype=torch.float64)
        for p in range(wa.shape[0]):
            y = torch.einsum("ock,bckhw->bohw", wa[p, :, cs, ts].double(), xb[p, :, cs, ts].double())
            if c["up"]:
                out[:, :, (p >> 1)::2, (p & 1)::2] = y
            else:
                out = y
        return out
    w = wa[:, cs].double()
    if tap is not None:
        m = torch.zeros(3, 3, dtype=torch.float64)
        m[tap // 3, tap % 3] = 1
        w = w * m
    return F.conv_transpose2d(xb[:, cs].double(), w.transpose(0, 1), stride=2)


def _blur64(c, z):
    return O.upfirdn2d(z, c["blur"].double(), pad=(1, 1))


def products(c, nterms=2, rm=None, lose_last_chunk=False):
    """{(a, b): raw sums of weight term a times activation term b, float64, ``[bs, cout, ho, wo]``} (the tconv routes: blurred, without the fp32 rounding
    of the pre-blur map, so that the planes add up linearly)."""
    rm = region_map(c) if rm is None else rm
    wt, xt = _operands(c, nterms, rm, lose_last_chunk)
    out = {}
    for a, b in PRODUCTS[nterms]:
        y = _product(c, wt[a], xt[b])
        out[(a, b)] = y if c["route"] == "conv" else _blur64(c, y)
    return out


def emulate(c, drop=None, zero_lo_channel=None, label_round=False, none_is_zero=False, region="output", d_shift=0, swap_parity=False, lose_last_chunk=False, raw_only=False, **epi):
    """What the kernel computes, with exact (float64) accumulation: the weight ``Weff * scale`` in fp32 (up layers on the conv route: blur-composed per
    parity), split RNE into bf16 hi and lo; the activation fl32(x * s) of the output pixel's region split the same way; ``hi*hi + hi*lo + lo*hi``; the tconv
    routes round the pre-blur map to fp32 (it is stored) and blur it; then the epilogue.  ``drop=(a, b)`` leaves one product out, ``zero_lo_channel=ci`` zeroes
    the second activation term of one input channel."""
    assert region in ("output", "position")
    rm = region_map(c, label_round, none_is_zero, region)
    wt, xt = _operands(c, 2, rm, lose_last_chunk)
    if zero_lo_channel is not None:
        xt[1] = xt[1].clone()
        xt[1].select(2 if c["route"] == "conv" else 1, zero_lo_channel).zero_()
    raw = None
    for a, b in PRODUCTS[2]:
        if drop is not None and (a, b) == tuple(drop):
            continue
        y = _product(c, wt[a], xt[b])
        raw = y if raw is None else raw + y
    if c["route"] != "conv":
        raw = _blur64(c, raw.float().double())
    if swap_parity:
        raw = _swap_parity(raw)
    return raw if raw_only else _epilogue(c, raw, rm, torch.float64, d_shift, **epi)


def emulate32(c):
    """``emulate`` with fp32 accumulation in the kernel's K order: per K slice of the split-K launch one fp32 accumulator that takes, chunk by chunk and tap
    by tap, the three MFMAs hi*hi, hi*lo, lo*hi (each the exact sum of its 16 channels, rounded once into the accumulator); the slices added in order by the
    finalize kernel; the tconv routes: the fp32 pre-blur map, then the 16 blur taps as a chain of fp32 FMAs."""
    rm = region_map(c)
    wt, xt = _operands(c, 2, rm)
    nchunk = cdiv(c["cin"], CKS)
    ksplit = select_kernel(**launch_of(c))[2] if c["route"] == "conv" else 1
    per = cdiv(nchunk, ksplit)
    total = None
    for ks in range(ksplit):
        acc = None
        for ch in range(ks * per, min(nchunk, (ks + 1) * per)):
            for tap in range(9):
                for a, b in PRODUCTS[2]:
                    t = _product(c, wt[a], xt[b], ch, tap)
                    acc = t.float() if acc is None else (acc.double() + t).float()
        if acc is None:
            continue          # an empty trailing slice adds an exact zero
        total = acc if total is None else (total.double() + acc.double()).float()
    if c["route"] != "conv":
        zp = F.pad(total, (1, 1, 1, 1))
        ho, wo = out_hw(c)
        kf = torch.flip(c["blur"].float(), [0, 1])
        out = torch.zeros((c["bs"], c["cout"], ho, wo), dtype=torch.float32)
        for ty in range(4):
            for tx in range(4):
                out = (out.double() + zp[:, :, ty:ty + ho, tx:tx + wo].double() * kf[ty, tx].double()).float()
        total = out
    return _epilogue(c, total.double(), rm)


def mutant_errors(c, ref, nterms=3, post=None):
    """{product: max |epilogue(all products but one) - ref|} of the ``nterms``-term split; ``post``: what follows the epilogue (the split-plane output's
    multiplication by the next layer's modulation), applied to the mutant — ``ref`` is then the reference of that output."""
    rm = region_map(c)
    pr = products(c, nterms, rm)
    full = sum(pr.values())
    post = post or (lambda v: v)
    return {k: maxdiff(post(_epilogue(c, full - v, rm)), ref) for k, v in pr.items()}


def fp32_class_bar(ref, c, post=None):
    """The bar of "kernel against its emulation" on one case, as ``conv_model.fp32_class_bar``: half the error of the least visible single-product mutant of the
    three-term bf16 split, from the float64 reference and the inputs alone.  That mutant (a product of relative size 2^-17) grows with sqrt(K) and so does the
    bar; the cin = 130 rows (K = 1170) need no further allowance: the fp32-accumulated emulation stays under 0.2 of the bar where the launch splits K and
    under 0.3 where one accumulator takes all 1170 products (tests/test_modconv_model_cpu.py; measured on the MI355X: 0.24 and 0.35)."""
    return 0.5 * min(mutant_errors(c, ref, 3, post).values())


def layer_bar(ref):
    return LAYER_TOL * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------ style_demod
STYLE_ROWS = [(1, 1, 16, 24), (2, 12, 130, 70), (3, 5, 64, 128)]          # (bs, nreg, cin, cout)
STYLE_DIM = 512
U = 2.0 ** -24


def style_case(row):
    bs, nreg, cin, cout = row
    tag = f"sd{bs}_{nreg}_{cin}_{cout}"
    return dict(styles=randn(tag + "st", (bs, nreg, STYLE_DIM)), mw=randn(tag + "mw", (cin, STYLE_DIM)), mb=randn(tag + "mb", (cin,), 0.3) + 1,
                wsq=randn(tag + "wsq", (cin, cout)).abs() * (1.0 / cin) + 1e-3, cout=cout)


def style_demod64(sc, no_scale=False, no_square=False):
    """s = the equalised linear of the style (weight / sqrt(sdim), bias), d = rsqrt(sum_ci s^2 wsq + 1e-8), in float64."""
    sdim = sc["styles"].shape[-1]
    s = sc["styles"].double() @ sc["mw"].double().T * (1.0 if no_scale else 1.0 / math.sqrt(sdim)) + sc["mb"].double()
    t = (s.abs() if no_square else s * s) @ sc["wsq"].double()
    return s, torch.rsqrt(t + 1e-8)


def style_demod_bar(sc):
    """Elementwise bars (s, d) in the manner of ``glue_model.vec_fc_bar``: roundings on the longest path of one output times 2^-24 times the sum of the
    magnitudes.  s: a lane takes sdim / 256 float4 steps of four products and four additions, six butterfly steps, the scale and the bias: D = 8 * steps + 8.
    d: each of 16 partial sums takes cin / 16 terms of two products and one addition, four steps join them, the epsilon; the error of s enters twice per
    term; rsqrtf is within 2 ulp and halves the relative error of its argument."""
    sdim, cin = sc["styles"].shape[-1], sc["mw"].shape[0]
    s, d = style_demod64(sc)
    scale = 1.0 / math.sqrt(sdim)
    bar_s = (8 * cdiv(sdim, 256) + 8) * U * ((sc["styles"].double().abs() @ sc["mw"].double().abs().T) * scale + sc["mb"].double().abs())
    t = (s * s) @ sc["wsq"].double()
    err_t = (3 * cdiv(cin, 16) + 5) * U * t + (2 * s.abs() * bar_s) @ sc["wsq"].double()
    bar_d = d * (0.5 * err_t / (t + 1e-8) + 3 * U)
    return bar_s, bar_d


# ------------------------------------------------------------------------------------------------ which kernel a launch reaches
# tile configurations (CB, PB, WC, WP, LOG_TW) of region_modconv3x3_sb_impl
T_64CO_64X4 = (2, 2, 1, 4, 6)
T_32CO_64X4 = (1, 2, 1, 4, 6)
T_128CO_64X4 = (4, 1, 1, 8, 6)      # in the source, but not selectable: its branch tests bit 1 of the constant ``tw64 = 1``
T_128CO_32X8 = (4, 1, 1, 8, 5)
T_64CO_32X8 = (2, 2, 1, 4, 5)
T_32CO_32X8 = (1, 2, 1, 4, 5)
T_128CO_16X16 = (4, 1, 1, 8, 4)
T_64CO_16X8 = (1, 2, 2, 2, 4)
T_64CO_8X8 = (1, 1, 2, 2, 3)
T_64CO_4X16 = (1, 1, 2, 2, 2)
TILES = (T_64CO_64X4, T_32CO_64X4, T_128CO_32X8, T_64CO_32X8, T_32CO_32X8, T_128CO_16X16, T_64CO_16X8, T_64CO_8X8, T_64CO_4X16)
# ... and of e4s_modconv_tconv_sb
TC_64CO = (2, 1, 1, 4, 5)
TC_32CO = (1, 2, 1, 4, 5)
TC_SMALL = (1, 1, 2, 2, 4)
SB, UF, UF_DMA, FINALIZE, BLUR_EP = "region_modconv_sb_kernel", "up_fused_sb_kernel", "up_fused_dma_kernel", "modconv_sb_finalize_kernel", "blur_epilogue_kernel"


def tile_geometry(tile):
    """(TN, TH, TW, LDS bytes) of ``SbCfg``."""
    cb, pb, wc, wp, log_tw = tile
    tn, npb, tw = wc * cb * 32, wp * pb, 1 << log_tw
    th = npb // (tw // 32) if tw > 32 else npb * (32 >> log_tw)
    patch = (th + 2) * (tw + 2)
    return tn, th, tw, CKS * patch * 4 + 2 * 9 * 2 * tn * 16 + MAX_REGIONS * CKS * 4


def select_tile(cout, w, masked, x_nhwc):
    if w >= 32:
        if w >= 64 and not masked and not x_nhwc:
            return T_64CO_64X4 if cout > 32 else T_32CO_64X4
        if masked and cout >= 128:                    # (the 64 x 4 form of this tile is compiled out: ``tw64 = 1`` keeps it for the single-region layers)
            return T_128CO_32X8
        return T_64CO_32X8 if cout > 32 else T_32CO_32X8
    if w >= 16 and masked and cout >= 128:
        return T_128CO_16X16
    if w >= 16:
        return T_64CO_16X8
    return T_64CO_8X8 if w >= 8 else T_64CO_4X16


def _sb(tile, uni=False, tconv=False, rgb=False, xn=False, osp=False):
    """Template arguments <CB, PB, WC, WP, LOG_TW, MINW, UNI, TCONV, RGB, XN, OSP>; MINW is 2 in every selectable instantiation."""
    return (SB, tile + (2, int(uni), int(tconv), int(rgb), int(xn), int(osp)))


def select_kernel(bs, cin, cout, h, w, masked, up, rgb, x_nhwc, out_nhwc, s_next, workspace, via="conv"):
    """(kernel base name, template arguments, ksplit) of the main kernel a launch reaches.  ``via``: ``"conv"`` = e4s_region_modconv3x3_sb, ``"tconv"`` =
    e4s_modconv_tconv_sb, ``"fused"`` = e4s_modconv_up_fused_sb (``s_next``: the split-plane form; ``masked`` then says whether d is given).
    ``workspace``: floats of split-K workspace the caller offers (0: none)."""
    if via == "tconv":
        if w + 1 > 16:
            return _sb(TC_64CO if cout > 32 else TC_32CO, True, True) + (1,)
        return _sb(TC_SMALL, True, True) + (1,)
    if via == "fused":
        if s_next:
            if cout % 32 == 0 and cin % 16 == 0 and masked:
                return (UF_DMA, (), 1)
            return (UF, (1, 4, 0, 1, 1, 1), 1)
        return (UF, (1, 4, int(x_nhwc), int(out_nhwc), 0, 0), 1)
    if rgb:
        assert w >= 32 and not up
    if out_nhwc:
        workspace = 0
    tile = select_tile(cout, w, masked, x_nhwc)
    tn, th, tw, lds = tile_geometry(tile)
    npar = 4 if up else 1
    base = cdiv(w, tw) * cdiv(h, th) * npar * cdiv(cout, tn) * bs
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    out_floats, nchunk = bs * cout * ho * wo, cdiv(cin, CKS)
    ksplit = 1
    if workspace and base < 384:
        target = 256 if lds > 64 * 1024 else 1024
        while ksplit < 16 and base * ksplit * 2 <= target and ksplit * 2 <= nchunk and ksplit * 2 * out_floats <= workspace:
            ksplit *= 2
    if rgb:
        assert tile[2] == 1 and cout <= tn
        if s_next:
            assert masked and not x_nhwc
            return _sb(tile, rgb=True, osp=True) + (1,)
        if x_nhwc:
            assert not masked
            return _sb(tile, uni=True, rgb=True, xn=True) + (1,)
        return _sb(tile, uni=not masked, rgb=True) + (1,)
    if lds > 64 * 1024:
        assert not x_nhwc
        return _sb(tile) + (ksplit,)
    if x_nhwc:
        assert not masked
        return _sb(tile, uni=True, xn=True) + (ksplit,)
    return _sb(tile, uni=not masked) + (ksplit,)


def launched(**ln):
    """Every kernel of one launch as (name, template arguments): the main kernel, the split-K finalize, the blur epilogue of the two-launch up layer."""
    name, args, ksplit = select_kernel(**ln)
    out = [(name, args)]
    if ksplit > 1:
        out.append((FINALIZE, ()))
    if ln.get("via") == "tconv":
        out.append((BLUR_EP, ()))
    return out


def all_instantiations():
    """Every kernel instantiation the three launchers can select, written out from their source rather than derived from ``select_kernel``."""
    out = set()
    big = (T_128CO_32X8, T_128CO_16X16)                                    # > 64 KB of LDS: masked only, one instantiation each
    for t in big:
        out.add(_sb(t))
    for t in (T_64CO_64X4, T_32CO_64X4, T_64CO_32X8, T_32CO_32X8, T_64CO_16X8, T_64CO_8X8, T_64CO_4X16):
        out.add(_sb(t, uni=True))
    for t in (T_64CO_32X8, T_32CO_32X8, T_64CO_16X8, T_64CO_8X8, T_64CO_4X16):   # the 64-wide tiles are single-region only
        out.add(_sb(t))
    for t in (T_64CO_32X8, T_32CO_32X8):                                   # channel-blocked input: w >= 32, and never the 64-wide tiles
        out.add(_sb(t, uni=True, xn=True))
        out.add(_sb(t, uni=True, rgb=True, xn=True))
    for t in (T_64CO_64X4, T_32CO_64X4, T_64CO_32X8, T_32CO_32X8):         # fused ToRGB: w >= 32, WC == 1, cout <= TN
        out.add(_sb(t, uni=True, rgb=True))
    for t in (T_128CO_32X8, T_64CO_32X8, T_32CO_32X8):
        out.add(_sb(t, rgb=True))
        out.add(_sb(t, rgb=True, osp=True))
    out.add((FINALIZE, ()))
    for t in (TC_64CO, TC_32CO, TC_SMALL):
        out.add(_sb(t, True, True))
    out.add((BLUR_EP, ()))
    for xn, on in ((0, 0), (1, 0), (0, 1), (1, 1)):
        out.add((UF, (1, 4, xn, on, 0, 0)))
    out.add((UF, (1, 4, 0, 1, 1, 1)))
    out.add((UF_DMA, ()))
    return out


def kernel_label(name, args):
    return f"{name}<{', '.join(str(a) for a in args)}>" if args else name


# ------------------------------------------------------------------------------------------------ the cases both test files share
SPLITK_MAX_OUT_FLOATS = 1 << 21          # ops.region_modconv3x3 offers 16 x the output as workspace up to this output size


def _row(id, bs, cin, cout, h, w, nreg=0, lh=0, lw=0, up=False, route="conv", noise=1, act=True, rgb=None, want_out=True, x_nhwc=False, out_nhwc=False,
         s_next=False, d=True):
    """``nreg`` 0: a single-region layer; ``noise``: 0 none, 1 one map, 2 one per sample; ``rgb``: None, "plain" or "skip"."""
    return dict(id=id, bs=bs, cin=cin, cout=cout, h=h, w=w, nreg=nreg, masked=nreg > 0, lh=lh, lw=lw, up=up or route != "conv", route=route, noise=noise, act=act, rgb=rgb,
                want_out=want_out, x_nhwc=x_nhwc, out_nhwc=out_nhwc, s_next=s_next, d=d)


# A. arithmetic: K = 144, 12 x 12
ARITH_CASES = [
    _row("same_single", 1, 16, 32, 12, 12),
    _row("same_masked", 1, 16, 32, 12, 12, nreg=3, lh=12, lw=12),
    _row("up_single_fused", 1, 16, 32, 12, 12, route="fused"),
    _row("up_single_tconv", 1, 16, 32, 12, 12, route="tconv"),
    _row("up_masked", 1, 16, 32, 12, 12, nreg=3, lh=24, lw=24, up=True),
]

# B. indexing: every tile configuration, single-region and masked, same resolution and up; w on both sides of 8 / 16 / 32 / 64, h odd and no multiple of the
# tile height, a channel tail on every tile, cin 16 (one chunk) / 20 (a ragged second chunk) / 130 (nine chunks: split-K with short and empty trailing slices),
# label maps at another resolution with a corner of label 255.
INDEX_ROWS = [
    # 4 x 16 tile (w < 8)
    _row("w7_single", 2, 16, 24, 5, 7, noise=2),
    _row("w7_single_up", 1, 20, 33, 3, 7, up=True),
    _row("w7_masked_k130", 3, 130, 70, 5, 7, nreg=3, lh=7, lw=9, noise=2),
    _row("w5_masked_up", 1, 20, 24, 3, 5, nreg=12, lh=13, lw=21, up=True),
    # 8 x 8 tile
    _row("w8_single", 1, 16, 65, 9, 8),
    _row("w15_masked", 2, 20, 33, 7, 15, nreg=12, lh=13, lw=21),
    _row("w15_single_k130", 1, 130, 24, 9, 15, act=False),
    _row("w9_masked_up", 1, 16, 24, 5, 9, nreg=3, lh=7, lw=11, up=True, noise=0),
    # 16 x 8 tile
    _row("w16_single", 2, 16, 70, 9, 16),
    _row("w31_masked", 1, 20, 65, 11, 31, nreg=3, lh=13, lw=21),
    _row("w17_single_up", 1, 16, 33, 5, 17, up=True),
    _row("w19_single_c136", 1, 16, 136, 9, 19),
    _row("w17_masked_k130", 2, 130, 70, 9, 17, nreg=12, lh=13, lw=21),
    # masked 128-channel tile of the 16-wide maps
    _row("w16_masked_c128", 2, 16, 128, 9, 16, nreg=12, lh=13, lw=21, noise=2),
    _row("w31_masked_c136_k130", 1, 130, 136, 17, 31, nreg=3, lh=9, lw=19),
    _row("w17_masked_c128_up", 1, 16, 128, 9, 17, nreg=3, lh=13, lw=21, up=True),
    # 32 x 8 tiles: 32 and 64 output channels
    _row("w32_single_c24", 1, 16, 24, 9, 32),
    _row("w63_masked_c24", 2, 20, 24, 9, 63, nreg=12, lh=13, lw=21),
    _row("w67_masked_c32", 1, 16, 32, 5, 67, nreg=3, lh=9, lw=19),
    _row("w33_single_c24_up", 1, 16, 24, 5, 33, up=True),
    _row("w33_single_c33", 2, 16, 33, 9, 33, noise=2),
    _row("w63_masked_c70", 1, 20, 70, 9, 63, nreg=3, lh=13, lw=21),
    _row("w64_masked_c65", 1, 16, 65, 5, 64, nreg=12, lh=13, lw=21),
    _row("w40_single_c136", 1, 16, 136, 9, 40),
    _row("w33_single_c65_k130", 1, 130, 65, 9, 33),
    _row("w33_masked_c65_up", 1, 16, 65, 5, 33, nreg=3, lh=13, lw=21, up=True),
    # masked 128-channel tile, 32 wide
    _row("w32_masked_c128", 1, 16, 128, 9, 32, nreg=12, lh=13, lw=21),
    _row("w63_masked_c136", 2, 20, 136, 9, 63, nreg=3, lh=13, lw=21, noise=2),
    _row("w33_masked_c128_k130", 1, 130, 128, 9, 33, nreg=3, lh=13, lw=21),
    _row("w33_masked_c128_up", 1, 16, 128, 5, 33, nreg=12, lh=13, lw=21, up=True),
    # masked 128-channel tile, 64 wide
    _row("w64_masked_c128", 1, 16, 128, 5, 64, nreg=3, lh=13, lw=21),
    _row("w67_masked_c136", 1, 20, 136, 5, 67, nreg=12, lh=13, lw=21),
    _row("w65_masked_c128_up", 1, 16, 128, 3, 65, nreg=3, lh=7, lw=33, up=True),
    # 64 x 4 tiles (single-region only)
    _row("w64_single_c24", 1, 16, 24, 5, 64),
    _row("w67_single_c32", 2, 20, 32, 5, 67, act=False),
    _row("w65_single_c24_up", 1, 16, 24, 3, 65, up=True),
    _row("w64_single_c33", 1, 16, 33, 5, 64),
    _row("w67_single_c70", 2, 20, 70, 5, 67, noise=2),
    _row("w67_single_c136", 1, 16, 136, 5, 67, noise=0),
    _row("w65_single_c65_up", 1, 20, 65, 3, 65, up=True),
]

# C. the non-plain instantiations at their smallest shapes
VARIANT_ROWS = [
    # fused ToRGB (w >= 32, every output channel in one workgroup tile); skips need even sizes
    _row("rgb_w64_single_c40", 1, 16, 40, 6, 64, rgb="skip"),
    _row("rgb_w67_single_c24", 2, 20, 24, 5, 67, rgb="plain", want_out=False),
    _row("rgb_w36_single_c40", 2, 20, 40, 9, 36, rgb="plain", noise=2),
    _row("rgb_w36_single_c24", 1, 16, 24, 10, 36, rgb="skip", want_out=False),
    _row("rgb_w36_blockedin_c40", 1, 16, 40, 9, 36, rgb="plain", x_nhwc=True),
    _row("rgb_w40_blockedin_c24", 1, 32, 24, 10, 40, rgb="skip", x_nhwc=True, out_nhwc=True),
    _row("rgb_w36_masked_c40", 1, 20, 40, 9, 36, nreg=3, lh=13, lw=21, rgb="plain"),
    _row("rgb_w40_masked_c24", 2, 16, 24, 10, 40, nreg=12, lh=13, lw=21, rgb="skip"),
    _row("rgb_w36_masked_c128", 1, 16, 128, 9, 36, nreg=3, lh=13, lw=21, rgb="plain", want_out=False),
    _row("rgb_w64_masked_c128", 1, 16, 128, 6, 64, nreg=12, lh=13, lw=21, rgb="skip"),
    # masked layer handing over as split planes
    _row("sp_w36_masked_c40", 1, 20, 40, 9, 36, nreg=3, lh=13, lw=21, rgb="plain", s_next=True),
    _row("sp_w40_masked_c24", 1, 16, 24, 10, 40, nreg=12, lh=13, lw=21, rgb="skip", s_next=True),
    _row("sp_w36_masked_c128", 2, 16, 128, 9, 36, nreg=3, lh=13, lw=21, rgb="plain", s_next=True),
    _row("sp_w64_masked_c128", 1, 16, 128, 6, 64, nreg=12, lh=13, lw=21, rgb="skip", s_next=True),
    # channel-blocked activations
    _row("blockedin_w36_c40", 2, 16, 40, 9, 36, x_nhwc=True),
    _row("blockedout_w67_c40", 1, 16, 40, 5, 67, out_nhwc=True),
    _row("blockedboth_w36_c24", 1, 32, 24, 9, 36, x_nhwc=True, out_nhwc=True, noise=0),
    # the transposed-conv + blur-epilogue pair: three tiles, both store paths of the epilogue (wo % 4), 2w across 128, more than 16 output rows
    _row("tconv_w15", 2, 20, 33, 5, 15, route="tconv", noise=2),
    _row("tconv_w8", 1, 16, 24, 7, 8, route="tconv", act=False),
    _row("tconv_w17_c24", 1, 20, 24, 5, 17, route="tconv"),
    _row("tconv_w66_c32", 1, 16, 32, 9, 66, route="tconv", noise=2),
    _row("tconv_w16_c70", 2, 16, 70, 5, 16, route="tconv", noise=0),
    _row("tconv_w67_c65_k130", 1, 130, 65, 3, 67, route="tconv", d=False),
    # the one-launch up kernel: 2h and 2w across its 28-pixel tile step, four layouts, split planes on the DMA kernel and on its fallback
    _row("fused_15x17", 2, 20, 40, 15, 17, route="fused", noise=2),
    _row("fused_15x17_c33_k130", 1, 130, 33, 15, 17, route="fused", act=False),
    _row("fused_blockedin", 1, 16, 40, 15, 17, route="fused", x_nhwc=True),
    _row("fused_blockedout", 2, 16, 40, 15, 17, route="fused", out_nhwc=True, noise=0),
    _row("fused_blockedboth", 1, 32, 24, 15, 17, route="fused", x_nhwc=True, out_nhwc=True, d=False),
    _row("fused_sp_c40", 2, 16, 40, 15, 17, route="fused_sp", s_next=True, noise=2),
    _row("fused_sp_c64", 1, 32, 64, 15, 17, route="fused_sp", s_next=True),
]
ALL_ROWS = ARITH_CASES + INDEX_ROWS + VARIANT_ROWS
ROW = {r["id"]: r for r in ALL_ROWS}
PROPERTY_ROWS = ("w7_masked_k130", "w16_masked_c128", "fused_15x17")     # D: small tile with split-K, masked 128-channel tile, one-launch up


def blur_kernel():
    """A 4x4 blur that is NOT symmetric (a flipped or transposed blur must show), of the stock kernel's size: sum 4."""
    ky, kx = torch.tensor([1.0, 3.2, 2.8, 1.1]), torch.tensor([0.9, 3.0, 3.1, 1.0])
    k = ky[:, None] * kx[None, :]
    return (k / k.sum() * 4).float()


_CASES = {}


def case(row):
    """The seeded inputs of one row (built once): weights ~ N(0, 1), s of mean 1 and spread 0.3, d the true demodulation of those, labels i.i.d. with a
    corner of label 255, a noise map per sample or one for all."""
    row = ROW[row] if isinstance(row, str) else row
    if row["id"] in _CASES:
        return _CASES[row["id"]]
    c = dict(row)
    t = row["id"]
    bs, cin, cout, h, w, nreg = (row[k] for k in ("bs", "cin", "cout", "h", "w", "nreg"))
    nr = max(nreg, 1)
    ho, wo = out_hw(row)
    c["x"] = randn(t + "x", (bs, cin, h, w))
    c["W"] = randn(t + "W", (cout, cin, 3, 3))
    c["s"] = randn(t + "s", (bs, nr, cin), 0.3) + 1
    c["nreg"] = nr
    wsq = (c["W"].double() * _scale64(row)).pow(2).sum((2, 3))                                   # [cout, cin]
    c["d"] = torch.rsqrt(c["s"].double().pow(2) @ wsq.T + 1e-8).float() if row["d"] else None     # [bs, nreg, cout]
    c["labels"] = None
    if row["masked"]:
        g = torch.Generator().manual_seed(len(t) * 7919 + cin * 31 + w)
        lab = torch.randint(0, nreg, (bs, row["lh"], row["lw"]), generator=g).to(torch.uint8)
        lab[:, : max(1, row["lh"] // 4), : max(1, row["lw"] // 4)] = LABEL_NONE
        c["labels"] = lab
    c["noise"] = randn(t + "n", ((bs if row["noise"] == 2 else 1), 1, ho, wo)) if row["noise"] else None
    c["noise_weight"] = torch.tensor([0.21])
    c["bias"] = randn(t + "b", (cout,), 0.1)
    c["blur"] = blur_kernel()
    c["sn"] = (randn(t + "sn", (bs, cout), 0.3) + 1) if row["s_next"] else None
    c["rgb"] = None
    if row["rgb"]:
        c["rgb"] = dict(w=randn(t + "rw", (3, cout)), s=randn(t + "rs", (bs, cout), 0.3) + 1, bias=randn(t + "rb", (3,), 0.1),
                        skip=randn(t + "rk", (bs, 3, ho // 2, wo // 2)) if row["rgb"] == "skip" else None, upk=blur_kernel())
    _CASES[row["id"]] = c
    return c


def launch_of(row):
    """The arguments of ``select_kernel`` for one row, with the workspace ``ops.region_modconv3x3`` offers."""
    ho, wo = out_hw(row)
    out_floats = row["bs"] * row["cout"] * ho * wo
    ws = 16 * out_floats if (out_floats <= SPLITK_MAX_OUT_FLOATS and not row["s_next"]) else 0
    via = {"conv": "conv", "tconv": "tconv", "fused": "fused", "fused_sp": "fused"}[row["route"]]
    masked = row["masked"] if via == "conv" else bool(row["d"])
    return dict(bs=row["bs"], cin=row["cin"], cout=row["cout"], h=row["h"], w=row["w"], masked=masked, up=row["up"] and via == "conv", rgb=bool(row["rgb"]),
                x_nhwc=row["x_nhwc"], out_nhwc=row["out_nhwc"], s_next=bool(row["s_next"]), workspace=ws, via=via)


def table_launches():
    """The launch of every row of the three tables."""
    return [launch_of(r) for r in ALL_ROWS]


def table_kernels():
    return {k for ln in table_launches() for k in launched(**ln)}
