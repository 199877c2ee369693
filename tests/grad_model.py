"""A plain CPU model of the gradient kernels of the synthesis path (csrc/modconv_bwd.hip, csrc/gemm_sb.hip, csrc/mconv_dgrad.hip, the forward and backward of
csrc/linear.hip), in the form of tests/loss_model.py: for every operation the definition in float64 (``reference64``; gradients by float64 autograd of the
float64 forward, which is the reference project's ``ModulatedConv2d`` / ``EqualLinear`` / ``LocalMLP`` in the one-pass form the kernels' headers state), a bound
computed from the reference's own magnitudes and the roundings on the kernel's longest path (``bar``), single-change mutants (``MUTANTS``), the same definition in
stock float32 (``stock32``), for the split-bf16 operations the operand split with the products summed in float64 (``emulate``) and in float32 in the kernel's
chunk, MFMA and split-K order (``emulate32``), and the case tables (``CASES``).  No GPU and no library.

An operation's inputs are a dict of numpy arrays, lists and scalars; every function returns a dict of output arrays.  Conventions of the bars (U = 2^-24):
  selections, copies and single float32 expressions   bar 0: the reference holds the float32 expression itself, bit for bit;
  fp32 sums     D U sum|terms| element-wise, D = roundings on the longest path of that kernel at that shape, stored in the case table beside the shape and
                checked against ``depth`` (the count read from the code);
  split-bf16    element-wise (3 x 2^-16 + D U) sum|a||b| against float64 (|a - hi - lo| <= 2^-16 |a| for either operand, the lo x lo product left out);
                against the emulation ``class_bar``: half the error of the least visible single-product mutant; outside both, the project's 3e-5 of max|ref|.
Kernels that take forward values (``s``, ``d``, ``wsq`` of the style tables) get the model's, rounded to float32.  No bar is a flat fraction of max|ref|."""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from conv_model import split_terms
from e4s2024_amd import seeded
from loss_model import POISON, T, N, U, arr, cdiv, ints, ratio  # noqa: F401  (shared conventions: seeded inputs, the ratio of an error to its bar)

f32, f64 = np.float32, np.float64
D64, D32 = torch.float64, torch.float32
MAX_REGIONS = 16
NT = 256
SQ2 = f32(1.41421356237309515)
OUTER = 3e-5                       # the project's bar of the split-bf16 kernels against float64, times max|ref| (tests/test_gpu_backward.py)
SPLIT = 3.0 * 2.0 ** -16           # a = hi + lo + e, |e| <= 2^-16 |a| (two RNE roundings to 8 significant bits); the lo x lo product: 2^-16 |a||b|
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def labels(key, bs, H, W, nreg, stray=True):
    """uint8 labels in [0, nreg); ``stray``: a few 255 and (nreg < 16) a few values in [nreg, 16), which belong to no region."""
    u = (arr(key, (bs, H, W)) * 0.2887 + 0.5).clip(0, 0.999)
    lab = np.floor(u * nreg).astype(np.uint8)
    if stray:
        m = arr(key + "m", (bs, H, W))
        lab[m > 1.3] = 255
        if nreg < MAX_REGIONS:
            lab[m < -1.6] = nreg
            lab[(m < -1.3) & (m >= -1.6)] = 15
    return lab


def region_index(lab, nreg, up, g, bs, h, w, swap=False):
    """[bs, h*w] region of group g's output pixel (2 qy + ga, 2 qx + gb); ``nreg`` stands for "no region"."""
    if lab is None:
        return np.zeros((bs, h * w), np.int64)
    ga, gb = divmod(g, up)
    if swap:
        ga, gb = gb, ga
    c = lab[:, ga::up, gb::up].reshape(bs, h * w).astype(np.int64)
    return np.where(c < nreg, c, nreg)


# ------------------------------------------------------------------------------------------------ roundings read from the code
def depth(kind, **k):
    """Float32 roundings on the longest path of a kernel's sum.
    ``scale``   mconv_scale_kernel: a thread's chain over every 256th pixel of its chunk, ``wave_sum`` (6), the four waves added to 0 (4).
    ``fold_dx`` mconv_fold_kernel / mconv_fold4_kernel: ``gsum`` takes up^2 x ks^2 products, each rounded and added.
    ``fold_ds`` the same kernels: ``t`` over the ks^2 taps, ``acc[r]`` over the up^2 groups of every 256th pixel (fold4: four pixels of every 1024), wave (6), waves (4).
    ``tables``  tables_bwd_s_kernel: t (5: three products, d and wsq rounded on entry), the chain over cout, ``gs + 2 s acc`` (5); tables_bwd_mod_kernel: a wave's
                quarter of the ``n`` terms, three additions, ``ms *`` (cdiv(n, 4) + 5).
    ``tables_w`` tables_bwd_w_kernel: the chain over the rows, t's 5, ``sv * sv``, ``2 c weight gwsq``, the addition, ``c *`` (rows + 12).
    ``mfma``    gemm_sb / wgrad / dgrad: three MFMAs per 16 k into one accumulator, the slices added by the finalize kernel.
    ``linear``  grouped_linear_kernel: a lane's chain (vector route: four products and their sum per 256 inputs; scalar: one per 64), the wave (6), ``* scale``.
    ``lin_dw``  grouped_linear_wgrad_kernel: the chain over the batch, ``* scale``.   ``lin_dx``  dgrad: a slice's chain, the slices added, ``* scale``, the slope.
    ``small``   small_map kernels: the chain over K (or J, transposed)."""
    if kind == "scale":
        return cdiv(min(k["chunk_px"], k["px"]), NT) + 6 + 4
    if kind == "fold_dx":
        return k["up"] ** 2 * k["ks"] ** 2
    if kind == "fold_ds":
        return k["ks"] ** 2 + k["up"] ** 2 * cdiv(min(k["chunk_px"], k["px"]), NT) + 6 + 4
    if kind == "tables":
        return (k["cout"] + 10 if k["gd"] else 0) + cdiv(k["n"], 4) + 5
    if kind == "tables_w":
        return k["rows"] + 12
    if kind == "mfma":
        return 3 * cdiv(k["K"], 16) + k.get("ksplit", 1)
    if kind == "linear":
        return (4 * cdiv(k["n"], 256) if k["vec"] else cdiv(k["n"], 64)) + 6 + 1
    if kind == "lin_dw":
        return k["bs"] + 1
    if kind == "lin_dx":
        return cdiv(k["out"], k["osplit"]) + k["osplit"] + 2
    if kind == "small":
        return k["n"]
    raise KeyError(kind)


def wave_tree32(t):
    """The float32 sum over the last axis in the order of ``scale`` / ``fold_ds``: thread i adds terms i, i + 256, ... to 0, ``wave_sum``'s butterfly
    (l ^ 32, 16, 8, 4, 2, 1: both partners form the same sum), then the four wave sums are added to 0 in order."""
    n = t.shape[-1]
    R = cdiv(n, NT)
    p = np.zeros(t.shape[:-1] + (R * NT,), f32)
    p[..., :n] = t
    p = p.reshape(t.shape[:-1] + (R, NT))
    acc = np.zeros(t.shape[:-1] + (NT,), f32)
    for r in range(R):
        acc = acc + p[..., r, :]
    acc = acc.reshape(t.shape[:-1] + (4, 64))
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc.reshape(acc.shape[:-1] + (2, o)).sum(-2, dtype=f32)
    v = np.zeros(t.shape[:-1], f32)
    for wv in range(4):
        v = v + acc[..., wv, 0]
    return v


# ================================================================================================ mconv_unfold / unfold2d
def _taps_np(x, ks, stride, pad, ho, wo, shift=0):
    """[bs, C, ks*ks, ho*wo] = x[stride q + k - pad] (0 outside); ``shift``: the pad taken one larger."""
    bs, C, hi, wi = x.shape
    qy, qx = np.arange(ho)[:, None], np.arange(wo)[None, :]
    out = np.zeros((bs, C, ks * ks, ho, wo), x.dtype)
    for ky in range(ks):
        for kx in range(ks):
            yy, xx = stride * qy + ky - pad - shift, stride * qx + kx - pad - shift
            ok = (yy >= 0) & (yy < hi) & (xx >= 0) & (xx < wi)
            out[:, :, ky * ks + kx] = np.where(ok, x[:, :, yy.clip(0, hi - 1), xx.clip(0, wi - 1)], 0)
    return out.reshape(bs, C, ks * ks, ho * wo)


def _unfold_t(x, s, lab, ks, up, nreg, swap=False):
    """The forward the fold differentiates, in torch: cols[g, b, (i, k), q] = s[b, c_g(q), i] x[b, i, q + k - pad]."""
    bs, cin, h, w = x.shape
    xs = F.unfold(x, ks, padding=ks // 2).view(bs, cin, ks * ks, h * w)
    s_ext = torch.cat([s, torch.zeros((bs, 1, cin), dtype=s.dtype)], 1)
    cols = []
    for g in range(up * up):
        idx = torch.from_numpy(region_index(lab, nreg, up, g, bs, h, w, swap))
        sv = torch.gather(s_ext, 1, idx[:, :, None].expand(bs, h * w, cin)).transpose(1, 2)
        cols.append(sv[:, :, None, :] * xs)
    return torch.stack(cols).reshape(up * up, bs, cin * ks * ks, h * w)


def unfold_ref(x, s, lab, ks, up, nreg, dt=f64, mutant=None):
    """``e4s_mconv_unfold``: one float32 product per element; the reference holds that product (exact in float64, rounded once)."""
    bs, cin, h, w = x.shape
    xs = _taps_np(x.astype(dt), ks, 1, ks // 2, h, w, shift=1 if mutant == "pad_off_by_one" else 0)
    s_ext = np.concatenate([s.astype(dt), np.zeros((bs, 1, cin), dt)], 1)
    cols = np.zeros((up * up, bs, cin, ks * ks, h * w), dt)
    for g in range(up * up):
        idx = region_index(lab, nreg, up, g, bs, h, w, swap=mutant == "parity_swapped")
        if mutant == "label_of_the_input_resolution" and lab is not None:
            idx = region_index(lab[:, ::up, ::up], nreg, 1, 0, bs, h, w)
        sv = np.take_along_axis(s_ext, idx[:, :, None], 1).transpose(0, 2, 1)                 # [bs, cin, P]
        cols[g] = sv[:, :, None, :] * xs
    return {"cols": cols.reshape(up * up, bs, cin * ks * ks, h * w).astype(f32).astype(f64)}


def _unfold_cases():
    rows = [(2, 3, 5, 7, 3, 1, 5, "stray"), (2, 3, 5, 7, 1, 2, 5, "stray"), (1, 2, 17, 19, 3, 2, 5, "stray"), (1, 2, 17, 19, 3, 1, 1, "nolab"),
            (1, 2, 17, 19, 1, 1, 16, "stray"), (2, 3, 5, 7, 3, 2, 16, "stray")]
    return [dict(name=f"b{b}.c{c}.{h}x{w}.k{k}.up{u}.r{r}.{m}", bs=b, cin=c, h=h, w=w, ks=k, up=u, nreg=r, lab=m) for b, c, h, w, k, u, r, m in rows]


def _unfold_inputs(c):
    n = c["name"]
    lab = None if c["lab"] == "nolab" else labels("ufl" + n, c["bs"], c["up"] * c["h"], c["up"] * c["w"], c["nreg"])
    return dict(x=arr("ufx" + n, (c["bs"], c["cin"], c["h"], c["w"])), s=arr("ufs" + n, (c["bs"], c["nreg"], c["cin"]), 1.0, 0.5), lab=lab, ks=c["ks"],
                up=c["up"], nreg=c["nreg"])


def unfold2d_ref(x, ks, stride, pad, ho, wo, dt=f64, mutant=None):
    """``e4s_unfold2d``: cols[b, c*KK + k, q] = x[b, c, stride q + k - pad] (0 outside): a copy."""
    st = 1 if mutant == "stride_ignored" else stride
    t = _taps_np(x.astype(dt), ks, st, pad, ho, wo, shift=1 if mutant == "pad_off_by_one" else 0)
    return {"cols": t.reshape(x.shape[0], x.shape[1] * ks * ks, ho * wo).astype(f64)}


def _unfold2d_cases():
    # stride 1 / pad ks // 2: the plain weight gradient; stride 2 / pad 0 with hi = 2 ho + 1: the transposed convolution's (_SingleStyledConvGrad)
    rows = [(2, 3, 5, 7, 5, 7, 3, 1, 1), (1, 2, 17, 19, 17, 19, 3, 1, 1), (2, 3, 11, 15, 5, 7, 3, 2, 0), (1, 2, 35, 39, 17, 19, 3, 2, 0), (2, 3, 5, 7, 5, 7, 1, 1, 0),
            (1, 2, 11, 15, 5, 7, 1, 2, 0)]
    return [dict(name=f"b{b}.c{c}.in{hi}x{wi}.out{ho}x{wo}.k{k}.s{s}p{p}", bs=b, C=c, hi=hi, wi=wi, ho=ho, wo=wo, ks=k, stride=s, pad=p) for b, c, hi, wi, ho, wo, k, s, p in rows]


def _unfold2d_inputs(c):
    return dict(x=arr("u2x" + c["name"], (c["bs"], c["C"], c["hi"], c["wi"])), ks=c["ks"], stride=c["stride"], pad=c["pad"], ho=c["ho"], wo=c["wo"])


def zero_bar(*names):
    return lambda **inp: {n: 0.0 for n in names}


# ================================================================================================ mconv_scale
def _scale_terms(gy, out, d, lab, noise, nw, bias, act, nreg, up, dt, mutant=None):
    bs, cout, H, W = gy.shape
    P2 = H * W
    g = gy.reshape(bs, cout, P2).astype(dt)
    o = np.zeros((bs, cout, P2), dt) if out is None else out.reshape(bs, cout, P2).astype(dt)
    slope = None
    if act:
        pos = (o >= 0) if mutant == "slope_ge" else (o > 0)
        slope32 = np.where(pos, SQ2, f32(f32(0.2) * SQ2)).astype(f32)
        slope = slope32.astype(dt)
    c = np.zeros((bs, P2), np.int64) if lab is None else lab.reshape(bs, P2).astype(np.int64)
    inreg = c < nreg
    idx = np.where(inreg, c, nreg)
    nz = np.zeros((bs, 1, P2), dt)
    if noise is not None:
        nb = noise.shape[0]
        nz = np.stack([noise[(b if nb > 1 and mutant != "noise_stride_0" else 0)] for b in range(bs)])[:, None, :].astype(dt)
    return g, o, slope, idx, inreg, nz


def scale_ref(gy, out, d, lab, noise, nw, bias, act, nreg, up, chunk_px, want_q, D=None, exact=(), dt=f64, mutant=None):
    """``e4s_mconv_scale``: gz = gy act'(out) d[c] in the parity-planar layout (the float32 expression: two products), and per chunk of ``chunk_px`` output pixels
    q[r] = sum_{p in r} g y, sum g, sum g noise, with g = gy act'(out) and y = out / act'(out) - bias - nw noise (the pre-activation value d z)."""
    bs, cout, H, W = gy.shape
    h, w, P2 = H // up, W // up, H * W
    g, o, slope, idx, inreg, nz = _scale_terms(gy, out, d, lab, noise, nw, bias, act, nreg, up, dt, mutant)
    # gz: the float32 expression
    g32 = gy.reshape(bs, cout, P2).astype(f32)
    if act:
        g32 = g32 * slope.astype(f32)
    dd = np.ones((bs, nreg, cout), f32) if d is None else d.astype(f32)
    d_ext = np.concatenate([dd, np.zeros((bs, 1, cout), f32)], 1)
    sel = idx if mutant != "d_of_the_next_region" else np.where(inreg, (idx + 1) % nreg, nreg)
    dsel = np.take_along_axis(d_ext, sel[:, :, None], 1).transpose(0, 2, 1)                   # [bs, cout, P2]
    gzf = np.where(inreg[:, None, :], g32 * dsel, f32(0)).astype(f32)
    if up == 2:
        order = (5, 3, 0, 1, 2, 4) if mutant == "parity_planes_transposed" else (3, 5, 0, 1, 2, 4)
        gz = gzf.reshape(bs, cout, h, 2, w, 2).transpose(order).reshape(4, bs, cout, h * w)
    else:
        gz = gzf[None]
    res = {"gz": gz.astype(f64)}
    gg = g * slope if act else g
    bv = np.zeros(cout, dt) if bias is None or mutant == "bias_not_subtracted" else bias.astype(dt)
    nwv = dt(0) if noise is None else dt(nw[0])
    y = (o / slope if act else o) - (bv[None, :, None] + nwv * nz)
    nchunk = cdiv(P2, chunk_px)
    t = gg * y
    q = np.zeros((nchunk, bs, nreg, cout), dt)
    db, dn = np.zeros((nchunk, bs, cout), dt), np.zeros((nchunk, bs, cout), dt)
    for ch in range(nchunk):
        sl = slice(ch * chunk_px, min(P2, (ch + 1) * chunk_px))
        for r in range(nreg):
            q[ch, :, r, :] = (t[:, :, sl] * (idx[:, None, sl] == r)).sum(-1)
        m = inreg[:, None, sl] if mutant == "no_region_left_out_of_dbias" else 1.0
        db[ch] = (gg[:, :, sl] * m).sum(-1)
        dn[ch] = (gg[:, :, sl] * nz[:, :, sl]).sum(-1)
    if want_q:
        res["q"] = q.astype(f64)
    res["dbias"] = db.astype(f64)
    if noise is not None:
        res["dnw"] = dn.astype(f64)
    return res


def scale_bar(gy, out, d, lab, noise, nw, bias, act, nreg, up, chunk_px, want_q, D, exact=()):
    """gz 0.  The sums: D U sum|terms| plus the terms' own roundings: g (1), y = out / slope (1), bias + nw noise (2), their difference (1) -> 5 on g y; 1 on g;
    2 on g noise.  An output named in ``exact`` (integer inputs, every partial sum exact): 0."""
    bs, cout, H, W = gy.shape
    P2 = H * W
    g, o, slope, idx, inreg, nz = _scale_terms(gy, out, d, lab, noise, nw, bias, act, nreg, up, f64)
    ga = np.abs(g * slope) if act else np.abs(g)
    A = np.abs(o / slope) if act else np.abs(o)
    B = (0 if bias is None else np.abs(bias.astype(f64))[None, :, None]) + (0 if noise is None else abs(float(nw[0])) * np.abs(nz))
    nchunk = cdiv(P2, chunk_px)
    q, db, dn = np.zeros((nchunk, bs, nreg, cout)), np.zeros((nchunk, bs, cout)), np.zeros((nchunk, bs, cout))
    for ch in range(nchunk):
        sl = slice(ch * chunk_px, min(P2, (ch + 1) * chunk_px))
        for r in range(nreg):
            q[ch, :, r, :] = (ga[:, :, sl] * (A + B)[:, :, sl] * (idx[:, None, sl] == r)).sum(-1)
        db[ch] = ga[:, :, sl].sum(-1)
        dn[ch] = (ga[:, :, sl] * np.abs(nz[:, :, sl])).sum(-1)
    res = {"gz": 0.0, "q": (D + 5) * U * q, "dbias": (D + 1) * U * db, "dnw": (D + 2) * U * dn}
    for k in exact:
        res[k] = 0.0
    return res


def scale_emulate32(gy, out, d, lab, noise, nw, bias, act, nreg, up, chunk_px, want_q, D=None, exact=()):
    """The kernel's own float32 expressions and its chain, butterfly and wave order."""
    bs, cout, H, W = gy.shape
    P2 = H * W
    g, o, slope, idx, inreg, nz = _scale_terms(gy, out, d, lab, noise, nw, bias, act, nreg, up, f32)
    gg = g * slope if act else g
    bv = np.zeros(cout, f32) if bias is None else bias.astype(f32)
    nwv = f32(0) if noise is None else f32(nw[0])
    y = (o / slope if act else o) - (bv[None, :, None].astype(f64) + nwv.astype(f64) * nz).astype(f32)          # (bias + nw noise: one fused multiply-add)
    t = gg * y
    nchunk = cdiv(P2, chunk_px)
    q = np.zeros((nchunk, bs, nreg, cout), f32)
    db, dn = np.zeros((nchunk, bs, cout), f32), np.zeros((nchunk, bs, cout), f32)
    for ch in range(nchunk):
        sl = slice(ch * chunk_px, min(P2, (ch + 1) * chunk_px))
        for r in range(nreg):
            q[ch, :, r, :] = wave_tree32(np.where(idx[:, None, sl] == r, t[:, :, sl], f32(0)))
        db[ch] = wave_tree32(gg[:, :, sl])
        dn[ch] = wave_tree32((gg[:, :, sl].astype(f64) * nz[:, :, sl]).astype(f32))
    res = {"dbias": db}
    if want_q:
        res["q"] = q
    if noise is not None:
        res["dnw"] = dn
    return res


def _scale_cases():
    # (name, bs, cout, h, w, up, nreg, act, d, noise batch (0: none, 1, 'bs'), bias, lab, q, chunk_px, ints)
    rows = [("17x19.act1.d.noiseB.bias.up1.r5.q.c256", 2, 3, 17, 19, 1, 5, 1, 1, "bs", 1, 1, 1, 256, 0),
            ("27x19.act1.d.noise1.bias.up1.r5.q.c256.3chunks", 2, 3, 27, 19, 1, 5, 1, 1, 1, 1, 1, 1, 256, 0),
            ("17x19.act1.nod.noiseB.bias.up2.r5.q.c256.6chunks", 2, 3, 17, 19, 2, 5, 1, 0, "bs", 1, 1, 1, 256, 0),
            ("17x19.act0.d.nonoise.nobias.up1.nolab.r1.noq.c256.ints", 2, 3, 17, 19, 1, 1, 0, 1, 0, 0, 0, 0, 256, 1),
            ("17x19.act1.d.noiseB.nobias.up1.r16.q.c8192", 2, 3, 17, 19, 1, 16, 1, 1, "bs", 0, 1, 1, 8192, 0),
            ("17x19.act0.nod.noise1.nobias.up2.r16.noq.c256", 2, 3, 17, 19, 2, 16, 0, 0, 1, 0, 1, 0, 256, 0),
            ("17x19.act1.d.noiseB.bias.up2.r16.q.c512", 2, 3, 17, 19, 2, 16, 1, 1, "bs", 1, 1, 1, 512, 0)]
    return [dict(name=r[0], bs=r[1], cout=r[2], h=r[3], w=r[4], up=r[5], nreg=r[6], act=r[7], d=r[8], noise=r[9], bias=r[10], lab=r[11], q=r[12], chunk_px=r[13],
                 ints=r[14], D=cdiv(min(r[13], r[5] ** 2 * r[3] * r[4]), 256) + 10) for r in rows]


def _scale_inputs(c):
    n = c["name"]
    bs, cout, H, W = c["bs"], c["cout"], c["up"] * c["h"], c["up"] * c["w"]
    assert c["D"] == depth("scale", chunk_px=c["chunk_px"], px=H * W), c
    gy = ints("scg" + n, (bs, cout, H, W)) if c["ints"] else arr("scg" + n, (bs, cout, H, W))
    out = arr("sco" + n, (bs, cout, H, W))
    out[np.abs(arr("scz" + n, (bs, cout, H, W))) < 0.05] = 0.0                         # a handful of exact zeros; about half of the rest is negative
    assert (out == 0).sum() >= 4 and (out < 0).any()
    nb = bs if c["noise"] == "bs" else c["noise"]
    return dict(gy=gy, out=out if (c["act"] or c["q"]) else None, d=arr("scd" + n, (bs, c["nreg"], cout), 1.0, 0.4) if c["d"] else None,
                lab=labels("scl" + n, bs, H, W, c["nreg"]) if c["lab"] else None, noise=arr("scn" + n, (nb, H * W)) if nb else None,
                nw=np.array([0.7], f32) if nb else None, bias=arr("scb" + n, (cout,), 0.1, 0.3) if c["bias"] else None, act=c["act"], nreg=c["nreg"],
                up=c["up"], chunk_px=c["chunk_px"], want_q=bool(c["q"]), D=c["D"], exact=("dbias",) if c["ints"] else ())


# ================================================================================================ mconv_fold
def _chunk_mask(P, chunk_px, ch):
    m = np.zeros(P)
    m[ch * chunk_px:min(P, (ch + 1) * chunk_px)] = 1.0
    return m


def fold_ref(U_, x, s, lab, ks, nreg, up, chunk_px, want_dx, want_ds, D=None, dt=D64, absolute=False):
    """``e4s_mconv_fold``: dx and the per-chunk ds of sum(U * cols(x, s)), cols the forward of ``e4s_mconv_unfold``, by autograd."""
    xt, st, Ut = T(x, dt).requires_grad_(), T(s, dt).requires_grad_(), T(U_, dt)
    if absolute:
        xt, st, Ut = T(np.abs(x), dt).requires_grad_(), T(np.abs(s), dt).requires_grad_(), Ut.abs()
    cols = _unfold_t(xt, st, lab, ks, up, nreg)
    P = x.shape[2] * x.shape[3]
    res = {}
    if want_dx:
        res["dx"] = N(torch.autograd.grad((cols * Ut).sum(), xt, retain_graph=True)[0]).astype(f64)
    if want_ds:
        nchunk = cdiv(P, chunk_px)
        res["ds_part"] = np.stack([N(torch.autograd.grad((cols * Ut * T(_chunk_mask(P, chunk_px, ch), dt)).sum(), st, retain_graph=True)[0])
                                   for ch in range(nchunk)]).astype(f64)
    return res


def fold_bar(U_, x, s, lab, ks, nreg, up, chunk_px, want_dx, want_ds, D):
    a = fold_ref(U_, x, s, lab, ks, nreg, up, chunk_px, want_dx, want_ds, absolute=True)
    return {k: D[k] * U * v for k, v in a.items()}


def fold_direct(U_, x, s, lab, ks, nreg, up, chunk_px, want_dx, want_ds, D=None, mutant=None):
    """The two sums of the header of csrc/modconv_bwd.hip written out (what the mutants change)."""
    G, KK, PAD = up * up, ks * ks, ks // 2
    bs, cin, h, w = x.shape
    P = h * w
    Uv = U_.astype(f64).reshape(G, bs, cin, KK, h, w)
    s_ext = np.concatenate([s.astype(f64), np.zeros((bs, 1, cin))], 1)
    idx = [region_index(lab, nreg, up, g, bs, h, w, swap=mutant == "parity_swapped") for g in range(G)]
    sv = [np.take_along_axis(s_ext, i[:, :, None], 1).transpose(0, 2, 1).reshape(bs, cin, h, w) for i in idx]
    res = {}
    if want_dx:
        dx = np.zeros((bs, cin, h, w))
        for g in range(G):
            for ky in range(ks):
                for kx in range(ks):
                    dy, dxx = ky - PAD, kx - PAD                    # input position = source position + (dy, dxx)
                    src = Uv[g, :, :, ky * ks + kx]
                    sy, sx = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dxx), w - max(0, dxx))
                    ty, tx = slice(max(0, dy), h + min(0, dy)), slice(max(0, dxx), w + min(0, dxx))
                    m = sv[g][:, :, ty, tx] if mutant == "region_of_the_input" else sv[g][:, :, sy, sx]
                    dx[:, :, ty, tx] += m * src[:, :, sy, sx]
                    flat, sflat = src.reshape(bs, cin, P), sv[g].reshape(bs, cin, P)
                    if mutant == "right_neighbour_read" and dxx == -1:          # source column w: the next row's first element of the flat plane
                        for iy in range(h):
                            e = (iy - dy) * w + w
                            if 0 <= iy - dy < h and e < P:
                                dx[:, :, iy, w - 1] += sflat[:, :, e] * flat[:, :, e]
                    if mutant == "left_tap_kept" and dxx == 1:                 # source column -1: the previous row's last element
                        for iy in range(h):
                            e = (iy - dy) * w - 1
                            if 0 <= iy - dy < h and e >= 0:
                                dx[:, :, iy, 0] += sflat[:, :, e] * flat[:, :, e]
        if mutant == "last_chunk_lost":
            dx.reshape(bs, cin, P)[:, :, (cdiv(P, chunk_px) - 1) * chunk_px:] = 0.0
        res["dx"] = dx
    if want_ds:
        xs = _taps_np(x.astype(f64), ks, 1, PAD, h, w)
        nchunk = cdiv(P, chunk_px)
        ds = np.zeros((nchunk, bs, nreg, cin))
        for g in range(G):
            t = (Uv[g].reshape(bs, cin, KK, P) * xs).sum(2)
            for ch in range(nchunk - (1 if mutant == "last_chunk_lost" else 0)):
                m = _chunk_mask(P, chunk_px, ch)
                for r in range(nreg):
                    ds[ch, :, r, :] += (t * (m * (idx[g] == r))[:, None, :]).sum(-1)
        res["ds_part"] = ds
    return res


def _fold_cases():
    # (h, w, ks, up, nreg, lab, route, chunk_px, u_off, mode, bs, cin).  route: what selects the kernel; vec needs w % 4 == 0, chunk 1024, aligned pointers
    rows = [(1, 4, 3, 1, 5, 1, "vec", 1024, 0, "both", 2, 3), (3, 4, 3, 2, 5, 1, "vec", 1024, 0, "both", 2, 3), (5, 8, 3, 1, 16, 1, "vec", 1024, 0, "dx", 2, 3),
            (6, 20, 3, 2, 5, 1, "vec", 1024, 0, "ds", 2, 3), (6, 20, 3, 1, 1, 0, "vec", 1024, 0, "both", 2, 3), (33, 32, 3, 1, 5, 1, "vec", 1024, 0, "both", 1, 2),
            (5, 8, 3, 1, 16, 1, "c256", 256, 0, "both", 2, 3), (17, 20, 3, 1, 5, 1, "c256", 256, 0, "both", 1, 2), (6, 20, 3, 2, 5, 1, "uoff", 1024, 1, "both", 2, 3),
            (9, 7, 3, 2, 5, 1, "w7", 1024, 0, "both", 2, 3), (9, 7, 3, 1, 16, 1, "w7", 1024, 0, "ds", 2, 3), (1, 4, 3, 2, 1, 0, "c256", 256, 0, "dx", 2, 3),
            (9, 7, 1, 1, 5, 1, "k1", 1024, 0, "both", 2, 3), (6, 20, 1, 2, 16, 1, "k1", 256, 0, "ds", 2, 3), (3, 4, 1, 1, 1, 0, "k1", 1024, 0, "dx", 2, 3)]
    out = []
    for h, w, ks, up, nreg, lab, route, chunk, uoff, mode, bs, cin in rows:
        px = h * w
        out.append(dict(name=f"{h}x{w}.k{ks}.up{up}.r{nreg}.{'lab' if lab else 'nolab'}.{route}.{mode}", h=h, w=w, ks=ks, up=up, nreg=nreg, lab=lab, route=route,
                        chunk_px=chunk, u_off=uoff, mode=mode, bs=bs, cin=cin,
                        D=dict(dx=up * up * ks * ks, ds_part=ks * ks + up * up * cdiv(min(chunk, px), 256) + 10)))
    return out


def fold_route(c):
    """The kernel ``e4s_mconv_fold`` launches for a case (the rule at the end of csrc/modconv_bwd.hip)."""
    if c["ks"] == 1:
        return "mconv_fold_kernel<1>"
    return "mconv_fold4_kernel" if c["w"] % 4 == 0 and c["chunk_px"] % 1024 == 0 and not c["u_off"] else "mconv_fold_kernel<3>"


def _fold_inputs(c):
    n = c["name"]
    assert c["D"]["dx"] == depth("fold_dx", up=c["up"], ks=c["ks"]) and c["D"]["ds_part"] == depth("fold_ds", up=c["up"], ks=c["ks"], chunk_px=c["chunk_px"], px=c["h"] * c["w"])
    assert (fold_route(c) == "mconv_fold4_kernel") == (c["route"] == "vec"), c
    bs, cin, h, w, G = c["bs"], c["cin"], c["h"], c["w"], c["up"] ** 2
    return dict(U_=arr("fou" + n, (G, bs, cin * c["ks"] ** 2, h * w)), x=arr("fox" + n, (bs, cin, h, w)), s=arr("fos" + n, (bs, c["nreg"], cin), 1.0, 0.5),
                lab=labels("fol" + n, bs, c["up"] * h, c["up"] * w, c["nreg"]) if c["lab"] else None, ks=c["ks"], nreg=c["nreg"], up=c["up"], chunk_px=c["chunk_px"],
                want_dx=c["mode"] != "ds", want_ds=c["mode"] != "dx", D=c["D"])


# ================================================================================================ style_tables_bwd
def tables_forward(styles, weight, mod_w, mod_b, ms, lr, dt=D64):
    """s = styles (mod_w ms)^T + mod_b lr;  ws = c weight;  d = rsqrt(s^2 wsq + 1e-8), wsq[i, o] = sum_k ws[o, i, k]^2   (model.py:276-281, one-pass form)."""
    cout, cin, k = weight.shape[1], weight.shape[2], weight.shape[-1]
    c = 1.0 / math.sqrt(cin * k * k)
    s = styles @ (mod_w * ms).t() + mod_b * lr
    ws = weight[0] * c
    wsq = (ws * ws).sum((2, 3)).t()
    d = torch.rsqrt((s * s) @ wsq + 1e-8)
    return s, ws, d, wsq


def tables_given(styles, weight, mod_w, mod_b, ms, lr, **_):
    """(s, d, wsq) as the forward kernels hand them over: the model's, rounded to float32."""
    s, _, d, wsq = tables_forward(T(styles), T(weight), T(mod_w), T(mod_b), ms, lr)
    return N(s).astype(f32), N(d).astype(f32), N(wsq).astype(f32)


def _tables_out(gs, gd, gws, g_styles, g_weight, g_mod_w, g_mod_b):
    res = {}
    if gs is not None or gd is not None:
        res.update(g_styles=g_styles, g_mod_w=g_mod_w, g_mod_b=g_mod_b)
    if gws is not None or gd is not None:
        res["g_weight"] = g_weight
    return res


def tables_ref(styles, weight, mod_w, mod_b, gs, gd, gws, ms, lr, D=None, dt=D64):
    """``e4s_style_tables_bwd``: the gradient of sum(gs s) + sum(gd d) + sum(gws ws) w.r.t. styles, weight, mod_w, mod_b by autograd."""
    leaves = [T(a, dt).requires_grad_() for a in (styles, weight, mod_w, mod_b)]
    s, ws, d, _ = tables_forward(*leaves, ms, lr, dt)
    L = (ws * 0).sum() + (s * 0).sum()
    for g, v in ((gs, s), (gd, d), (gws, ws)):
        if g is not None:
            L = L + (T(g, dt) * v).sum()
    g_styles, g_weight, g_mod_w, g_mod_b = [N(t).astype(f64) for t in torch.autograd.grad(L, leaves)]
    return _tables_out(gs, gd, gws, g_styles, g_weight, g_mod_w, g_mod_b)


def tables_direct(styles, weight, mod_w, mod_b, gs, gd, gws, ms, lr, D=None, mutant=None, absolute=False):
    """The formulas of the header of the tables_bwd kernels written out; ``absolute``: every term by its magnitude (the bars' sum|terms|)."""
    cout, cin, k = weight.shape[1], weight.shape[2], weight.shape[-1]
    c = 1.0 / math.sqrt(cin * k * k)
    s32, d32, wsq32 = tables_given(styles, weight, mod_w, mod_b, ms, lr)
    a = np.abs if absolute else (lambda v: v)
    rows = styles.shape[0] * styles.shape[1]
    st, s, d, wsq = a(styles.astype(f64).reshape(rows, -1)), a(s32.astype(f64).reshape(rows, cin)), d32.astype(f64).reshape(rows, cout), wsq32.astype(f64)
    mw, w = a(mod_w.astype(f64)), a(weight.astype(f64))
    gsv = np.zeros((rows, cin)) if gs is None else a(gs.astype(f64).reshape(rows, cin))
    t = np.zeros((rows, cout)) if gd is None else a(-0.5 * gd.astype(f64).reshape(rows, cout) * d ** 3)
    wq = wsq.reshape(cout, cin).T if mutant == "wsq_transposed" else wsq
    gsp = gsv + (1.0 if mutant == "factor_2_missing" else 2.0) * s * (t @ wq.T)
    gwsq = t.T @ (s * s)                                                                       # [cout, cin]
    g_weight = c * ((0 if gws is None else a(gws.astype(f64))) + 2.0 * c * w[0] * gwsq[:, :, None, None])[None]
    gsr = gsp.copy()
    if mutant == "last_quarter_lost":
        gsr[:, 3 * cdiv(cin, 4):] = 0.0
    g_styles = ms * gsr @ mw
    g_mod_w = (lr if mutant == "mod_lr_on_g_mod_w" else ms) * gsp.T @ st
    g_mod_b = abs(lr) * gsp.sum(0) if absolute else lr * gsp.sum(0)
    if absolute:
        g_styles, g_mod_w = np.abs(g_styles), np.abs(g_mod_w)
    return _tables_out(gs, gd, gws, g_styles.reshape(styles.shape), g_weight, g_mod_w, g_mod_b)


def tables_bar(styles, weight, mod_w, mod_b, gs, gd, gws, ms, lr, D):
    a = tables_direct(styles, weight, mod_w, mod_b, gs, gd, gws, ms, lr, absolute=True)
    return {k: D[k] * U * v for k, v in a.items()}


def _tables_cases():
    out = []
    for bs, nreg, sdim, cin, cout, k in ((1, 5, 70, 5, 300, 3), (2, 3, 16, 260, 8, 1)):
        rows = bs * nreg
        for have in ("all", "nogs", "nogd", "nogws"):
            gd = have != "nogd"
            out.append(dict(name=f"rows{rows}.sd{sdim}.cin{cin}.cout{cout}.kk{k * k}.{have}", bs=bs, nreg=nreg, sdim=sdim, cin=cin, cout=cout, k=k, have=have,
                            D=dict(g_styles=(cout + 10 if gd else 0) + cdiv(cin, 4) + 5, g_mod_w=(cout + 10 if gd else 0) + cdiv(rows, 4) + 5,
                                   g_mod_b=(cout + 10 if gd else 0) + cdiv(rows, 4) + 5, g_weight=rows + 12)))
    return out


def _tables_inputs(c):
    n = f"{c['cin']}.{c['cout']}"
    bs, nreg, sdim, cin, cout, k = c["bs"], c["nreg"], c["sdim"], c["cin"], c["cout"], c["k"]
    gd = c["have"] != "nogd"
    assert c["D"]["g_styles"] == depth("tables", cout=cout, gd=gd, n=cin) and c["D"]["g_mod_w"] == depth("tables", cout=cout, gd=gd, n=bs * nreg)
    assert c["D"]["g_weight"] == depth("tables_w", rows=bs * nreg)
    return dict(styles=arr("tbst" + n, (bs, nreg, sdim)), weight=arr("tbw" + n, (1, cout, cin, k, k)), mod_w=arr("tbmw" + n, (cin, sdim)),
                mod_b=arr("tbmb" + n, (cin,), 1.0, 0.3), gs=None if c["have"] == "nogs" else arr("tbgs" + n, (bs, nreg, cin)),
                gd=arr("tbgd" + n, (bs, nreg, cout)) if gd else None, gws=None if c["have"] == "nogws" else arr("tbgw" + n, (cout, cin, k, k)),
                ms=1.0 / math.sqrt(sdim), lr=0.37, D=c["D"])


# ================================================================================================ gemm_sb / mconv_wgrad: the split-bf16 GEMM
def ksplit_rule(tiles, nchunk, batch, M, N, workspace_floats, tile_cap=512, chunks_min=4, ks_max=1024):
    """The ``while`` of e4s_gemm_sb / e4s_mconv_wgrad: doubled while there are fewer than 512 workgroups, every slice keeps 4 chunks and the workspace holds it."""
    ks = 1
    while workspace_floats and tiles * batch * ks < tile_cap and ks * 2 * chunks_min <= nchunk and ks * 2 * batch * M * N <= workspace_floats and ks < ks_max:
        ks *= 2
    return ks


def split_numbers(path, anchor):
    """(tile cap, chunks per slice, largest split) read from the first ``while`` after ``anchor`` in a source file of the project."""
    src = open(os.path.join(ROOT, path)).read()
    line = src[src.index(anchor):]
    line = re.search(r"^\s*while\b.*$", line, re.M).group(0)
    cap = int(re.search(r"<\s*(\d+)\s*(?:&&|and)", line).group(1))
    chunks = int(re.search(r"\*\s*2\s*\*\s*(\d+)\s*<=\s*nchunk", line).group(1))
    top = int(re.search(r"(?<!\* )\b(?:ksplit|kspl|ks)\s*<\s*(\d+)", line).group(1))
    return cap, chunks, top


def gemm_tiles(M, N, a_kc, b_kc):
    skinny = bool(a_kc and b_kc and M <= 8)
    return cdiv(M, 32 if skinny else 128) * cdiv(N, 256 if skinny else 128)


def gemm_ops(a, b, M, N, K, a_kc, b_kc, **_):
    """The logical operands opA [Ba, M, K], opB [Bb, K, N] of the stored (padded) ones."""
    A = a[:, :, :K] if a_kc else a[:, :, :M].transpose(0, 2, 1)
    B = b[:, :, :K].transpose(0, 2, 1) if b_kc else b[:, :, :N]
    return A, B


def gemm_ref(a, b, M, N, K, a_kc, b_kc, dt=f64, **_):
    A, B = gemm_ops(a, b, M, N, K, a_kc, b_kc)
    return {"c": np.matmul(A.astype(dt), B.astype(dt)).astype(f64)}


def gemm_bar(a, b, M, N, K, a_kc, b_kc, D, **_):
    A, B = gemm_ops(a, b, M, N, K, a_kc, b_kc)
    return {"c": (SPLIT + D * U) * np.matmul(np.abs(A).astype(f64), np.abs(B).astype(f64))}


def _split(v):
    hi, lo = split_terms(torch.from_numpy(np.ascontiguousarray(v, dtype=f32)), 2, torch.bfloat16)
    return hi.double().numpy(), lo.double().numpy()


PRODUCTS = ((0, 0), (0, 1), (1, 0))              # (A term, B term) in the kernels' MFMA order: hi*hi, hi*lo, lo*hi


def gemm_emulate(a, b, M, N, K, a_kc, b_kc, drop=None, mutant=None, ksplit=1, **_):
    """Both operands split RNE into bf16 hi and lo, hi*hi + hi*lo + lo*hi summed in float64.  ``drop``: one product left out."""
    A, B = gemm_ops(a, b, M, N, K, a_kc, b_kc)
    if mutant == "lda_taken_as_K":
        flat = a.reshape(a.shape[0], -1)
        A = flat[:, :M * K].reshape(-1, M, K) if a_kc else flat[:, :M * K].reshape(-1, K, M).transpose(0, 2, 1)
    if mutant == "k_tail_not_zeroed" and K % 32:              # the clamped reads of g_load enter the MFMA: k >= K repeats the last float4 (K-contiguous) or k = K - 1
        e = 32 - K % 32
        ta = A[:, :, K - 4:][:, :, np.arange(e) % 4] if a_kc else np.repeat(A[:, :, K - 1:], e, 2)
        tb = B[:, K - 4:, :][:, np.arange(e) % 4, :] if b_kc else np.repeat(B[:, K - 1:, :], e, 1)
        A, B = np.concatenate([A, ta], 2), np.concatenate([B, tb], 1)
    if mutant == "last_slice_lost" and ksplit > 1:
        per = cdiv(cdiv(K, 32), ksplit)
        last = (cdiv(cdiv(K, 32), per) - 1) * per * 32
        A, B = A[:, :, :last], B[:, :last, :]
    At, Bt = _split(A), _split(B)
    c = 0.0
    for i, j in PRODUCTS:
        if (i, j) != drop:
            c = c + np.matmul(At[i], Bt[j])
    c = np.broadcast_to(c, (max(a.shape[0], b.shape[0]), M, N)).copy()
    if mutant == "row_beyond_M_written" and c.shape[0] > 1:    # row M of sample b is row 0 of sample b + 1 in the dense output
        c[1:, 0, :] = c[:-1, M - 1, :]
    return {"c": c}


def gemm_emulate32(a, b, M, N, K, a_kc, b_kc, ksplit=1, **_):
    """``gemm_emulate`` with float32 accumulation in the kernel's order: per split-K slice one accumulator that takes, 16 k at a time, the three MFMAs (each the exact
    sum of its 16 products, rounded once into the accumulator); an empty slice is a zero; the slices added to 0 in order (``gemm_sb_finalize_kernel``) or, for at
    most 65536 outputs and 16 slices or more, as four strided chains and (r0 + r1) + (r2 + r3) (``gemm_sb_finalize_wide_kernel``)."""
    A, B = gemm_ops(a, b, M, N, K, a_kc, b_kc)
    At, Bt = _split(A), _split(B)
    batch = max(a.shape[0], b.shape[0])
    nchunk = cdiv(K, 32)
    per = cdiv(nchunk, ksplit)
    parts = []
    for ks in range(ksplit):
        acc = np.zeros((batch, M, N), f32)
        for ch in range(ks * per, min(nchunk, (ks + 1) * per)):
            for t in range(2):
                k0, k1 = 32 * ch + 16 * t, min(K, 32 * ch + 16 * t + 16)
                if k0 >= K:
                    continue                                   # (an MFMA of zeros adds an exact zero)
                for i, j in PRODUCTS:
                    acc = (acc.astype(f64) + np.matmul(At[i][:, :, k0:k1], Bt[j][:, k0:k1, :])).astype(f32)
        parts.append(acc)
    if ksplit == 1:
        return {"c": parts[0]}
    if batch * M * N <= 65536 and ksplit >= 16:
        r = []
        for p in range(4):
            v = np.zeros((batch, M, N), f32)
            for k in range(p, ksplit, 4):
                v = v + parts[k]
            r.append(v)
        return {"c": (r[0] + r[1]) + (r[2] + r[3])}
    v = np.zeros((batch, M, N), f32)
    for p in parts:
        v = v + p
    return {"c": v}


def descaled(c, inp):
    """An output with the case's power-of-two row and column scales taken out again (exact: the split and every sum scale with them)."""
    if inp.get("row_scale") is None:
        return c
    return c / inp["row_scale"][None, :, None] / inp["col_scale"][None, None, :]


def _gemm_cases():
    # (M, N, K, batch, a_kc, b_kc, shared ('a', 'b' or ''), pad, workspace, scaled, note)
    rows = [(128, 128, 64, 1, 1, 1, "", 0, 1, 0, ""), (3, 288, 4096, 2, 1, 1, "", 0, 1, 0, "skinny.split"), (3, 288, 4096, 2, 0, 0, "", 0, 1, 0, "split"),
            (200, 70, 100, 3, 1, 0, "a", 0, 1, 0, "ktail"), (200, 70, 100, 3, 0, 1, "a", 0, 1, 0, "ktail"), (513, 129, 36, 1, 0, 0, "", 0, 1, 0, "ktail"),
            (513, 129, 36, 1, 1, 1, "", 0, 1, 0, "ktail"), (32, 288, 16, 4, 1, 1, "a", 0, 1, 0, ""), (32, 288, 16, 4, 0, 0, "a", 0, 1, 0, ""),
            (70, 50, 40, 2, 1, 1, "", 1, 1, 0, "lda"), (70, 50, 40, 2, 0, 0, "", 1, 1, 0, "lda"), (70, 50, 40, 2, 1, 0, "", 1, 1, 0, "lda"), (70, 50, 40, 2, 0, 1, "", 1, 1, 0, "lda"),
            (70, 50, 40, 3, 1, 0, "b", 0, 1, 0, "stride_b0"), (70, 50, 40, 3, 0, 1, "a", 0, 1, 0, "stride_a0"), (20, 30, 4, 1, 1, 1, "", 0, 1, 0, "k4"), (20, 30, 36, 1, 0, 0, "", 0, 1, 0, "k36"),
            (8, 257, 64, 2, 1, 1, "", 0, 1, 0, "skinny"), (9, 257, 64, 2, 1, 1, "", 0, 1, 0, "notskinny"), (128, 128, 1056, 1, 1, 1, "", 0, 1, 0, "emptyslice"),
            (128, 128, 1056, 1, 1, 1, "", 0, 0, 0, "nows"), (128, 128, 4100, 1, 1, 1, "", 0, 1, 0, "wide"), (128, 128, 4100, 1, 0, 0, "", 0, 1, 0, "wide"), (128, 128, 4064, 1, 1, 1, "", 0, 1, 0, "wide16"),
            (40, 24, 96, 1, 1, 1, "", 0, 1, 1, "scaled"), (40, 24, 96, 1, 0, 0, "", 0, 1, 1, "scaled")]
    out = []
    for M, N, K, batch, akc, bkc, sh, pad, ws, sc, note in rows:
        ksp = ksplit_rule(gemm_tiles(M, N, akc, bkc), cdiv(K, 32), batch, M, N, 1 << 40 if ws else 0)
        out.append(dict(name=f"{'kc' if akc else 'mc'}_{'kc' if bkc else 'mc'}.{M}x{N}x{K}.b{batch}" + (f".share_{sh}" if sh else "") + (f".{note}" if note else ""),
                        M=M, N=N, K=K, batch=batch, a_kc=akc, b_kc=bkc, share=sh, pad=pad, ws=ws, scaled=sc, ksplit=ksp, D=3 * cdiv(K, 16) + ksp))
    return out


def _gemm_inputs(c):
    n = c["name"]
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    assert c["D"] == depth("mfma", K=K, ksplit=c["ksplit"]), c
    Ba, Bb = (1 if c["share"] == "a" else batch), (1 if c["share"] == "b" else batch)
    A, B = arr("gea" + n, (Ba, M, K)), arr("geb" + n, (Bb, K, N))
    rs = cs = None
    if c["scaled"]:
        rs, cs = (2.0 ** (np.arange(M) % 13 - 6)).astype(f32), (2.0 ** (np.arange(N) * 5 % 13 - 6)).astype(f32)
        A, B = A * rs[None, :, None], B * cs[None, None, :]
    a = A if c["a_kc"] else A.transpose(0, 2, 1)
    b = B.transpose(0, 2, 1) if c["b_kc"] else B
    if c["pad"]:                                            # lda = K + 4 / M + 4, ldb = K + 8 / N + 3, the padding poisoned
        a = np.concatenate([a, np.full(a.shape[:2] + (4,), POISON, f32)], 2)
        b = np.concatenate([b, np.full(b.shape[:2] + (8 if c["b_kc"] else 3,), POISON, f32)], 2)
    return dict(a=np.ascontiguousarray(a), b=np.ascontiguousarray(b), M=M, N=N, K=K, a_kc=c["a_kc"], b_kc=c["b_kc"], batch=batch, ws=c["ws"], ksplit=c["ksplit"], D=c["D"],
                row_scale=rs, col_scale=cs)


# ------------------------------------------------------------------------------------------------ mconv_wgrad: the same GEMM on a virtual B
def wgrad_as_gemm(gz, x, s, lab, ks, up, nreg, ksplit, D=None, mutant=None):
    """A = gz [G bs, cout, P], B row (ci, tap) = the modulated im2col row the kernel builds while staging: one float32 product s x."""
    G, bs, cout, P = gz.shape
    cin = x.shape[1]
    sv = np.ones((bs, 1, cin), f32) if s is None else s
    cols = unfold_ref(x, sv, lab, ks, up, nreg if s is not None else 1, mutant=mutant)["cols"].astype(f32)
    return dict(a=gz.reshape(G * bs, cout, P), b=cols.reshape(G * bs, cin * ks * ks, P), M=cout, N=cin * ks * ks, K=P, a_kc=1, b_kc=1, ksplit=ksplit, D=D)


def _wg(fn):
    def run(mutant=None, drop=None, **inp):
        kw = {}
        if drop is not None:
            kw["drop"] = drop
        if mutant in ("last_slice_lost",):
            kw["mutant"], mutant = mutant, None
        r = fn(**wgrad_as_gemm(mutant=mutant, **inp), **kw)
        return {"dw": r["c"]}
    return run


wgrad_ref, wgrad_bar, wgrad_emulate, wgrad_emulate32 = _wg(gemm_ref), _wg(gemm_bar), _wg(gemm_emulate), _wg(gemm_emulate32)


def wgrad_stock(**inp):
    return {"dw": gemm_ref(dt=f32, **wgrad_as_gemm(**inp))["c"]}


def wgrad_tiles(cout, n):
    return cdiv(cout, 32 if cout <= 32 else (64 if cout <= 64 else 128)) * cdiv(n, 128)


def _wgrad_cases():
    # (ks, cin, cout, h, w, up, nreg, masked, bs, labels: 'stray', 'all16' (every region in one 16-pixel run, one uniform run), 'none')
    rows = [(1, 130, 3, 2, 16, 1, 5, 1, 2, "stray", "2Ntiles.tm32"), (1, 260, 48, 2, 16, 1, 5, 1, 1, "stray", "3Ntiles.tm64"),
            (3, 20, 130, 3, 16, 2, 5, 1, 1, "stray", "ktail.tm128"), (3, 16, 64, 4, 32, 1, 1, 0, 2, "none", "plain"),
            (1, 130, 3, 1, 32, 1, 16, 1, 1, "all16", "h1.uni"), (3, 20, 40, 16, 16, 1, 16, 1, 1, "all16", "split"), (3, 20, 40, 33, 16, 1, 5, 1, 1, "stray", "tail16.split")]
    out = []
    for ks, cin, cout, h, w, up, nreg, masked, bs, lab, note in rows:
        ksp = ksplit_rule(wgrad_tiles(cout, cin * ks * ks), cdiv(h * w, 32), up * up * bs, cout, cin * ks * ks, 1 << 40)
        out.append(dict(name=f"k{ks}.cin{cin}.cout{cout}.{h}x{w}.up{up}.r{nreg}.{'masked' if masked else 'plain'}.b{bs}.{lab}.{note}", ks=ks, cin=cin, cout=cout, h=h,
                        w=w, up=up, nreg=nreg, masked=masked, bs=bs, lab=lab, ksplit=ksp, D=3 * cdiv(h * w, 16) + ksp))
    return out


def _wgrad_inputs(c):
    n = c["name"]
    bs, cin, cout, h, w, up = c["bs"], c["cin"], c["cout"], c["h"], c["w"], c["up"]
    assert c["D"] == depth("mfma", K=h * w, ksplit=c["ksplit"]), c
    lab = None
    if c["lab"] == "stray":
        lab = labels("wgl" + n, bs, up * h, up * w, c["nreg"])
        lab[:, 0, :up * 16] = 2                              # one uniform run as well
    elif c["lab"] == "all16":
        lab = labels("wgl" + n, bs, up * h, up * w, c["nreg"], stray=False)
        lab[:, 0, :16] = np.arange(16, dtype=np.uint8)
        if w > 16:
            lab[:, 0, 16:32] = 7
        else:
            lab[:, 1, :16] = 7
        if h > 1:
            lab[:, -1, -3:] = 255
    return dict(gz=arr("wgg" + n, (up * up, bs, cout, h * w)), x=arr("wgx" + n, (bs, cin, h, w)), s=arr("wgs" + n, (bs, c["nreg"], cin), 1.0, 0.5) if c["masked"] else None,
                lab=lab, ks=c["ks"], up=up, nreg=c["nreg"], ksplit=c["ksplit"], D=c["D"])


# ================================================================================================ mconv_dgrad (fused data and style gradient)
def _dgrad_U(gz, wg, split=False, drop=None, acc32=False):
    """U[g, b, (i, k), p] = sum_o wg[g, o, i, k] gz[g, b, o, p]; ``split``: the three products of the split operands; ``acc32``: a tap's accumulator in float32,
    taking per chunk of 16 output channels the three MFMAs in the kernel's order (each the exact sum of its 16 products, rounded once)."""
    G, bs, cout, P = gz.shape
    cin = wg.shape[2]
    W2 = wg.reshape(G, 1, cout, cin * 9).transpose(0, 1, 3, 2)
    if not split:
        return np.matmul(W2.astype(f64), gz.astype(f64))
    Wt, Gt = _split(W2), _split(gz)
    if acc32:
        u = np.zeros((G, bs, cin * 9, P), f32)
        for o0 in range(0, cout, 16):
            for i, j in PRODUCTS:
                u = (u.astype(f64) + np.matmul(Wt[i][..., o0:o0 + 16], Gt[j][:, :, o0:o0 + 16, :])).astype(f32)
        return u.astype(f64)
    u = 0.0
    for i, j in PRODUCTS:
        if (i, j) != drop:
            u = u + np.matmul(Wt[i], Gt[j])
    return u


def dgrad_ref(gz, wg, x, s, lab, nreg, up, want_dx, want_ds, D=None, dt=f64, drop=None, split=False, acc32=False, absolute=False):
    """``e4s_mconv_dgrad``: U = W^T gz (never stored), then the two sums of ``e4s_mconv_fold``; ds summed over the kernel's tiles."""
    if absolute:
        gz, wg = np.abs(gz), np.abs(wg)
    u = _dgrad_U(gz.astype(dt), wg.astype(dt), split=split, drop=drop, acc32=acc32)
    r = fold_ref(u, x, s, lab, 3, nreg, up, 1 << 30, want_dx, want_ds, dt=D64 if dt == f64 else D32, absolute=absolute)
    if "ds_part" in r:
        r["ds"] = r.pop("ds_part")[0]
    return r


def dgrad_emulate(drop=None, **inp):
    return dgrad_ref(split=True, drop=drop, **inp)


def dgrad_emulate32(**inp):
    """The nine accumulators in float32 in the kernel's chunk and MFMA order; what follows them (``* s``, the col2im sums, the style sums) in float64."""
    return dgrad_ref(split=True, acc32=True, **inp)


def dgrad_bar(D, **inp):
    a = dgrad_ref(absolute=True, **inp)
    return {k: (SPLIT + D[k] * U) * v for k, v in a.items()}


def _dgrad_cases():
    rows = [(1, 32, 5, 33, 16, 1, 1, "both", 1), (7, 33, 24, 33, 16, 1, 1, "both", 2), (7, 61, 5, 33, 5, 2, 1, "dx", 1), (7, 32, 24, 33, 1, 1, 0, "ds", 1),
            (1, 61, 24, 33, 16, 2, 1, "both", 1)]
    out = []
    for h, w, cout, cin, nreg, up, lab, mode, bs in rows:
        m = 3 * cdiv(cout, 16)
        out.append(dict(name=f"{h}x{w}.cout{cout}.cin{cin}.r{nreg}.up{up}.{'lab' if lab else 'nolab'}.{mode}.b{bs}", h=h, w=w, cout=cout, cin=cin, nreg=nreg, up=up, lab=lab,
                        mode=mode, bs=bs, D=dict(dx=m + 1 + 9 * up * up, ds=m + 9 + 5 + up * up + 8 + cdiv(h, 6) * cdiv(w, 30))))
    return out


def _dgrad_inputs(c):
    # D: the MFMAs of a tap's accumulator; dx: ``* s``, the nine shifted planes of every group added; ds: nine fused multiply-adds, the half-wave's shuffles (5),
    # ``dsw +=`` per group, the eight waves, the tiles (added by the caller)
    n = c["name"]
    bs, cin, cout, h, w, up = c["bs"], c["cin"], c["cout"], c["h"], c["w"], c["up"]
    return dict(gz=arr("dgg" + n, (up * up, bs, cout, h * w)), wg=arr("dgw" + n, (up * up, cout, cin, 3, 3), 0.0, 0.2), x=arr("dgx" + n, (bs, cin, h, w)),
                s=arr("dgs" + n, (bs, c["nreg"], cin), 1.0, 0.5), lab=labels("dgl" + n, bs, up * h, up * w, c["nreg"]) if c["lab"] else None, nreg=c["nreg"], up=up,
                want_dx=c["mode"] != "ds", want_ds=c["mode"] != "dx", D=c["D"])


# ================================================================================================ grouped_linear
def _lrelu(v, slope, lib):
    return lib.where(v > 0, v, v * slope)


def linear_ref(x, W, bias, addend, scale, bias_mul, act, slope, D=None, route=None, dt=f64, mutant=None):
    """``e4s_grouped_linear``: act(scale W[g] x[b, g] + bias_mul bias[g]) + addend  (EqualLinear, model.py:154-162; LocalMLP, networks.py:23-49)."""
    xv = x.astype(dt)
    v = np.stack([xv[:, g] @ W[g].astype(dt).T for g in range(len(W))], 1) * dt(scale)
    if bias is not None:
        v = v + np.stack(bias).astype(dt)[None] * (dt(1) if mutant == "bias_mul_missing" else dt(bias_mul))
    if addend is not None and mutant == "addend_before_act":
        v = v + addend.astype(dt)
    if act:
        v = _lrelu(v, dt(slope), np) * (dt(SQ2) if act == 2 else dt(1))
    if addend is not None and mutant != "addend_before_act":
        v = v + addend.astype(dt)
    if mutant == "ninth_row_dropped" and v.shape[0] > 8:
        v[8] = 0
    return {"out": v.astype(f64)}


def linear_bar(x, W, bias, addend, scale, bias_mul, act, slope, D, route=None):
    """S = scale sum|w||x| carries the sum's D roundings; every later step (bias, activation, gain, addend) one rounding of the value it produces."""
    S = np.stack([np.abs(x[:, g]).astype(f64) @ np.abs(W[g]).astype(f64).T for g in range(len(W))], 1) * abs(scale)
    V = S + (0 if bias is None else np.abs(np.stack(bias)).astype(f64)[None] * abs(bias_mul))
    gain = float(SQ2) if act == 2 else 1.0
    return {"out": U * (gain * (D * S + 6 * V) + (0 if addend is None else np.abs(addend).astype(f64)))}


def _linear_cases():
    # (bs, groups, in, out, act, bias, addend, x: 1 = offset by one float, 2 = rows in + 1 floats apart (both leave the vector route though in % 4 == 0),
    #  out a slice of a wider buffer)
    rows = [(17, 16, 260, 7, 1, 1, 1, 0, 0), (9, 1, 512, 512, 2, 1, 0, 0, 0), (2, 2, 30, 7, 0, 1, 1, 0, 0), (16, 2, 30, 7, 1, 0, 1, 0, 0), (8, 3, 64, 9, 2, 1, 0, 1, 0),
            (3, 2, 64, 5, 0, 1, 1, 0, 1), (2, 2, 30, 7, 2, 0, 0, 0, 1), (3, 2, 64, 5, 1, 1, 1, 2, 0)]
    out = []
    for bs, g, i, o, act, b, ad, xo, sl in rows:
        vec = i % 4 == 0 and not xo
        out.append(dict(name=f"b{bs}.g{g}.in{i}.out{o}.act{act}" + ("" if b else ".nobias") + ("" if ad else ".noaddend") + ("", ".xoff", ".xstride")[xo] + (".outslice" if sl else "")
                        + (".vec" if vec else ".scalar"), bs=bs, groups=g, in_dim=i, out_dim=o, act=act, bias=b, addend=ad, xoff=xo, outslice=sl, vec=vec,
                        D=(4 * cdiv(i, 256) if vec else cdiv(i, 64)) + 7))
    return out


def _linear_inputs(c):
    n = c["name"]
    assert c["D"] == depth("linear", n=c["in_dim"], vec=c["vec"]), c
    g, i, o = c["groups"], c["in_dim"], c["out_dim"]
    return dict(x=arr("lix" + n, (c["bs"], g, i)), W=[arr(f"liw{k}" + n, (o, i)) for k in range(g)], bias=[arr(f"lib{k}" + n, (o,)) for k in range(g)] if c["bias"] else None,
                addend=arr("lia" + n, (o,)) if c["addend"] else None, scale=1.0 / math.sqrt(i), bias_mul=0.6, act=c["act"], slope=0.2, D=c["D"],
                route=dict(xoff=c["xoff"], outslice=c["outslice"]))


# ------------------------------------------------------------------------------------------------ grouped_linear_bwd
def linbwd_ref(gy, x, W, h_prev, scale, bias_mul, slope, osplit, want, D=None, dt=D64, mutant=None, absolute=False):
    """``e4s_grouped_linear_bwd``: the gradient of sum(gy (scale W lrelu(pre) + bias_mul b)) w.r.t. W, b and pre by autograd, where ``h_prev`` = lrelu(pre) is the
    layer's input (``h_prev`` None: w.r.t. the input x itself)."""
    a = np.abs if absolute else (lambda v: v)
    Wt = T(a(np.stack(W)), dt).requires_grad_()
    bt = torch.zeros((len(W), W[0].shape[0]), dtype=dt, requires_grad=True)
    sl = 1.0 if absolute else slope
    if h_prev is not None:
        pre = T(np.where(h_prev > 0, a(h_prev), a(h_prev) / sl), dt).requires_grad_()
        xin = F.leaky_relu(pre, sl)
        if mutant == "lrelu_ge":
            xin = torch.where(pre >= 0, pre, pre * sl)
    else:
        pre = T(a(x), dt).requires_grad_()
        xin = pre
    sc = scale * scale if mutant == "scale_twice" else scale
    y = torch.einsum("goi,bgi->bgo", Wt, xin) * sc + bt[None] * bias_mul
    gW, gb, gx = torch.autograd.grad((T(a(gy), dt) * y).sum(), [Wt, bt, pre])
    if mutant == "empty_slice_not_zeroed":                     # slices past out_dim: whatever the scratch held
        per = cdiv(W[0].shape[0], osplit)
        empty = sum(1 for os_ in range(osplit) if os_ * per >= W[0].shape[0])
        gx = gx + empty * POISON * scale
    res = {"dW": N(gW), "db": N(gb), "dx": N(gx)}
    return {k: v.astype(f64) for k, v in res.items() if k in want}


def linbwd_bar(D, **inp):
    a = linbwd_ref(absolute=True, **inp)
    return {k: D[k] * U * v for k, v in a.items()}


def _linbwd_cases():
    # (bs, groups, in, out, osplit, h_prev, want)
    rows = [(1, 1, 4, 5, 1, 0, "Wbx"), (3, 5, 4, 13, 8, 1, "Wbx"), (8, 5, 1028, 13, 32, 1, "Wbx"), (8, 1, 1028, 5, 8, 0, "Wbx"), (3, 5, 1028, 5, 32, 1, "x"),
            (8, 5, 4, 13, 1, 1, "Wb"), (3, 1, 1028, 13, 8, 0, "Wx"), (1, 5, 4, 5, 32, 1, "Wbx")]
    out = []
    for bs, g, i, o, osp, hp, want in rows:
        w = tuple({"W": "dW", "b": "db", "x": "dx"}[k] for k in want)
        out.append(dict(name=f"b{bs}.g{g}.in{i}.out{o}.os{osp}" + (".hprev" if hp else "") + "." + want + (".emptyslices" if osp > o else ""), bs=bs, groups=g, in_dim=i,
                        out_dim=o, osplit=osp, hprev=hp, want=w, D=dict(dW=bs + 1, db=bs + 1, dx=cdiv(o, osp) + osp + 2)))
    return out


def _linbwd_inputs(c):
    n = c["name"]
    assert c["D"]["dW"] == depth("lin_dw", bs=c["bs"]) and c["D"]["dx"] == depth("lin_dx", out=c["out_dim"], osplit=c["osplit"]), c
    g, i, o = c["groups"], c["in_dim"], c["out_dim"]
    x = arr("lbx" + n, (c["bs"], g, i))
    if c["hprev"]:
        x[np.abs(arr("lbz" + n, (c["bs"], g, i))) < 0.2] = 0.0          # exact zeros in the previous layer's output
        assert (x == 0).any() and (x < 0).any()
    return dict(gy=arr("lbg" + n, (c["bs"], g, o)), x=x, W=[arr(f"lbw{k}" + n, (o, i)) for k in range(g)], h_prev=x if c["hprev"] else None, scale=1.0 / math.sqrt(i),
                bias_mul=0.6, slope=0.2, osplit=c["osplit"], want=c["want"], D=c["D"])


# ================================================================================================ small_map
def small_ref(Tm, src, trans, grouped, D=None, dt=f64, mutant=None):
    """``e4s_small_map``: out[j, n] = sum_k T[j, k] w[n, k] (grouped: out[j // 9, n, j % 9]); transposed: dw[n, k] = sum_j T[j, k] g[j, n]."""
    J, K = Tm.shape
    Tv = Tm.astype(dt)
    if mutant == "T_transposed":
        Tv = np.ascontiguousarray(Tv.T).reshape(J, K)
    if not trans:
        out = Tv @ src.astype(dt).T                                               # [J, N]
        if grouped:
            out = out.reshape(J // 9, 9, -1).transpose(0, 2, 1)
        return {"out": out.astype(f64)}
    g = src.astype(dt)
    if grouped:
        g = g.transpose(0, 2, 1).reshape(J, -1)
    return {"out": (g.T @ Tv).astype(f64)}


def small_bar(Tm, src, trans, grouped, D):
    return {"out": D * U * small_ref(np.abs(Tm), np.abs(src), trans, grouped)["out"]}


def _small_cases():
    rows = [(5, 7, 300, 0, 0), (5, 7, 300, 1, 0), (36, 36, 300, 0, 0), (36, 36, 300, 1, 0), (36, 9, 257, 0, 0), (36, 9, 257, 1, 0), (36, 9, 257, 0, 1), (36, 9, 257, 1, 1)]
    return [dict(name=f"J{J}.K{K}.N{n}.{'trans' if t else 'fwd'}" + (".grouped" if g else "") + (".fixed" if (J, K) == (36, 9) else ".generic"), J=J, K=K, N=n, trans=t, grouped=g,
                 D=J if t else K) for J, K, n, t, g in rows]


def _small_inputs(c):
    n = c["name"]
    assert c["D"] == depth("small", n=c["J"] if c["trans"] else c["K"]), c
    J, K, Nn = c["J"], c["K"], c["N"]
    shape = (Nn, K) if not c["trans"] else ((J // 9, Nn, 9) if c["grouped"] else (J, Nn))
    return dict(Tm=arr("smt" + n, (J, K)), src=arr("sms" + n, shape), trans=c["trans"], grouped=c["grouped"], D=c["D"])


# ================================================================================================ the tables
def _mut(fn, name):
    return lambda **inp: fn(mutant=name, **inp)


def _f32(fn, dt=f32):
    return lambda **inp: fn(dt=dt, **inp)


OPS = {
    # op: (cases, inputs, reference64, bar, stock32, emulate32 or None)
    "mconv_unfold": (_unfold_cases(), _unfold_inputs, unfold_ref, zero_bar("cols"), _f32(unfold_ref), None),
    "unfold2d": (_unfold2d_cases(), _unfold2d_inputs, unfold2d_ref, zero_bar("cols"), _f32(unfold2d_ref), None),
    "mconv_scale": (_scale_cases(), _scale_inputs, scale_ref, scale_bar, _f32(scale_ref), scale_emulate32),
    "mconv_fold": (_fold_cases(), _fold_inputs, fold_ref, fold_bar, _f32(fold_ref, D32), None),
    "style_tables_bwd": (_tables_cases(), _tables_inputs, tables_ref, tables_bar, _f32(tables_ref, D32), None),
    "gemm_sb": (_gemm_cases(), _gemm_inputs, gemm_ref, gemm_bar, _f32(gemm_ref), gemm_emulate32),
    "mconv_wgrad": (_wgrad_cases(), _wgrad_inputs, wgrad_ref, wgrad_bar, wgrad_stock, wgrad_emulate32),
    "mconv_dgrad": (_dgrad_cases(), _dgrad_inputs, dgrad_ref, dgrad_bar, _f32(dgrad_ref), dgrad_emulate32),
    "grouped_linear": (_linear_cases(), _linear_inputs, linear_ref, linear_bar, _f32(linear_ref), None),
    "grouped_linear_bwd": (_linbwd_cases(), _linbwd_inputs, linbwd_ref, linbwd_bar, _f32(linbwd_ref, D32), None),
    "small_map": (_small_cases(), _small_inputs, small_ref, small_bar, _f32(small_ref), None),
}
CASES = {op: v[0] for op, v in OPS.items()}
# the split-bf16 operations: op -> (emulate, the output the class bar is taken on)
SPLIT_OPS = {"gemm_sb": (gemm_emulate, "c"), "mconv_wgrad": (wgrad_emulate, "dw"), "mconv_dgrad": (dgrad_emulate, None)}

_GEMM_MUT = {"lo*hi dropped": lambda **i: gemm_emulate(drop=(1, 0), **i), "hi*lo dropped": lambda **i: gemm_emulate(drop=(0, 1), **i),
             "K tail not zeroed": _mut(gemm_emulate, "k_tail_not_zeroed"), "last split slice lost": _mut(gemm_emulate, "last_slice_lost"),
             "a row beyond M written": _mut(gemm_emulate, "row_beyond_M_written"), "lda taken as K": _mut(gemm_emulate, "lda_taken_as_K")}
MUTANTS = {
    "mconv_unfold": {"pad off by one": _mut(unfold_ref, "pad_off_by_one"), "parity (ga, gb) swapped": _mut(unfold_ref, "parity_swapped"),
                     "label of the input resolution": _mut(unfold_ref, "label_of_the_input_resolution")},
    "unfold2d": {"pad off by one": _mut(unfold2d_ref, "pad_off_by_one"), "stride ignored": _mut(unfold2d_ref, "stride_ignored")},
    "mconv_scale": {"slope chosen with >=": _mut(scale_ref, "slope_ge"), "noise batch stride 0": _mut(scale_ref, "noise_stride_0"),
                    "parity planes transposed": _mut(scale_ref, "parity_planes_transposed"), "d of the wrong region": _mut(scale_ref, "d_of_the_next_region"),
                    "no-region pixels left out of dbias": _mut(scale_ref, "no_region_left_out_of_dbias"), "the bias not subtracted before q": _mut(scale_ref, "bias_not_subtracted")},
    "mconv_fold": {"region of the input instead of the source position": _mut(fold_direct, "region_of_the_input"),
                   "right neighbour at px + 4 == w read": _mut(fold_direct, "right_neighbour_read"), "left boundary tap kept": _mut(fold_direct, "left_tap_kept"),
                   "parity (ga, gb) swapped": _mut(fold_direct, "parity_swapped"), "last chunk lost": _mut(fold_direct, "last_chunk_lost")},
    "style_tables_bwd": {"factor 2 of s (t wsq^T) missing": _mut(tables_direct, "factor_2_missing"), "wsq read transposed": _mut(tables_direct, "wsq_transposed"),
                         "last quarter-slice lost": _mut(tables_direct, "last_quarter_lost"), "mod_lr on g_mod_w": _mut(tables_direct, "mod_lr_on_g_mod_w")},
    "gemm_sb": _GEMM_MUT,
    "mconv_wgrad": {"lo*hi dropped": lambda **i: wgrad_emulate(drop=(1, 0), **i), "hi*lo dropped": lambda **i: wgrad_emulate(drop=(0, 1), **i),
                    "last split slice lost": _mut(wgrad_emulate, "last_slice_lost"), "parity (ga, gb) swapped": _mut(wgrad_emulate, "parity_swapped"),
                    "pad off by one": _mut(wgrad_emulate, "pad_off_by_one")},
    "mconv_dgrad": {"lo*hi dropped": lambda **i: dgrad_emulate(drop=(1, 0), **i), "hi*lo dropped": lambda **i: dgrad_emulate(drop=(0, 1), **i)},
    "grouped_linear": {"bias_mul missing": _mut(linear_ref, "bias_mul_missing"), "addend before the activation": _mut(linear_ref, "addend_before_act"),
                       "ninth batch row dropped": _mut(linear_ref, "ninth_row_dropped")},
    "grouped_linear_bwd": {"lrelu' taken at >=": _mut(linbwd_ref, "lrelu_ge"), "empty slice not zeroed": _mut(linbwd_ref, "empty_slice_not_zeroed"),
                           "scale applied twice": _mut(linbwd_ref, "scale_twice")},
    "small_map": {"T transposed": _mut(small_ref, "T_transposed")},
}

_BUILT = {}


def case_names(op):
    return [c["name"] for c in CASES[op]]


def case(op, name):
    return next(c for c in CASES[op] if c["name"] == name)


def built(op, name):
    """(inputs, reference64, bar) of a case, computed once and left unchanged."""
    if (op, name) not in _BUILT:
        _, make, ref, bar, _, _ = OPS[op]
        inp = make(case(op, name))
        _BUILT[op, name] = (inp, ref(**inp), bar(**inp))
    return _BUILT[op, name]


_CLASS = {}


def built_class(op, name):
    """(emulation, class bar) of a case of a split-bf16 operation: the bar is one number for ``gemm_sb`` / ``mconv_wgrad`` and one per output for ``mconv_dgrad``."""
    if (op, name) not in _CLASS:
        inp, ref, _ = built(op, name)
        emu, key = SPLIT_OPS[op]
        full = emu(**inp)
        errs = [emu(drop=pr, **inp) for pr in PRODUCTS]
        bar = {k: 0.5 * min(np.abs(descaled(e[k], inp) - descaled(ref[k], inp)).max() for e in errs) for k in full}
        _CLASS[op, name] = (full, bar)
    return _CLASS[op, name]
