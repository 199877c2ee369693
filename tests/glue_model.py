"""A plain CPU model of the streaming kernels between the convolutions (csrc/norm.hip, and ``gate_add_up_kernel`` / ``tensor2im_kernel`` of csrc/parser.hip):
for every operation the float64 reference written from the reference project's definition (``reference64``), a bound computed from the reference's own
magnitudes and the number of float32 roundings on the kernel's longest path (``bar``), single-change mutants of the reference (``MUTANTS``), the stock
float32 PyTorch form (``stock32``), a float32 emulation of the kernel's own summation tree (``emulate32``) and the case tables (``CASES``): the smallest
shapes that reach each guard of the kernels.  No GPU and no library import.

An operation's inputs are a dict of numpy arrays and scalars (``inputs(op, case)``); every function returns a dict of output arrays.  Conventions of the bars
(U = 2^-24, one float32 rounding):
  reductions   D U sum|terms| (over the count for a mean), D = roundings on the longest path of that kernel's tree at that shape, stored in the case table
               beside the shape and checked against ``depth`` (the count read from the code);
  rstd         relative: half the relative error of var + eps (D + 3 roundings: the tree with its division, a term's subtraction and square, the addition
               of eps; the second-order shift by the mean's error) + 2 U for ``sqrtf`` (one ulp) + U for the reciprocal;
  element-wise roundings on the element's path x U x sum|terms added|;
  uint8 / exact outputs   bar 0: equality."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

U = 2.0 ** -24
SEED = 61
MAX_REGIONS = 16
f32, f64 = np.float32, np.float64


def arr(key, shape, mean=0.0, std=1.0):
    return seeded.seeded_array(SEED, key, tuple(shape), float(mean), float(std), "normal").astype(f32)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ summation trees
def depth(kind, n):
    """Roundings on the longest path of a kernel's sum of ``n`` terms, division by the count included (csrc/norm.hip).
    ``block``: plane_stats_kernel / norm_gate_add_stats_kernel — 256 threads; a thread adds one float4 group ((a + b) + (c + d), 2 roundings) per round of 1024
    elements (``hw % 4 == 0``; one element per round of 256 otherwise), the wave butterfly 6, ``sh[0] + sh[1] + sh[2] + sh[3]`` 3, the division 1.
    ``wave``: norm_self_wave_kernel — one wave, rounds of 256, no cross-wave step.  ``big``: norm_self_stats_big_kernel — 1024 threads, rounds of 4096, 16 partial sums
    added to 0 one after the other.  ``dot``: vec_fc_kernel / se_gate_kernel — a lane's ``a += w x`` every 64 inputs (product and sum: one rounding more than the steps), the butterfly."""
    if kind == "block":
        return (cdiv(n, 1024) + 2 if n % 4 == 0 else cdiv(n, 256)) + 6 + 3 + 1
    if kind == "wave":
        return cdiv(n, 256) + 2 + 6 + 1
    if kind == "big":
        return cdiv(n, 4096) + 2 + 6 + 16 + 1
    if kind == "dot":
        return cdiv(n, 64) + 1 + 6
    if kind == "pool":            # masked_avg_pool_kernel: a lane adds one element (or an exact 0) every 64, the butterfly, the division
        return cdiv(n, 64) + 6 + 1
    raise KeyError(kind)


def stats_kind(hw, self_form=False):
    """Which tree the statistics of a plane come from (the dispatch of e4s_norm_self_gate_add_stats / e4s_norm_gate_add_stats / the plane_stats fall-back)."""
    if self_form and hw % 4 == 0:
        return "wave" if hw <= 1024 else ("block" if hw <= 16384 else "big")
    return "block"


def tree_sum32(v, kind="block"):
    """The float32 sum of the 1-D float32 array ``v`` in the order of the kernel's tree (``depth``)."""
    v = np.asarray(v, f32)
    n = v.size
    threads = {"block": 256, "wave": 64, "big": 1024}[kind]
    if n % 4 == 0:
        rounds = cdiv(n, 4 * threads)
        p = np.zeros(rounds * threads * 4, f32)          # (an absent group adds an exact 0)
        p[:n] = v
        p = p.reshape(rounds, threads, 4)
        g = (p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])
    else:
        rounds = cdiv(n, threads)
        p = np.zeros(rounds * threads, f32)
        p[:n] = v
        g = p.reshape(rounds, threads)
    s = np.zeros(threads, f32)
    for r in range(rounds):
        s = s + g[r]
    s = s.reshape(-1, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    t = f32(0.0) if kind == "big" else None
    for k in range(s.shape[0]):
        t = s[k, 0] if t is None else f32(t + s[k, 0])
    return f32(t)


def _stats32(p, eps, kind, nmean=False):
    """(mean, rstd[, nmean]) of one plane in float32 through the kernel's tree: two passes, biased variance."""
    p = np.asarray(p, f32).ravel()
    n = f32(p.size)
    m = f32(tree_sum32(p, kind) / n)
    a = (p - m).astype(f32)
    var = f32(tree_sum32((a * a).astype(f32), kind) / n)
    r = f32(f32(1.0) / f32(np.sqrt(f64(f32(var + f32(eps))))))
    if nmean:
        return m, r, f32(f32(tree_sum32(a, kind) * r) / n)
    return m, r


def _rstd_rel(D, var, eps, dmean):
    return 0.5 * ((D + 3) * U * var + dmean ** 2) / (var + eps) + 3 * U


def _plane_bars(o, D, eps, elbar=None):
    """Bars of (mean, rstd) of the planes ``o`` [bs, C, h, w] (float64) when the kernel's own elements lie within ``elbar`` of them."""
    hw = o.shape[2] * o.shape[3]
    bm = D * U * np.abs(o).sum((2, 3)) / hw
    var = o.var((2, 3))
    dv = 0.0
    if elbar is not None:
        bm = bm + elbar.mean((2, 3))
        dv = 2 * np.sqrt(var) * np.sqrt((elbar ** 2).mean((2, 3))) + (elbar ** 2).mean((2, 3))
    rel = _rstd_rel(D, var, eps, bm) + 0.5 * dv / (var + eps)
    return bm, rel / np.sqrt(var + eps)


def _planted(x, const_plane=True):
    """Large values in the last element and in the first element of the last partial round of every plane, so that a lost element cannot hide inside the bar of a
    large plane; the last plane of the batch constant (where ``eps`` decides)."""
    bs, C, h, w = x.shape
    hw = h * w
    flat = x.reshape(bs * C, hw)
    step = 1024 if hw % 4 == 0 else 256
    first = step * ((hw - 1) // step)
    flat[:, hw - 1] = 400.0
    if first != hw - 1:
        flat[:, first] = -300.0
    if const_plane:
        flat[-1, :] = 3.1
    return x


# ================================================================================================ plane_stats
PLANE_SHAPES = [((2, 3, 7, 7), 11), ((1, 2, 17, 31), 13), ((2, 3, 2, 2), 13), ((1, 5, 30, 34), 13), ((1, 3, 4, 257), 14), ((1, 2, 50, 82), 17),
                ((1, 2, 264, 256), 78)]
PLANE_MODES = ("mean", "stats", "nmean")


def _plane_cases():
    return [dict(name=f"{'x'.join(map(str, s))}.{m}", shape=s, D=D, mode=m) for s, D in PLANE_SHAPES for m in PLANE_MODES]


def _plane_inputs(c):
    s = c["shape"]
    assert c["D"] == depth("block", s[2] * s[3]), c
    x = _planted(arr("ps" + c["name"].split(".")[0], s, 6.0, 2.0))
    return dict(x=x, eps=1e-5, mode=c["mode"], D=c["D"], emitted=None)


def plane_stats_ref(x, eps, mode, D=None, emitted=None, lose=None, ddof=0, eps_outside=False, nmean_no_rstd=False):
    """mean [bs, C]; 'stats': + rstd = 1 / sqrt(biased var + eps); 'nmean': + the mean of the plane normalised with the EMITTED float32 (mean, rstd)
    (``emitted``; those two have bars of their own) — what the SE squeeze sees: (mean64 - mean_emitted) * rstd_emitted."""
    xd = x.astype(f64)
    bs, C, h, w = xd.shape
    hw = h * w
    flat = xd.reshape(bs, C, hw)
    keep = np.ones(hw, bool)
    if lose == "last":
        keep[hw - 1] = False
    if lose == "round":
        step = 1024 if hw % 4 == 0 else 256
        keep[step * ((hw - 1) // step):] = False
    m = (flat * keep).sum(2) / hw
    out = {"mean": m}
    if mode == "mean":
        return out
    var = (((flat - m[:, :, None]) ** 2) * keep).sum(2) / (hw - ddof)
    out["rstd"] = 1.0 / (np.sqrt(var) + eps) if eps_outside else 1.0 / np.sqrt(var + eps)
    if mode == "nmean":
        me, re_ = (m.astype(f32), out["rstd"].astype(f32)) if emitted is None else emitted
        out["nmean"] = (flat.mean(2) - me.astype(f64)) * (1.0 if nmean_no_rstd else re_.astype(f64))
    return out


def plane_stats_bar(x, eps, mode, D, emitted=None):
    xd = x.astype(f64)
    bm, br = _plane_bars(xd, D, eps)
    out = {"mean": bm}
    if mode != "mean":
        out["rstd"] = br
    if mode == "nmean":
        # sum of (x - mean_e): D roundings of the tree and the division + the subtraction + the product with rstd; |x - mean_e| <= |x - mean64| + bar(mean)
        r = 1.0 / np.sqrt(xd.var((2, 3)) + eps)
        spread = np.abs(xd - xd.mean((2, 3), keepdims=True)).mean((2, 3)) + bm
        out["nmean"] = (D + 2) * U * spread * (r + br)
    return out


def plane_stats_emulate(x, eps, mode, **_):
    bs, C = x.shape[:2]
    res = [_stats32(x[b, c], eps, "block", True) for b in range(bs) for c in range(C)]
    out = {"mean": np.array([r[0] for r in res], f32).reshape(bs, C)}
    if mode != "mean":
        out["rstd"] = np.array([r[1] for r in res], f32).reshape(bs, C)
    if mode == "nmean":
        out["nmean"] = np.array([r[2] for r in res], f32).reshape(bs, C)
    return out


def plane_stats_stock(x, eps, mode, **_):
    t = torch.from_numpy(x)
    m = t.mean((2, 3))
    out = {"mean": m.numpy()}
    if mode != "mean":
        r = 1.0 / torch.sqrt(t.var((2, 3), unbiased=False) + eps)
        out["rstd"] = r.numpy()
        if mode == "nmean":
            out["nmean"] = ((t - m[:, :, None, None]) * r[:, :, None, None]).mean((2, 3)).numpy()
    return out


# ================================================================================================ vec_fc
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 3
FC_SHAPES = [((1, 1, 1), 8), ((3, 63, 5), 8), ((2, 64, 4), 8), ((2, 130, 7), 10), ((1, 512, 19), 15)]


def _fc_cases():
    return [dict(name=f"{'x'.join(map(str, s))}.{'bn' if bn else 'plain'}.act{a}", shape=s, D=D, bn=bn, act=a)
            for s, D in FC_SHAPES for bn in (False, True) for a in (ACT_NONE, ACT_RELU, ACT_SIGMOID)]


def seeded_bn(key, c):
    """(gamma, beta, running_mean, running_var, eps): the variance from 1e-6 (its first entry) to about 2, some gammas negative (the last one always)."""
    var = np.exp(arr(key + "v", (c,)) * 3.0 - 4.0).clip(1e-6, 2.0).astype(f32)
    var[0] = 1e-6
    gamma = arr(key + "g", (c,), 0.3, 1.0)
    gamma[-1] = -abs(gamma[-1]) - 0.25
    return gamma, arr(key + "b", (c,), 0.0, 0.5), arr(key + "m", (c,), 0.0, 0.3), var, 1e-5


def _fc_inputs(c):
    bs, cin, cout = c["shape"]
    assert c["D"] == depth("dot", cin), c
    key = f"fc{cin}.{cout}"
    return dict(x=arr(key + "x", (bs, cin), 0.5, 1.0), w=arr(key + "w", (cout, cin), 0.0, cin ** -0.5), bn=seeded_bn(key, cout) if c["bn"] else None,
                act=c["act"], D=c["D"])


def _sigmoid(a, sign=-1.0):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(sign * a))


def vec_fc_ref(x, w, bn, act, D=None, lose_tail=False, bn_after_act=False, eps_outside=False, no_beta=False, sig_plus=False):
    xd, wd = x.astype(f64), w.astype(f64)
    cin = xd.shape[1]
    if lose_tail:
        xd = xd.copy()
        xd[:, 64 * (cin // 64):] = 0
    a = xd @ wd.T

    def norm(v):
        if bn is None:
            return v
        gamma, beta, mean, var, eps = (np.asarray(t, f64) for t in bn)
        s = gamma / (np.sqrt(var) + eps if eps_outside else np.sqrt(var + eps))
        return (v - mean) * s + (0.0 if no_beta else beta)

    def activate(v):
        return np.maximum(v, 0) if act == ACT_RELU else (_sigmoid(v, 1.0 if sig_plus else -1.0) if act == ACT_SIGMOID else v)

    return {"y": norm(activate(a)) if bn_after_act else activate(norm(a))}


def _sigmoid_bar(pre_bar, y):
    """|d sigmoid| <= 1/4 |d a|; ``expf`` one ulp (2 U) on e with dy/y = (1 - y) de/e, the addition and the reciprocal one rounding each; nothing
    below the smallest normal float32 (``expf`` overflows past 88.7 and the quotient is 0)."""
    return 0.25 * pre_bar + 4 * U * y + 2.0 ** -126


def vec_fc_bar(x, w, bn, act, D):
    xd, wd = x.astype(f64), w.astype(f64)
    a = xd @ wd.T
    bar = D * U * (np.abs(xd) @ np.abs(wd).T)
    if bn is not None:
        gamma, beta, mean, var, eps = (np.asarray(t, f64) for t in bn)
        s = gamma / np.sqrt(var + eps)
        # a - mean 1; s: the addition 1, sqrtf 2, the division 1; the product 1; + beta 1
        bar = bar * np.abs(s) + 7 * U * (np.abs((a - mean) * s) + np.abs(beta))
        a = (a - mean) * s + beta
    if act == ACT_SIGMOID:
        bar = _sigmoid_bar(bar, _sigmoid(a))
    return {"y": bar}


def _dot32(x, w):
    """[bs, cout] float32 dot products in vec_fc_kernel's order: lane l adds w[i] x[i] for i = l, l + 64, ...; then the wave butterfly."""
    bs, cin = x.shape
    rounds = cdiv(cin, 64)
    xp = np.zeros((bs, rounds * 64), f32)
    xp[:, :cin] = x
    wp = np.zeros((w.shape[0], rounds * 64), f32)
    wp[:, :cin] = w
    s = np.zeros((bs, w.shape[0], 64), f32)
    for r in range(rounds):
        s = s + (xp[:, None, r * 64:(r + 1) * 64] * wp[None, :, r * 64:(r + 1) * 64]).astype(f32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ o]
    return s[:, :, 0]


def _act32(a, act):
    if act == ACT_RELU:
        return np.maximum(a, f32(0))
    if act == ACT_SIGMOID:
        with np.errstate(over="ignore"):
            return (f32(1) / (f32(1) + np.exp(-a).astype(f32))).astype(f32)
    return a


def vec_fc_emulate(x, w, bn, act, **_):
    a = _dot32(x, w)
    if bn is not None:
        gamma, beta, mean, var, eps = bn
        a = ((a - mean) * (gamma / np.sqrt((var + f32(eps)).astype(f64)).astype(f32)).astype(f32) + beta).astype(f32)
    return {"y": _act32(a, act)}


def vec_fc_stock(x, w, bn, act, **_):
    y = F.linear(torch.from_numpy(x), torch.from_numpy(w))
    if bn is not None:
        gamma, beta, mean, var, eps = bn
        y = F.batch_norm(y, torch.from_numpy(mean), torch.from_numpy(var), torch.from_numpy(gamma), torch.from_numpy(beta), False, 0.0, eps)
    y = F.relu(y) if act == ACT_RELU else (torch.sigmoid(y) if act == ACT_SIGMOID else y)
    return {"y": y.numpy()}


# ================================================================================================ se_gate
SE_SHAPES = [((1, 16, 1), 8, 8), ((2, 130, 8), 10, 8), ((3, 512, 32), 15, 8), ((2, 96, 33), 9, 8), ((2, 70, 40), 9, 8), ((1, 64, 64), 8, 8)]


def _se_cases():
    return [dict(name="x".join(map(str, s)), shape=s, D=D1, D2=D2) for s, D1, D2 in SE_SHAPES]


def _se_inputs(c):
    bs, C, H = c["shape"]
    assert c["D"] == depth("dot", C) and c["D2"] == depth("dot", H), c
    key = f"se{C}.{H}"
    return dict(pooled=arr(key + "p", (bs, C), 0.3, 1.0), w1=arr(key + "a", (H, C), 0.0, C ** -0.5), w2=arr(key + "b", (C, H), 0.0, 2.0 * H ** -0.5),
                D=c["D"], D2=c["D2"])


def se_gate_ref(pooled, w1, w2, D=None, D2=None, lose_hidden=False, no_relu=False, lose_outputs=False):
    p, a, b = pooled.astype(f64), w1.astype(f64), w2.astype(f64)
    hid = p @ a.T
    if not no_relu:
        hid = np.maximum(hid, 0)
    if lose_hidden:
        hid[:, 32:] = 0
    g = _sigmoid(hid @ b.T)
    if lose_outputs:
        g[:, 64 * (g.shape[1] // 64):] = 0
    return {"gate": g}


def se_gate_bar(pooled, w1, w2, D, D2):
    p, a, b = pooled.astype(f64), w1.astype(f64), w2.astype(f64)
    hid = np.maximum(p @ a.T, 0)
    hbar = D * U * (np.abs(p) @ np.abs(a).T)
    t = hid @ b.T
    tbar = hbar @ np.abs(b).T + D2 * U * (hid @ np.abs(b).T)
    return {"gate": _sigmoid_bar(tbar, _sigmoid(t))}


def se_gate_emulate(pooled, w1, w2, **_):
    hid = np.maximum(_dot32(pooled, w1), f32(0))
    return {"gate": _act32(_dot32(hid, w2), ACT_SIGMOID)}


def se_gate_stock(pooled, w1, w2, **_):
    p, a, b = (torch.from_numpy(t) for t in (pooled, w1, w2))
    return {"gate": torch.sigmoid(F.linear(F.relu(F.linear(p, a)), b)).numpy()}


# ================================================================================================ norm_gate_add (three forms)
def _nga_case(form, bs, C, h, w, D, ss=0, sc_stats=False, prelu=False, gate=True, norm=True):
    """``ss`` 0 = no shortcut; ``norm``: (mean, rstd) given (non-fused / stats forms; the self form computes them)."""
    name = f"{bs}x{C}x{h}x{w}.ss{ss}" + (".scn" if sc_stats else "") + (".prelu" if prelu else "") + ("" if gate else ".nogate") + ("" if norm else ".nonorm")
    return dict(name=name, form=form, shape=(bs, C, h, w), D=D, ss=ss, sc_stats=sc_stats, prelu=prelu, gate=gate, norm=norm)


NGA_PLAIN = [
    _nga_case("plain", 2, 3, 7, 7, 0, ss=2, norm=False),                      # the ID loss's call: 7 x 7 maps, stride-2 shortcut of 14 x 14, scalar path
    _nga_case("plain", 2, 2, 5, 3, 0, ss=1, sc_stats=True, prelu=True),       # everything on
    _nga_case("plain", 1, 3, 30, 34, 0, ss=2, sc_stats=True, prelu=True),
    _nga_case("plain", 1, 2, 264, 256, 0, gate=False),                        # 67 584 pixels: the grid-stride loop wraps
    _nga_case("plain", 2, 2, 6, 10, 0, ss=2, sc_stats=True, prelu=True),      # (added: a per-plane / per-channel slope mix-up needs two images AND a strided shortcut's mutants a PReLU)
]
NGA_STATS = [
    _nga_case("stats", 5, 1, 2, 2, 13, ss=1, sc_stats=True, prelu=True),
    _nga_case("stats", 1, 5, 30, 34, 13, ss=2, prelu=True),
    _nga_case("stats", 5, 1, 32, 32, 13),
    _nga_case("stats", 1, 5, 4, 257, 14, ss=2, sc_stats=True, prelu=True),
    _nga_case("stats", 5, 1, 36, 36, 14, ss=1),
    _nga_case("stats", 1, 5, 64, 64, 16, ss=2, sc_stats=True, prelu=True),
    _nga_case("stats", 5, 1, 50, 82, 17, ss=1, sc_stats=True, prelu=True),
    _nga_case("stats", 1, 5, 128, 128, 28, ss=2, prelu=True),
    _nga_case("stats", 5, 1, 6, 10, 13, ss=2, sc_stats=True, prelu=True),     # (added: the slope mix-up with a strided shortcut in one small case)
]
_SELF_SIZES = [(2, 2, 10, 0), (30, 34, 13, 0), (32, 32, 13, 0), (4, 257, 14, 1), (36, 36, 14, 1), (64, 64, 16, 1), (50, 82, 17, 1), (128, 128, 28, 1)]
NGA_SELF = []
for _h, _w, _D, _over in _SELF_SIZES:
    # bs C = 1, 5 (five images of one channel: a slope taken by plane is wrong), 8 (two images of four)
    NGA_SELF += [_nga_case("self", 1, 1, _h, _w, _D, ss=1, sc_stats=True, prelu=True, norm=False),
                 _nga_case("self", 5, 1, _h, _w, _D, ss=2, sc_stats=True, prelu=True, norm=False),
                 _nga_case("self", 2, 4, _h, _w, _D, ss=1 if _over else 0, prelu=bool(_over), norm=False)]
NGA_SELF += [_nga_case("self", 2, 2, 241, 68, 30, prelu=True, norm=False), _nga_case("self", 1, 2, 200, 180, 34, prelu=True, norm=False),
             _nga_case("self", 1, 2, 256, 256, 41, prelu=True, norm=False)]
STATS_EPS, SELF_EPS = 1e-5, 1e-3


def _nga_inputs(c):
    bs, C, h, w = c["shape"]
    form, ss = c["form"], c["ss"]
    key = "nga" + c["name"] + form
    hw = h * w
    if form != "plain":
        assert c["D"] == depth(stats_kind(hw, form == "self"), hw), c
    x = arr(key + "x", (bs, C, h, w), 6.0, 2.0)
    if hw >= 1020:
        _planted(x, const_plane=False)
    d = dict(x=x, mean=None, rstd=None, gate=None, shortcut=None, sc_stats=None, ss=max(ss, 1), prelu=None, stats_eps=None, self_eps=None, D=c["D"])
    if c["norm"]:
        st = plane_stats_ref(x, 1e-5, "stats")
        d["mean"], d["rstd"] = st["mean"].astype(f32), st["rstd"].astype(f32)
    if c["gate"]:
        d["gate"] = (0.3 + 0.11 * np.arange(bs * C)).astype(f32).reshape(bs, C)          # distinct per plane
    if ss:
        sc = arr(key + "s", (bs, C, h * ss, w * ss), -4.0, 1.5)
        d["shortcut"] = sc
        if c["sc_stats"]:
            st = plane_stats_ref(sc, 1e-5, "stats")
            d["sc_stats"] = (st["mean"].astype(f32), st["rstd"].astype(f32))
    if c["prelu"]:
        d["prelu"] = (0.05 + 0.17 * np.arange(C)).astype(f32)                           # distinct per channel
    if form in ("stats", "self"):
        d["stats_eps"] = STATS_EPS
    if form == "self":
        d["self_eps"] = SELF_EPS
    return d


def _bc(v):
    return np.asarray(v, f64)[:, :, None, None]


def nga_ref(x, mean, rstd, gate, shortcut, sc_stats, ss, prelu, stats_eps, self_eps, D=None, mutant=None):
    """``prelu((x - mean) * rstd * gate + (shortcut[::ss, ::ss] - sc_mean) * sc_rstd)`` in float64; ``self_eps``: (mean, rstd) are the plane's own;
    ``stats_eps``: + the InstanceNorm statistics of the result."""
    xd = x.astype(f64)
    bs, C, h, w = xd.shape
    if self_eps is not None:
        e = stats_eps if mutant == "eps_swapped" else self_eps
        m, r = xd.mean((2, 3), keepdims=True), 1.0 / np.sqrt(xd.var((2, 3), keepdims=True) + e)
    else:
        m, r = (_bc(mean), _bc(rstd)) if mean is not None else (0.0, 1.0)
    g = _bc(gate) if gate is not None else 1.0
    A = (xd - m) * r
    B = None
    if shortcut is not None:
        sd = shortcut.astype(f64)
        if mutant == "sc_offset_row" and ss > 1:
            s = sd[:, :, 1::ss, ::ss]
        elif mutant == "sc_avg" and ss > 1:
            s = sd.reshape(bs, C, h, ss, w, ss).mean((3, 5))
        elif mutant == "sc_row_stride" and ss > 1:              # row stride w instead of w ss: flat index y ss w + x ss of the plane
            flat = sd.reshape(bs, C, -1)
            idx = (np.arange(h)[:, None] * ss * w + np.arange(w)[None, :] * ss).ravel()
            s = flat[:, :, idx].reshape(bs, C, h, w)
        else:
            s = sd[:, :, ::ss, ::ss]
        if mutant == "sc_x_stats":
            B = (s - m) * r
        elif sc_stats is not None:
            B = (s - _bc(sc_stats[0])) * _bc(sc_stats[1])
        else:
            B = s
    if mutant == "gate_after_shortcut":
        t = (A + (B if B is not None else 0.0)) * g
    else:
        t = A * g + (B if B is not None else 0.0)
    pre = t
    if prelu is not None:
        sl = np.asarray(prelu, f64)
        slope = np.broadcast_to(sl[None, :], (bs, C)).copy()
        if mutant == "slope_by_plane":                          # prelu[plane]: right for the first image only; past the vector's end whatever lies there
            pl = np.arange(bs * C)
            slope = np.where(pl < C, sl[np.minimum(pl, C - 1)], 2.0 * sl[pl % C] + 0.1).reshape(bs, C)
        slope = slope[:, :, None, None]
        if mutant == "prelu_norm_only":
            a2 = A * g
            t = np.where(a2 > 0, a2, a2 * slope) + (B if B is not None else 0.0)
        else:
            t = np.where(t > 0, t, t * slope)
    out = {"out": t}
    if stats_eps is not None:
        o = pre if mutant == "stats_before_prelu" else t
        e = self_eps if (mutant == "eps_swapped" and self_eps is not None) else stats_eps
        out["omean"] = o.mean((2, 3))
        out["orstd"] = 1.0 / np.sqrt(o.var((2, 3)) + e)
    return out


def nga_bar(x, mean, rstd, gate, shortcut, sc_stats, ss, prelu, stats_eps, self_eps, D):
    xd = x.astype(f64)
    bs, C, h, w = xd.shape
    extra = 0.0
    g = np.abs(_bc(gate)) if gate is not None else 1.0
    if self_eps is not None:
        m, var = xd.mean((2, 3), keepdims=True), xd.var((2, 3), keepdims=True)
        r = 1.0 / np.sqrt(var + self_eps)
        bm, br = _plane_bars(xd, D, self_eps)
        extra = (bm[:, :, None, None] * r + np.abs(xd - m) * br[:, :, None, None]) * g          # |dm r g| + |(x - m) dr g|
    else:
        m, r = (_bc(mean), _bc(rstd)) if mean is not None else (0.0, 1.0)
    A = np.abs((xd - m) * r) * g
    B = 0.0
    if shortcut is not None:
        s = shortcut.astype(f64)[:, :, ::ss, ::ss]
        B = np.abs((s - _bc(sc_stats[0])) * _bc(sc_stats[1])) if sc_stats is not None else np.abs(s)
    slope = 1.0
    if prelu is not None:
        slope = np.maximum(1.0, np.abs(np.asarray(prelu, f64)))[None, :, None, None]
    # x - m, * r, * g | s - sm, * sr (the longer branch: 3), the sum, the slope: 5 <= 6
    el = (6 * U * (A + B) + extra) * slope
    out = {"out": el}
    if stats_eps is not None:
        ref = nga_ref(x, mean, rstd, gate, shortcut, sc_stats, ss, prelu, stats_eps, self_eps)["out"]
        out["omean"], out["orstd"] = _plane_bars(ref, D, stats_eps, np.broadcast_to(el, ref.shape))
    return out


def nga_emulate(x, mean, rstd, gate, shortcut, sc_stats, ss, prelu, stats_eps, self_eps, D=None):
    """The three kernels' float32 arithmetic, the statistics through their own trees."""
    bs, C, h, w = x.shape
    kind = stats_kind(h * w, self_eps is not None)
    one, zero = f32(1), f32(0)
    out = np.empty_like(x)
    om, orr = np.empty((bs, C), f32), np.empty((bs, C), f32)
    for b in range(bs):
        for c in range(C):
            p = x[b, c]
            if self_eps is not None:
                m, r = _stats32(p, self_eps, kind)
            else:
                m, r = (mean[b, c], rstd[b, c]) if mean is not None else (zero, one)
            t = ((p - m).astype(f32) * r).astype(f32) * (gate[b, c] if gate is not None else one)
            if shortcut is not None:
                s = shortcut[b, c, ::ss, ::ss]
                sm, sr = (sc_stats[0][b, c], sc_stats[1][b, c]) if sc_stats is not None else (zero, one)
                t = (t + ((s - sm).astype(f32) * sr).astype(f32)).astype(f32)
            t = np.where(t > 0, t, (t * (prelu[c] if prelu is not None else one)).astype(f32)).astype(f32)
            out[b, c] = t
            if stats_eps is not None:
                om[b, c], orr[b, c] = _stats32(t, stats_eps, kind)
    res = {"out": out}
    if stats_eps is not None:
        res["omean"], res["orstd"] = om, orr
    return res


def nga_stock(x, mean, rstd, gate, shortcut, sc_stats, ss, prelu, stats_eps, self_eps, D=None):
    t = torch.from_numpy(x)
    bc = lambda v: torch.from_numpy(np.asarray(v, f32))[:, :, None, None]      # noqa: E731
    if self_eps is not None:
        t = F.instance_norm(t, eps=self_eps)
    elif mean is not None:
        t = (t - bc(mean)) * bc(rstd)
    if gate is not None:
        t = t * bc(gate)
    if shortcut is not None:
        s = F.max_pool2d(torch.from_numpy(shortcut), 1, ss)
        if sc_stats is not None:
            s = (s - bc(sc_stats[0])) * bc(sc_stats[1])
        t = t + s
    if prelu is not None:
        t = F.prelu(t, torch.from_numpy(prelu))
    out = {"out": t.numpy()}
    if stats_eps is not None:
        out["omean"] = t.mean((2, 3)).numpy()
        out["orstd"] = (1.0 / torch.sqrt(t.var((2, 3), unbiased=False) + stats_eps)).numpy()
    return out


_NGA_COMMON = ["gate_after_shortcut", "sc_x_stats", "sc_offset_row", "sc_avg", "sc_row_stride", "slope_by_plane", "prelu_norm_only"]


def _nga_mutants(names):
    return {n: (lambda n: lambda **kw: nga_ref(mutant=n, **kw))(n) for n in names}


# ================================================================================================ masked_avg_pool
POOL_SHAPES = [((2, 20, 16, 16, 64, 64, 12), 11), ((2, 5, 16, 12, 50, 37, 12), 10), ((1, 3, 7, 9, 7, 9, 1), 8), ((1, 6, 13, 5, 26, 10, 7), 9),
               ((1, 2, 64, 64, 512, 512, 12), 71)]


def _pool_cases():
    return [dict(name="x".join(map(str, s)), shape=s, D=D) for s, D in POOL_SHAPES]


def _pool_inputs(c):
    bs, C, h, w, lh, lw, nreg = c["shape"]
    assert c["D"] == depth("pool", h * w), c
    key = "mp" + c["name"]
    u = (arr(key + "l", (bs, lh, lw)) * 0.2887 + 0.5).clip(0, 0.999)       # ~uniform in [0, 1)
    hi = MAX_REGIONS if nreg == 7 else nreg                                 # the nreg = 7 case carries labels in [7, 16) as well
    # blocks of labels of the size of one feature pixel's footprint and smaller, so that floor and round pick different labels
    by, bx = max(1, lh // (2 * h) + 1), max(1, lw // (2 * w) + 1)
    coarse = u[:, ::by, ::bx]
    lab = np.repeat(np.repeat((coarse * hi).astype(np.uint8), by, 1), bx, 2)[:, :lh, :lw].copy()
    if nreg > 1:
        lab[lab == 3] = 4                                                   # region 3 is empty
    v = arr(key + "m", (bs, lh, lw))
    lab[v > 1.3] = 255                                                      # about a tenth of the pixels belong to no region
    return dict(feats=arr(key + "f", (bs, C, h, w), 3.0, 1.0), labels=lab, nreg=nreg, D=c["D"])


def nearest_index(n_out, n_in, rounding=False):
    """ATen's nearest source index in float32: ``min(floor(dst * (in / out)), in - 1)`` (``nearest_src``, common.h)."""
    scale = f32(f32(n_in) / f32(n_out))
    t = (np.arange(n_out).astype(f32) * scale).astype(f32)
    if rounding:
        t = (t + f32(0.5)).astype(f32)
    return np.minimum(np.floor(t).astype(np.int64), n_in - 1)


def pool_ref(feats, labels, nreg, D=None, mutant=None):
    fd = feats.astype(f64)
    bs, C, h, w = fd.shape
    lh, lw = labels.shape[1:]
    iy, ix = nearest_index(h, lh, mutant == "round"), nearest_index(w, lw, mutant == "round")
    lab = labels[:, iy][:, :, ix].astype(np.int64)
    if mutant == "none_is_zero":
        lab = np.where(lab == 255, 0, lab)
    if mutant == "fold":
        lab = np.where((lab >= nreg) & (lab != 255), nreg - 1, lab)
    out = np.zeros((bs, nreg, C), f64)
    for r in range(nreg):
        sel = (lab == r)[:, None].astype(f64)
        n = sel.sum((2, 3))
        s = (fd * sel).sum((2, 3))
        with np.errstate(invalid="ignore", divide="ignore"):
            if mutant == "div_hw":
                out[:, r] = s / (h * w)
            elif mutant == "empty_nan":
                out[:, r] = s / n
            else:
                out[:, r] = np.where(n > 0, s / np.maximum(n, 1), 0.0)
    return {"out": out}


def pool_bar(feats, labels, nreg, D):
    ref = pool_ref(np.abs(feats), labels, nreg)["out"]
    return {"out": D * U * ref}


def pool_emulate(feats, labels, nreg, **_):
    """masked_avg_pool_kernel: lane l adds element l, l + 64, ... (or an exact 0), the butterfly, the division by the ballot count."""
    bs, C, h, w = feats.shape
    hw = h * w
    lh, lw = labels.shape[1:]
    lab = labels[:, nearest_index(h, lh)][:, :, nearest_index(w, lw)].reshape(bs, hw)
    rounds = cdiv(hw, 64)
    out = np.zeros((bs, nreg, C), f32)
    lanes = np.arange(64)
    for b in range(bs):
        lp = np.full(rounds * 64, 255, np.int64)
        lp[:hw] = lab[b]
        fp = np.zeros((C, rounds * 64), f32)
        fp[:, :hw] = feats[b].reshape(C, hw)
        for r in range(nreg):
            sel = lp == r
            g = np.where(sel[None], fp, f32(0)).reshape(C, rounds, 64)
            s = np.zeros((C, 64), f32)
            for k in range(rounds):
                s = s + g[:, k]
            for o in (32, 16, 8, 4, 2, 1):
                s = s + s[:, lanes ^ o]
            n = int(sel.sum())
            out[b, r] = s[:, 0] / f32(n) if n else 0
    return {"out": out}


def pool_stock(feats, labels, nreg, **_):
    f = torch.from_numpy(feats)
    bs, C, h, w = f.shape
    lab = F.interpolate(torch.from_numpy(labels)[:, None].float(), size=(h, w), mode="nearest")
    out = torch.zeros(bs, nreg, C)
    for r in range(nreg):
        sel = (lab == r).float()
        n = sel.sum((2, 3))
        out[:, r] = torch.where(n > 0, (f * sel).sum((2, 3)) / n.clamp(min=1), torch.zeros(()))
    return {"out": out.numpy()}


# ================================================================================================ bilinear_resize
BILINEAR = [((1, 1), (5, 7), None), ((5, 7), (1, 1), None), ((3, 300), (3, 130), None), ((9, 6), (36, 24), False), ((9, 6), (20, 17), False),
            ((64, 48), (64, 48), None)]


def _bil_cases():
    out = []
    for i, o, only in BILINEAR:
        for align in ((False, True) if only is None else (only,)):
            out.append(dict(name=f"{i[0]}x{i[1]}to{o[0]}x{o[1]}.{'align' if align else 'half'}", insize=i, size=o, align=align, exact=i == o))
    return out


def _bil_inputs(c):
    return dict(x=arr("bl" + c["name"], (2, 2) + c["insize"], 6.0, 2.0), size=c["size"], align=c["align"], exact=c["exact"])


def bilinear_coord(n_out, n_in, align, clamp_neg=True, clamp_i1=True):
    """(i0, i1, l1) along one axis as ``bilinear_coord`` (common.h) forms them in float32: the scale a float32 quotient, ``src`` one rounding of
    ``dst * scale`` (align_corners) or of ``(dst + 0.5) * scale - 0.5`` (one fused multiply-add), clamped at 0; ``l1 = src - i0`` is exact."""
    dst = np.arange(n_out).astype(f64)
    if align:
        scale = f64(f32(f64(n_in - 1) / f64(n_out - 1))) if n_out > 1 else 0.0
        src = (dst * scale).astype(f32)
    else:
        scale = f64(f32(f64(n_in) / f64(n_out)))
        src = ((dst + 0.5) * scale - 0.5).astype(f32)         # exact in float64 (24 x 24 bits, then a shift by 0.5), rounded once: the fma
        if clamp_neg:
            src = np.maximum(src, f32(0))
    i0 = np.minimum(np.trunc(src).astype(np.int64), n_in - 1)
    i1 = i0 + ((i0 < n_in - 1) if clamp_i1 else 1)
    return i0, i1, (src - i0.astype(f32)).astype(f32).astype(f64)


def bilinear_ref(x, size, align, exact=False, mutant=None, weights_only=False):
    xd = np.abs(x.astype(f64)) if weights_only else x.astype(f64)
    bs, C, h, w = xd.shape
    if mutant == "modes_exchanged":
        align = not align
    y0, y1, ly = bilinear_coord(size[0], h, align, mutant != "no_clamp_neg", mutant != "i1_unclamped")
    x0, x1, lx = bilinear_coord(size[1], w, align, mutant != "no_clamp_neg", mutant != "i1_unclamped")
    if weights_only:
        ly, lx = np.abs(ly), np.abs(lx)
    flat = np.concatenate([xd.reshape(bs * C, h * w), np.zeros((bs * C, w + 2))], 1)       # i1 past the edge reads on in memory (zeros past the plane here)

    def at(yy, xx):
        return flat[:, (yy[:, None] * w + xx[None, :]).ravel()].reshape(bs, C, size[0], size[1])

    ly, lx = ly[:, None], lx[None, :]
    if mutant == "weights_exchanged":                      # a pixel's row weight taken for its column weight and the other way round
        ly, lx = lx, ly
    hy, hx = 1.0 - ly, 1.0 - lx
    if weights_only:
        hy, hx = np.abs(hy), np.abs(hx)
    return {"out": hy * (hx * at(y0, x0) + lx * at(y0, x1)) + ly * (hx * at(y1, x0) + lx * at(y1, x1))}


def bilinear_bar(x, size, align, exact=False):
    """hx 1, hx v00 1, the fma 1, hy * top 1, the sum 1 (hy beside them): 5 <= 6, times the weighted absolute values.  The identity resize is exact: every
    weight is 0 or 1."""
    if exact:
        return {"out": np.zeros((x.shape[0], x.shape[1]) + tuple(size))}
    return {"out": 6 * U * bilinear_ref(x, size, align, weights_only=True)["out"]}


def bilinear_stock(x, size, align, **_):
    return {"out": F.interpolate(torch.from_numpy(x), size=tuple(size), mode="bilinear", align_corners=align).numpy()}


# ================================================================================================ gate_add_upsample
GAU = [((2, 3, 5, 7, 1), "g"), ((1, 4, 3, 3, 2), "gv"), ((2, 2, 16, 33, 2), "gm"), ((1, 1, 1, 1, 3), ""), ((1, 5, 4, 6, 2), "gmv"),
       ((2, 3, 2, 5, 3), "gmv")]            # (the last one added: add_vec by channel instead of by plane shows with two images only)


def _gau_cases():
    return [dict(name="x".join(map(str, s)) + "." + (f or "bare"), shape=s, flags=f) for s, f in GAU]


def _gau_inputs(c):
    bs, C, h, w, up = c["shape"]
    key, f = "gau" + c["name"], c["flags"]
    n = bs * C
    return dict(feat=arr(key + "f", (bs, C, h, w), 3.0, 1.0), gate=(0.2 + 0.13 * np.arange(n)).astype(f32).reshape(bs, C) if "g" in f else None,
                add_map=arr(key + "m", (bs, C, h, w), -2.0, 1.0) if "m" in f else None,
                add_vec=(-1.0 + 0.37 * np.arange(n)).astype(f32).reshape(bs, C) if "v" in f else None, up=up)


def gau_ref(feat, gate, add_map, add_vec, up, mutant=None):
    """``F.interpolate(feat * gate + add_map, scale_factor=up, mode='nearest') + add_vec`` with gate / add_vec per (image, channel)."""
    fd = feat.astype(f64)
    bs, C, h, w = fd.shape
    oh, ow = h * up, w * up
    Y, X = np.arange(oh), np.arange(ow)
    sy = Y % h if mutant == "y_mod_h" else Y // up
    sx = X // up
    pick = lambda t: t[:, :, sy][:, :, :, sx]        # noqa: E731
    g = _bc(gate) if gate is not None else 1.0
    v = pick(fd) * g
    if add_map is not None:
        if mutant == "map_at_output_res":            # add_map[(plane * oh + Y) * ow + X], as if it had the output's size (past its end: the values again)
            am = np.resize(add_map.astype(f64).ravel(), bs * C * oh * ow).reshape(bs, C, oh, ow)
        else:
            am = pick(add_map.astype(f64))
        v = (pick(fd) + am) * g if mutant == "gate_on_sum" else v + am
    if add_vec is not None:
        av = np.asarray(add_vec, f64).reshape(bs, C)
        if mutant == "vec_by_channel":
            av = np.broadcast_to(av.ravel()[:C][None], (bs, C))
        v = v + av[:, :, None, None]
    return {"out": v}


def gau_bar(feat, gate, add_map, add_vec, up):
    """The product, the two sums: at most three roundings."""
    tot = gau_ref(np.abs(feat), None if gate is None else np.abs(gate), None if add_map is None else np.abs(add_map),
                  None if add_vec is None else np.abs(add_vec), up)["out"]
    return {"out": 3 * U * tot}


def gau_stock(feat, gate, add_map, add_vec, up):
    t = torch.from_numpy(feat)
    bs, C = t.shape[:2]
    if gate is not None:
        t = t * torch.from_numpy(gate).reshape(bs, C, 1, 1)
    if add_map is not None:
        t = t + torch.from_numpy(add_map)
    t = F.interpolate(t, scale_factor=up, mode="nearest")
    if add_vec is not None:
        t = t + torch.from_numpy(add_vec).reshape(bs, C, 1, 1)
    return {"out": t.numpy()}


# ================================================================================================ tensor2im_u8
T2I = [(2, 3, 5, 7), (1, 3, 16, 16), (1, 3, 1, 1), (1, 3, 520, 512)]


def _t2i_cases():
    return [dict(name="x".join(map(str, s)), shape=s) for s in T2I]


def _t2i_inputs(c):
    s = c["shape"]
    if s == (1, 3, 16, 16):
        # every grey level's exact pre-image 2 k / 255 - 1 in one channel, its float32 neighbours below and above in the other two
        k = (np.arange(256, dtype=f64) * 2.0 / 255.0 - 1.0).astype(f32)
        x = np.stack([k, np.nextafter(k, f32(-4)), np.nextafter(k, f32(4))]).reshape(1, 3, 16, 16)
    else:
        x = arr("t2i" + c["name"], s, 0.0, 0.8)       # scaled past +-1: about a fifth of the values clamp
    return dict(img=np.ascontiguousarray(x, f32))


def t2i_ref(img, mutant=None):
    """``tensor2im``: ``((x + 1) / 2).clamp(0, 1) * 255`` in float32, in that order, truncated to uint8, [bs, H, W, 3]."""
    v = ((img.astype(f32) + f32(1)) / f32(2)).astype(f32)
    if mutant == "clamp_after_scale":
        v = np.clip((v * f32(255)).astype(f32), 0, 1)
    else:
        v = (np.clip(v, 0, 1) * f32(255)).astype(f32)
    v = np.rint(v) if mutant == "round" else np.trunc(v)
    out = v.astype(np.uint8)
    return {"out": out if mutant == "chw" else np.ascontiguousarray(out.transpose(0, 2, 3, 1))}


def t2i_bar(img):
    return {"out": np.zeros((img.shape[0],) + img.shape[2:] + (3,))}


def t2i_stock(img):
    t = ((torch.from_numpy(img) + 1) / 2).clamp(0, 1) * 255
    return {"out": t.to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()}


# ================================================================================================ the tables
def _mut(fn, **kw):
    return lambda **inp: fn(**inp, **kw)


OPS = {
    # op: (cases, inputs, reference64, bar, stock32, emulate32 or None)
    "plane_stats": (_plane_cases(), _plane_inputs, plane_stats_ref, plane_stats_bar, plane_stats_stock, plane_stats_emulate),
    "vec_fc": (_fc_cases(), _fc_inputs, vec_fc_ref, vec_fc_bar, vec_fc_stock, vec_fc_emulate),
    "se_gate": (_se_cases(), _se_inputs, se_gate_ref, se_gate_bar, se_gate_stock, se_gate_emulate),
    "norm_gate_add": (NGA_PLAIN, _nga_inputs, nga_ref, nga_bar, nga_stock, nga_emulate),
    "norm_gate_add_stats": (NGA_STATS, _nga_inputs, nga_ref, nga_bar, nga_stock, nga_emulate),
    "norm_gate_add_self": (NGA_SELF, _nga_inputs, nga_ref, nga_bar, nga_stock, nga_emulate),
    "masked_avg_pool": (_pool_cases(), _pool_inputs, pool_ref, pool_bar, pool_stock, pool_emulate),
    "bilinear_resize": (_bil_cases(), _bil_inputs, bilinear_ref, bilinear_bar, bilinear_stock, None),
    "gate_add_upsample": (_gau_cases(), _gau_inputs, gau_ref, gau_bar, gau_stock, None),
    "tensor2im_u8": (_t2i_cases(), _t2i_inputs, t2i_ref, t2i_bar, t2i_stock, None),
}
CASES = {op: v[0] for op, v in OPS.items()}

MUTANTS = {
    "plane_stats": {
        "last element lost": _mut(plane_stats_ref, lose="last"),
        "last partial round lost": _mut(plane_stats_ref, lose="round"),
        "variance over hw - 1": _mut(plane_stats_ref, ddof=1),
        "eps outside the square root": _mut(plane_stats_ref, eps_outside=True),
        "nmean without rstd": _mut(plane_stats_ref, nmean_no_rstd=True),
    },
    "vec_fc": {
        "cin % 64 tail lost": _mut(vec_fc_ref, lose_tail=True),
        "BatchNorm after the activation": _mut(vec_fc_ref, bn_after_act=True),
        "sqrt(var) + eps": _mut(vec_fc_ref, eps_outside=True),
        "beta lost": _mut(vec_fc_ref, no_beta=True),
        "sigmoid of +a": _mut(vec_fc_ref, sig_plus=True),
    },
    "se_gate": {
        "hidden units >= 32 lost": _mut(se_gate_ref, lose_hidden=True),
        "ReLU lost": _mut(se_gate_ref, no_relu=True),
        "outputs >= 64 floor(C / 64) lost": _mut(se_gate_ref, lose_outputs=True),
    },
    "norm_gate_add": _nga_mutants(_NGA_COMMON),
    "norm_gate_add_stats": _nga_mutants(_NGA_COMMON + ["stats_before_prelu"]),
    "norm_gate_add_self": _nga_mutants(_NGA_COMMON + ["stats_before_prelu", "eps_swapped"]),
    "masked_avg_pool": {
        "division by hw": _mut(pool_ref, mutant="div_hw"),
        "labels sampled with round": _mut(pool_ref, mutant="round"),
        "empty region gives NaN": _mut(pool_ref, mutant="empty_nan"),
        "label 255 counted as region 0": _mut(pool_ref, mutant="none_is_zero"),
        "label >= nreg folded into nreg - 1": _mut(pool_ref, mutant="fold"),
    },
    "bilinear_resize": {
        "align_corners modes exchanged": _mut(bilinear_ref, mutant="modes_exchanged"),
        "negative src not clamped": _mut(bilinear_ref, mutant="no_clamp_neg"),
        "i1 not clamped at the edge": _mut(bilinear_ref, mutant="i1_unclamped"),
        "x and y weights exchanged": _mut(bilinear_ref, mutant="weights_exchanged"),
    },
    "gate_add_upsample": {
        "add_map read at output resolution": _mut(gau_ref, mutant="map_at_output_res"),
        "gate applied to the sum": _mut(gau_ref, mutant="gate_on_sum"),
        "add_vec by channel": _mut(gau_ref, mutant="vec_by_channel"),
        "source row Y % h": _mut(gau_ref, mutant="y_mod_h"),
    },
    "tensor2im_u8": {
        "round to nearest": _mut(t2i_ref, mutant="round"),
        "clamp after the scaling": _mut(t2i_ref, mutant="clamp_after_scale"),
        "CHW output": _mut(t2i_ref, mutant="chw"),
    },
}

_BUILT = {}


def case_names(op):
    return [c["name"] for c in CASES[op]]


def built(op, name):
    """(inputs, reference64, bar) of a case, computed once and left unchanged."""
    if (op, name) not in _BUILT:
        c = next(c for c in CASES[op] if c["name"] == name)
        _, make, ref, bar, _, _ = OPS[op]
        inp = make(c)
        _BUILT[op, name] = (inp, ref(**inp), bar(**inp))
    return _BUILT[op, name]


def with_emitted(inp, got):
    """plane_stats, mode 'nmean': the reference and bar of ``nmean`` for the float32 (mean, rstd) that came with it."""
    inp = dict(inp, emitted=(np.asarray(got["mean"], f32), np.asarray(got["rstd"], f32)))
    return inp, plane_stats_ref(**inp), plane_stats_bar(**inp)


def ratio(got, ref, bar):
    """Worst |got - ref| / bar over all outputs; a bar of 0 asks for equality (0 or inf); a NaN or a shape mismatch is inf."""
    worst = 0.0
    for k, r in ref.items():
        g = np.asarray(got[k])
        if g.shape != r.shape:
            return math.inf
        e = np.abs(g.astype(f64) - r.astype(f64))
        if np.isnan(e).any():
            return math.inf
        b = np.broadcast_to(np.asarray(bar[k], f64), e.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e == 0, 0.0, np.where(b > 0, e / b, math.inf))
        worst = max(worst, float(q.max()) if q.size else 0.0)
    return worst
