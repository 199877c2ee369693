"""A plain CPU model of what csrc/conv.hip computes: the operand splits of its four arithmetics with the products summed in float64 (``emulate``), the
float64 reference of the same operation (``reference64``), the single-product mutants (``drop=``) the parity bars are derived from, and a mirror of the
launch rules (``select_kernel`` / ``all_instantiations``) that says which kernel instantiation a launch reaches.  No GPU and no library import.

Arithmetic names: ``"sb"`` two-term bf16 (NS = 2), ``"sb3"`` three-term bf16 (NS = 3), ``"f16x3"`` two-term f16 (NS = 4), ``"f32"`` exact fp32.
A product ``(a, b)`` multiplies weight term ``a`` with activation term ``b`` (``TA`` / ``TB`` of ``compute_chunk``)."""
import math
import zlib

import torch
import torch.nn.functional as F

ARITHS = ("sb", "sb3", "f16x3", "f32")
NS = {"sb": 2, "sb3": 3, "f16x3": 4, "f32": 0}
PRODUCTS = {
    "f32": ((0, 0),),
    "sb": ((0, 0), (0, 1), (1, 0)),
    "f16x3": ((0, 0), (0, 1), (1, 0)),
    "sb3": ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)),
}
_TERMS = {"f32": (1, torch.float32), "sb": (2, torch.bfloat16), "sb3": (3, torch.bfloat16), "f16x3": (2, torch.float16)}


# ------------------------------------------------------------------------------------------------ operand splits
def split_terms(t, n, dtype):
    """``n`` terms of ``t`` (fp32): hi = dtype(t), lo = dtype(t - hi), ... — each the round-to-nearest-even of the running fp32 residual
    (``c2_split2``, ``c2_split2_f16``, the ``NS == 3`` branch).  Returned as fp32 tensors that hold the ``dtype`` values exactly."""
    r = t.float()
    out = []
    for _ in range(n):
        h = r.to(dtype).float()
        out.append(h)
        r = r - h
    return out


# ------------------------------------------------------------------------------------------------ weight preparation
def _sqrt32(t):
    """Correctly rounded fp32 square root, as the device's ``sqrtf`` (a vectorised CPU ``torch.sqrt`` of fp32 is an ulp off now and then, and one ulp
    in a channel's scale re-rounds the second bf16 term of its weights: visible at the bar of the two-term kernel)."""
    return torch.sqrt(t.double()).float()


def _div32(a, b):
    return (a.double() / b.double()).float()


def fold32(w, bn=None, conv_bias=None):
    """(weight * g[co], bias or None) in the fp32 formula of ``conv_prep_sb_kernel``: g = gamma / sqrt(var + eps), bias = beta - mean * g + conv_bias * g.
    ``bn`` = (gamma, beta, mean, var, eps) or None."""
    w = w.float()
    if bn is None:
        return w, (conv_bias.float().clone() if conv_bias is not None else None)
    gamma, beta, mean, var, eps = bn
    g = _div32(gamma.float(), _sqrt32(var.float() + torch.tensor(eps, dtype=torch.float32)))
    b = beta.float() - mean.float() * g
    if conv_bias is not None:
        b = b + conv_bias.float() * g
    return w * g[:, None, None, None], b


def fold64(w, bn=None, conv_bias=None):
    """The same fold in float64 (the reference's)."""
    w = w.double()
    if bn is None:
        return w, (conv_bias.double() if conv_bias is not None else None)
    gamma, beta, mean, var, eps = bn
    g = gamma.double() / torch.sqrt(var.double() + eps)
    b = beta.double() - mean.double() * g
    if conv_bias is not None:
        b = b + conv_bias.double() * g
    return w.double() * g[:, None, None, None], b


def f16_kexp(w, bn=None):
    """log2 of the power-of-two pre-scale ``PreparedConv.get`` chooses for the f16 split: the largest folded weight lands in (2^9, 2^10]."""
    wmax = w.float().abs().flatten(1).amax(1)
    if bn is not None:
        gamma, _, _, var, eps = bn
        wmax = wmax * _div32(gamma.float(), _sqrt32(var.float() + torch.tensor(eps, dtype=torch.float32))).abs()
    m = float(wmax.max())
    k = 10 - int(math.ceil(math.log2(m))) if m > 0 and math.isfinite(m) else 0
    return max(-30, min(30, k))


# ------------------------------------------------------------------------------------------------ the operation
def _input(x, x1, in_norm, dtype):
    x = x if x1 is None else torch.cat([x, x1], 1)
    x = x.to(dtype)
    if in_norm is not None:
        mean, rstd = in_norm
        x = (x - mean.to(dtype)[:, :, None, None]) * rstd.to(dtype)[:, :, None, None]
    return x


def _epilogue(y, bias, residual, relu, prelu):
    if bias is not None:
        y = y + bias.to(y.dtype)[None, :, None, None]
    if residual is not None:
        y = y + residual.to(y.dtype)
    if relu:
        y = F.relu(y)
    if prelu is not None:
        y = F.prelu(y, prelu.to(y.dtype))
    return y


def reference(x, w, *, dtype=torch.float64, bn=None, conv_bias=None, stride=1, pad=0, x1=None, in_norm=None, residual=None, relu=False, prelu=None):
    """``act(conv2d(norm(cat(x, x1)), fold(w)) + bias + residual)`` with plain ``F.conv2d`` in ``dtype``; ``in_norm`` = the fp32 (mean, rstd) ``[bs, cin]``
    the kernel is given (the operation is defined by those numbers, so the reference uses them too)."""
    wf, b = fold64(w, bn, conv_bias) if dtype == torch.float64 else fold32(w, bn, conv_bias)
    y = F.conv2d(_input(x, x1, in_norm, dtype), wf.to(dtype), stride=stride, padding=pad)
    return _epilogue(y, b, residual, relu, prelu)


def reference64(x, w, **kw):
    return reference(x, w, dtype=torch.float64, **kw)


def stock32(x, w, **kw):
    """The same operation on stock fp32 ``F.conv2d``: what an fp32-class bar must let pass."""
    return reference(x, w, dtype=torch.float32, **kw)


def emulate(x, w, arith, *, bn=None, conv_bias=None, stride=1, pad=0, x1=None, in_norm=None, residual=None, relu=False, prelu=None, drop=None,
            zero_lo_channel=None):
    """What the kernel of ``arith`` computes, with exact (float64) accumulation: weights folded in fp32 (f16x3: times 2^kexp), InstanceNorm-on-load in
    fp32, both operands split into the arithmetic's terms, the kernel's product list summed in float64, zero padding, then 2^-kexp, bias, residual and
    activation.  ``drop=(a, b)`` leaves the product of weight term ``a`` and activation term ``b`` out; ``zero_lo_channel=c`` zeroes the second
    activation term of input channel ``c``."""
    wf, b = fold32(w, bn, conv_bias)
    kexp = f16_kexp(w, bn) if arith == "f16x3" else 0
    n, dt = _TERMS[arith]
    wt = split_terms(wf * float(2.0 ** kexp), n, dt)
    xt = split_terms(_input(x, x1, in_norm, torch.float32), n, dt)
    if zero_lo_channel is not None:
        xt[1] = xt[1].clone()
        xt[1][:, zero_lo_channel] = 0
    y = None
    for a, bb in PRODUCTS[arith]:
        if drop is not None and (a, bb) == tuple(drop):
            continue
        t = F.conv2d(xt[bb].double(), wt[a].double(), stride=stride, padding=pad)
        y = t if y is None else y + t
    if y is None:
        y = torch.zeros_like(F.conv2d(xt[0].double(), wt[0].double(), stride=stride, padding=pad))
    return _epilogue(y * float(2.0 ** -kexp), b, residual, relu, prelu)


def maxdiff(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def mutant_errors(arith, ref, x, w, **kw):
    """{product: max |emulate(drop=product) - ref|} for every product of ``arith``."""
    return {pr: maxdiff(emulate(x, w, arith, drop=pr, **kw), ref) for pr in PRODUCTS[arith]}


def fp32_class_bar(ref, x, w, **kw):
    """The bar of the three fp32-class arithmetics on one case: half the error of the least visible single-product mutant of the three-term bf16 split.
    A kernel inside it is on the right side of every mutant with a factor two to spare."""
    return 0.5 * min(mutant_errors("sb3", ref, x, w, **kw).values())


# ------------------------------------------------------------------------------------------------ which kernel a launch reaches
def cdiv(a, b):
    return -(-a // b)


def out_size(h, w, ks, stride, pad):
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def route(arith, cin, ks):
    """The arithmetic ``ops.conv2d`` runs for a ``PreparedConv`` that asks for ``arith`` (``PreparedConv.use_sb``): the splits exist for 3x3 / 1x1 with
    cin >= 16, everything else is the exact-fp32 kernel."""
    return arith if (ks in (1, 3) and cin >= 16) else "f32"


_F32_CKK = {(3, 1): 8, (3, 2): 8, (1, 1): 32, (1, 2): 8, (7, 2): 2}
_SB_KS = ((3, 1), (3, 2), (1, 1), (1, 2))
# tile configurations (CB, PB, WC, WP, LOG_TW)
T_128CO_128PX = (2, 2, 2, 2, 5)      # fp32 only
T_64CO_256PX = (2, 2, 1, 4, 5)
T_64CO_128PX = (2, 1, 1, 4, 5)       # splits only
T_64CO_64PX = (1, 1, 2, 2, 5)
T_64CO_64PX_W16 = (1, 1, 2, 2, 4)
T_5X5 = (1, 1, 1, 4, 4)


def _pf(ns, ks, s, tile):
    return 2 if (ns in (2, 4) and tile[0] * tile[1] <= 2 and (s == 1 or ks == 1)) else 1


def _sb_name(ks, s, tile, ns):
    return ("conv2d_sb_kernel", (ks, s) + tile + (_pf(ns, ks, s, tile), ns))


def select_kernel(arith, ks, stride, bs, cin, cout, h, w, pad, plain=True):
    """(kernel name, template arguments) of the launch ``e4s_conv2d*`` makes for the arithmetic that really runs (see ``route``); ``plain``: no
    concatenated input, no norm-on-load and no residual (the condition of the direct 3-channel kernel)."""
    ho, wo = out_size(h, w, ks, stride, pad)
    nb = lambda tn, th, tw: cdiv(wo, tw) * cdiv(ho, th) * cdiv(cout, tn) * bs      # noqa: E731
    if arith == "f32":
        if cin <= 4 and plain and ks == 3 and ho * wo >= 4096:
            return ("conv_small_cin_kernel", (3,))
        head = (ks, stride, _F32_CKK[(ks, stride)])
        if wo >= 32:
            if cout > 64 and nb(128, 4, 32) >= 192:
                return ("conv2d_kernel", head + T_128CO_128PX)
            if cout > 32 and nb(64, 8, 32) >= 192:
                return ("conv2d_kernel", head + T_64CO_256PX)
            return ("conv2d_kernel", head + T_64CO_64PX)
        return ("conv2d_kernel", head + T_64CO_64PX_W16)
    ns = NS[arith]
    if ks == 5:
        assert stride == 1 and ns in (2, 3)
        return _sb_name(5, 1, T_5X5, ns)
    assert (ks, stride) in _SB_KS
    if wo >= 32:
        if ns == 3:
            if cout > 32 and nb(64, 4, 32) >= 256:
                return _sb_name(ks, stride, T_64CO_128PX, ns)
        else:
            if stride == 1 and cout > 32 and nb(64, 8, 32) >= 512:
                return _sb_name(ks, stride, T_64CO_256PX, ns)
            if cout > 32 and nb(64, 4, 32) >= 512:
                return _sb_name(ks, stride, T_64CO_128PX, ns)
        return _sb_name(ks, stride, T_64CO_64PX, ns)
    return _sb_name(ks, stride, T_64CO_64PX_W16, ns)


def all_instantiations():
    """Every kernel instantiation the dispatchers of csrc/conv.hip can select, written out from their source rather than derived from ``select_kernel``."""
    out = {("conv_small_cin_kernel", (3,))}
    for (ks, s), ckk in _F32_CKK.items():
        for tile in (T_128CO_128PX, T_64CO_256PX, T_64CO_64PX, T_64CO_64PX_W16):
            out.add(("conv2d_kernel", (ks, s, ckk) + tile))
    for ns in (2, 4):
        for ks, s in _SB_KS:
            for tile in ((T_64CO_256PX,) if s == 1 else ()) + (T_64CO_128PX, T_64CO_64PX, T_64CO_64PX_W16):
                out.add(_sb_name(ks, s, tile, ns))
    for ks, s in _SB_KS:
        for tile in (T_64CO_128PX, T_64CO_64PX, T_64CO_64PX_W16):
            out.add(_sb_name(ks, s, tile, 3))
    out.add(_sb_name(5, 1, T_5X5, 2))
    out.add(_sb_name(5, 1, T_5X5, 3))
    return out


def kernel_label(name, args):
    return f"{name}<{', '.join(str(a) for a in args)}>"


# ------------------------------------------------------------------------------------------------ the cases both test files share
def randn(key, shape, std=1.0):
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    return torch.randn(tuple(shape), generator=g, dtype=torch.float32) * std


def host_stats(x, eps=1e-5):
    """fp32 (mean, rstd) ``[bs, c]`` of the planes of ``x``, computed in float64."""
    xd = x.double()
    return xd.mean((2, 3)).float(), (1.0 / torch.sqrt(xd.var((2, 3), unbiased=False) + eps)).float()


def seeded_bn(key, c):
    return (randn(key + "g", (c,), 0.2) + 1, randn(key + "b", (c,), 0.2), randn(key + "m", (c,), 0.2), randn(key + "v", (c,), 0.2).abs() + 0.5, 1e-5)


# A. arithmetic cases: (name, ks, cin, cout, entry point, fused).  The 5x5 form exists on the two bf16 splits only and is reached through lossnet.conv_sb,
# which has bias, residual and ReLU but no norm-on-load, PReLU or BatchNorm fold.
ARITH_CASES = [
    ("3x3", 3, 32, 64, "ops", False),
    ("3x3_fused", 3, 32, 64, "ops", True),
    ("1x1", 1, 64, 64, "ops", False),
    ("1x1_fused", 1, 64, 64, "ops", True),
    ("5x5", 5, 32, 64, "conv_sb", False),
    ("5x5_fused", 5, 32, 64, "conv_sb", True),
]
ARITH_HW = 24


def arith_case(name):
    """(x, w, keyword arguments of ``emulate`` / ``reference64``, arithmetics, entry point) of one arithmetic case."""
    _, ks, cin, cout, via, fused = next(c for c in ARITH_CASES if c[0] == name)
    x = randn(name + "x", (1, cin, ARITH_HW, ARITH_HW))
    w = randn(name + "w", (cout, cin, ks, ks), (cin * ks * ks) ** -0.5)
    kw = dict(stride=1, pad=ks // 2)
    if fused and via == "ops":
        x = x * 3 + 1
        kw.update(bn=seeded_bn(name, cout), conv_bias=randn(name + "cb", (cout,), 0.3), in_norm=host_stats(x),
                  residual=randn(name + "r", (1, cout, ARITH_HW, ARITH_HW)), prelu=randn(name + "s", (cout,), 0.1) + 0.25)
    elif fused:
        kw.update(conv_bias=randn(name + "cb", (cout,), 0.3), residual=randn(name + "r", (1, cout, ARITH_HW, ARITH_HW)), relu=True)
    return x, w, kw, (ARITHS if via == "ops" else ("sb", "sb3")), via


# B. indexing cases: (id, entry point, ks, stride, pad, bs, cin, cout, h, w) — h, w are INPUT sizes.  Output sizes A 130 x 70 (bs 3, cout 200), B 90 x 70
# (bs 2, cout 200), C 170 x 70 (bs 3, cout 48), D 9 x 37 (cout 40), E 5 x 17 (cout 70) are the smallest launches that reach each tile configuration of each
# arithmetic (``select_kernel``); cin walks through 1 .. 5 chunks of 16 (8, 32 or 2 on the fp32 kernels) with ragged last chunks.
def _rows():
    rows = []
    for ks, pad in ((3, 1), (1, 0)):
        c = {3: (20, 40, 56), 1: (80, 48, 72)}[ks]
        rows += [(f"A{ks}1", "ops", ks, 1, pad, 3, c[0], 200, 130, 70), (f"B{ks}1", "ops", ks, 1, pad, 2, c[1], 200, 90, 70),
                 (f"C{ks}1", "ops", ks, 1, pad, 3, c[2], 48, 170, 70), (f"D{ks}1", "ops", ks, 1, pad, 1, 80, 40, 9, 37),
                 (f"E{ks}1", "ops", ks, 1, pad, 2, 16 if ks == 3 else 17, 70, 5, 17), (f"F{ks}1", "ops", ks, 1, pad, 1, 24, 40, 9, 37),
                 (f"G{ks}1", "ops", ks, 1, pad, 1, 64, 40, 9, 37)]
        # stride 2: B from an odd map, C from an even one, D odd x even, E even x odd
        rows += [(f"B{ks}2", "ops", ks, 2, pad, 2, c[1], 200, 179, 139), (f"C{ks}2", "ops", ks, 2, pad, 3, c[2], 48, 340, 140),
                 (f"D{ks}2", "ops", ks, 2, pad, 1, 80, 40, 17, 74), (f"E{ks}2", "ops", ks, 2, pad, 2, 24, 70, 10, 33),
                 (f"F{ks}2", "ops", ks, 2, pad, 1, 16, 40, 18, 73)]
    # the 7x7 stride-2 form (fp32 only: 2-channel chunks)
    rows += [("B72", "ops", 7, 2, 3, 2, 3, 200, 179, 139), ("C72", "ops", 7, 2, 3, 3, 3, 48, 340, 140), ("D72", "ops", 7, 2, 3, 1, 5, 40, 17, 74),
             ("E72", "ops", 7, 2, 3, 2, 2, 70, 10, 33)]
    # fewer than 16 input channels: the fp32 implicit GEMM whatever arithmetic is asked for
    rows += [("T31", "ops", 3, 1, 1, 1, 10, 8, 9, 5), ("T32", "ops", 3, 2, 1, 2, 7, 33, 12, 35)]
    # lossnet.conv_sb: 5x5 at pads 2, 0 and 1, and 3x3 without padding
    rows += [("L52", "conv_sb", 5, 1, 2, 2, 40, 70, 19, 21), ("L50", "conv_sb", 5, 1, 0, 1, 16, 33, 23, 20), ("L51", "conv_sb", 5, 1, 1, 1, 24, 32, 9, 35),
             ("L30", "conv_sb", 3, 1, 0, 2, 24, 40, 11, 39), ("L30w", "conv_sb", 3, 1, 0, 1, 40, 70, 7, 19)]
    return rows


INDEX_ROWS = _rows()

# the direct 3-channel kernel: (id, stride, cin, h, w, activation); cout 70, pad 1, conv bias.  An output of 64 x 64 pixels is the smallest the direct
# kernel takes, 63 x 64 the largest that stays on the implicit GEMM.
SMALL_CIN_ROWS = [
    ("S_c3s1_prelu", 1, 3, 64, 64, "prelu"), ("S_c1s1_relu", 1, 1, 64, 64, "relu"), ("S_c3s2_prelu", 2, 3, 127, 128, "prelu"),
    ("S_c1s2_relu", 2, 1, 128, 128, "relu"), ("S_c3s1_gemm", 1, 3, 63, 64, "prelu"), ("S_c1s2_gemm", 2, 1, 126, 128, "relu"),
]
SMALL_CIN_COUT = 70

# fusions at one ragged shape (3x3, stride 1, pad 1): bs 2, cin 40, cout 70, 13 x 37
FUSION_SHAPE = (2, 40, 70, 13, 37)
FUSIONS = ("bn_bias", "residual_relu", "innorm_prelu", "x1_split16", "x1_straddle20", "x1_split16_innorm", "x1_straddle20_innorm")


def fusion_case(name):
    """(x, x1 or None, w, keyword arguments of the model) of one fusion."""
    bs, cin, cout, h, w_ = FUSION_SHAPE
    x = randn("fu_x", (bs, cin, h, w_)) * 3 + 1
    w = randn("fu_w", (cout, cin, 3, 3), (cin * 9) ** -0.5)
    kw = dict(stride=1, pad=1)
    if name == "bn_bias":
        kw.update(bn=seeded_bn("fu", cout), conv_bias=randn("fu_cb", (cout,), 0.3))
    if name == "residual_relu":
        kw.update(residual=randn("fu_r", (bs, cout, h, w_)), relu=True)
    if "innorm" in name:
        kw.update(in_norm=host_stats(x))
    if name == "innorm_prelu":
        kw.update(prelu=randn("fu_s", (cout,), 0.1) + 0.25)
    x1 = None
    if name.startswith("x1_"):
        c0 = 16 if "split16" in name else 20
        x, x1 = x[:, :c0].contiguous(), x[:, c0:].contiguous()
    return x, x1, w, kw


def table_launches():
    """(entry point, requested arithmetic, ks, stride, bs, cin, cout, h, w, pad, plain) of every launch the indexing, small-cin and fusion tables make."""
    out = []
    for _, via, ks, s, pad, bs, cin, cout, h, w in INDEX_ROWS:
        for a in (ARITHS if via == "ops" else ("sb", "sb3")):
            out.append((via, a, ks, s, bs, cin, cout, h, w, pad, True))
    for _, s, cin, h, w, _ in SMALL_CIN_ROWS:
        out.append(("ops", "f32", 3, s, 1, cin, SMALL_CIN_COUT, h, w, 1, True))
    bs, cin, cout, h, w = FUSION_SHAPE
    for a in ARITHS:
        out.append(("ops", a, 3, 1, bs, cin, cout, h, w, 1, False))
    return out


def table_kernels(default_arith="sb"):
    """The set of kernel instantiations ``table_launches`` reaches; ``default_arith``: what a plain ``PreparedConv()`` runs (``ops.CONV_MODE``).
    ``lossnet.conv_sb`` takes prepared slabs, so its arithmetic is the one asked for."""
    seen = set()
    for via, a, ks, s, bs, cin, cout, h, w, pad, plain in table_launches():
        if via == "ops":
            a = route(default_arith if a == "sb" else a, cin, ks)
        seen.add(select_kernel(a, ks, s, bs, cin, cout, h, w, pad, plain))
    return seen
