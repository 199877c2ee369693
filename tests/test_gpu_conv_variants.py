"""Every arithmetic and every tile of csrc/conv.hip against float64 and against the CPU model of tests/conv_model.py.

A. arithmetic cases (small K): the two-term bf16 kernel against its float64-accumulated emulation, the three fp32-class arithmetics (three-term bf16, two-term
   f16, exact fp32) against float64 — both at HALF the error of the least visible single-product mutant of the three-term split, a bar that
   tests/test_conv_model_cpu.py shows to separate right from wrong on the CPU alone.
B. indexing cases: the smallest launches that make the dispatchers select each of their 63 kernel instantiations, ragged in every dimension, at the suite's
   existing bars; one test reads the kernel names of the whole table from torch.profiler and compares them with the list written here.
C. the loss nets' host glue: ``prep_dgrad`` against the float64 autograd data gradient, ``prep_fwd`` with scale and shift.
D. the f16 range report of the two-term f16 kernel, and padding channels that must stay out of it."""
import re

import pytest
import torch
import torch.nn.functional as F

import conv_model as M
from conftest import record_parity
from e4s2024_amd import lossnet, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONV_RTOL = 1e-4 if ops.CONV_MODE == "sb" else 2e-5        # tests/test_gpu_encoder.py
FP32_RTOL = 2e-6                                           # tests/test_gpu_parser.py::test_stem7_kernel_against_float64
DEFAULT_ARITH = "sb" if ops.CONV_MODE == "sb" else "f32"   # what a plain PreparedConv() runs
EXACT = {"sb": False, "f32": True, "sb3": "sb3", "f16x3": "f16x3"}


def dev(t):
    return None if t is None else t.to(DEV)


def bn_module(bn):
    if bn is None:
        return None
    gamma, beta, mean, var, eps = bn
    m = torch.nn.BatchNorm2d(gamma.numel(), eps=eps).eval()
    with torch.no_grad():
        m.weight.copy_(gamma); m.bias.copy_(beta); m.running_mean.copy_(mean); m.running_var.copy_(var)
    return m.to(DEV)


def run_ops(arith, x, w, *, x1=None, bn=None, conv_bias=None, stride=1, pad=0, in_norm=None, residual=None, relu=False, prelu=None):
    prep = ops.PreparedConv(exact=EXACT[arith]).get(dev(w), bn_module(bn), dev(conv_bias))
    return ops.conv2d(dev(x), prep, stride, pad, x1=dev(x1), in_norm=None if in_norm is None else (dev(in_norm[0]), dev(in_norm[1])),
                      prelu=dev(prelu), relu=relu, residual=dev(residual))


def run_conv_sb(arith, x, w, *, conv_bias=None, stride=1, pad=0, residual=None, relu=False):
    """``lossnet.conv_sb`` on three-way slabs (``prep_fwd``) or on two-way slabs — those only ``prep_dgrad`` makes, of the flipped and transposed weight, so
    it is given the weight whose data-gradient convolution is ``w``."""
    wd = dev(w)
    if arith == "sb3":
        slabs, bias = lossnet.prep_fwd(wd, None, dev(conv_bias))
    else:
        slabs, bias = lossnet.prep_dgrad(wd.flip(2, 3).transpose(0, 1).contiguous()), dev(conv_bias)
    return lossnet.conv_sb(dev(x), slabs, bias, k=w.shape[2], stride=stride, pad=pad, relu=relu, residual=dev(residual))


def effective(via, arith, cin, ks):
    """The arithmetic a request ends on."""
    return arith if via == "conv_sb" else M.route(DEFAULT_ARITH if arith == "sb" else arith, cin, ks)


def index_bar(arith, ref):
    scale = ref.abs().max().item()
    return CONV_RTOL * max(1.0, scale) if arith == "sb" else FP32_RTOL * scale


def check_all(via, tag, ariths, x, w, kw, x1=None):
    """Runs one shape on every arithmetic against ONE float64 reference at the indexing bars; records every distance, then asserts."""
    ref = M.reference64(x, w, x1=x1, **kw)
    cin, ks = w.shape[1], w.shape[2]
    bad, done = [], set()
    for a in ariths:
        eff = effective(via, a, cin, ks)
        if eff in done:          # (fewer than 16 channels, 7x7: every request ends on the fp32 kernel)
            continue
        done.add(eff)
        out = run_ops(a, x, w, x1=x1, **kw) if via == "ops" else run_conv_sb(a, x, w, **kw)
        assert tuple(out.shape) == tuple(ref.shape)
        d, bar = M.maxdiff(out, ref), index_bar(eff, ref)
        record_parity(f"conv_variants.{eff}.{tag}", d, bar)
        if not (torch.isfinite(out).all().item() and d <= bar):
            bad.append((eff, d, bar))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ A. arithmetic
@pytest.mark.parametrize("name", [c[0] for c in M.ARITH_CASES])
def test_arithmetic_against_emulation_and_float64(name):
    """Worst measured share of the bar on an MI355X: the two-term bf16 kernel against its emulation 0.50 (``5x5_fused``; 0.15 .. 0.50 over the six cases, the
    fp32 accumulation of the MFMA chain), three-term bf16 0.71 (``5x5``), two-term f16 0.36 (``3x3``), exact fp32 0.71 (``3x3_fused``), all against float64.
    The emulation has to fold the BatchNorm scale with a correctly rounded fp32 square root and division, as the device does (``conv_model._sqrt32``): one
    ulp in a channel's scale re-rounds the second bf16 terms of its weights and moves the emulation by 0.5 .. 2 bars."""
    x, w, kw, ariths, via = M.arith_case(name)
    ref = M.reference64(x, w, **kw)
    scale = ref.abs().max().item()
    bar = M.fp32_class_bar(ref, x, w, **kw)
    bad = []
    for a in ariths:
        eff = effective(via, a, w.shape[1], w.shape[2])
        out = run_ops(a, x, w, **kw) if via == "ops" else run_conv_sb(a, x, w, **kw)
        d64 = M.maxdiff(out, ref)
        if eff == "sb":
            # the kernel and its emulation differ by fp32 accumulation only: the fp32-class bar sees a wrong lo plane, a lost or doubled product
            demu = M.maxdiff(out, M.emulate(x, w, "sb", **kw))
            record_parity(f"conv_variants.sb.{name}.vs_emulation", demu, bar, f"{demu / scale:.2e} of max|ref|")
            record_parity(f"conv_variants.sb.{name}.vs_float64", d64, CONV_RTOL * max(1.0, scale), f"{d64 / scale:.2e} of max|ref|")
            if not (demu <= bar and d64 <= CONV_RTOL * max(1.0, scale)):
                bad.append((a, demu, d64, bar))
        else:
            record_parity(f"conv_variants.{eff}.{name}.vs_float64", d64, bar, f"{d64 / scale:.2e} of max|ref|")
            if not d64 <= bar:
                bad.append((a, d64, bar))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ B. indexing
@pytest.mark.parametrize("row", M.INDEX_ROWS, ids=[r[0] for r in M.INDEX_ROWS])
def test_every_tile_of_every_arithmetic_against_float64(row):
    tag, via, ks, stride, pad, bs, cin, cout, h, w_ = row
    x = M.randn(tag + "x", (bs, cin, h, w_))
    w = M.randn(tag + "w", (cout, cin, ks, ks), (cin * ks * ks) ** -0.5)
    check_all(via, tag, M.ARITHS if via == "ops" else ("sb", "sb3"), x, w, dict(stride=stride, pad=pad))


@pytest.mark.parametrize("row", M.SMALL_CIN_ROWS, ids=[r[0] for r in M.SMALL_CIN_ROWS])
def test_direct_small_cin_kernel_and_its_threshold(row):
    tag, stride, cin, h, w_, act = row
    cout = M.SMALL_CIN_COUT
    x = M.randn(tag + "x", (2, cin, h, w_))
    w = M.randn(tag + "w", (cout, cin, 3, 3), (cin * 9) ** -0.5)
    kw = dict(stride=stride, pad=1, conv_bias=M.randn(tag + "b", (cout,), 0.3))
    if act == "prelu":
        kw["prelu"] = M.randn(tag + "s", (cout,), 0.1) + 0.25
    else:
        kw["relu"] = True
    check_all("ops", tag, ("f32",), x, w, kw)


@pytest.mark.parametrize("name", M.FUSIONS)
def test_fusions_on_every_arithmetic(name):
    x, x1, w, kw = M.fusion_case(name)
    check_all("ops", "fusion_" + name, M.ARITHS, x, w, kw, x1=x1)


def test_empty_batch():
    w = M.randn("e_w", (40, 20, 3, 3), 0.1)
    x = torch.zeros((0, 20, 9, 11), device=DEV)
    for a in M.ARITHS:
        assert tuple(run_ops(a, x, w, stride=1, pad=1).shape) == (0, 40, 9, 11)
    assert tuple(run_ops("f32", torch.zeros((0, 3, 64, 64), device=DEV), M.randn("e_w3", (8, 3, 3, 3)), pad=1).shape) == (0, 8, 64, 64)
    for a in ("sb", "sb3"):
        assert tuple(run_conv_sb(a, x, w, pad=0).shape) == (0, 40, 7, 9)


# the kernels the dispatchers of csrc/conv.hip can select: <KS, S, CKK, CB, PB, WC, WP, LOG_TW> of the fp32 kernel, <KS, S, CB, PB, WC, WP, LOG_TW, PF, NS> of the splits
KERNELS = """
conv_small_cin_kernel<3>
conv2d_kernel<1, 1, 32, 1, 1, 2, 2, 4> conv2d_kernel<1, 1, 32, 1, 1, 2, 2, 5> conv2d_kernel<1, 1, 32, 2, 2, 1, 4, 5> conv2d_kernel<1, 1, 32, 2, 2, 2, 2, 5>
conv2d_kernel<1, 2, 8, 1, 1, 2, 2, 4> conv2d_kernel<1, 2, 8, 1, 1, 2, 2, 5> conv2d_kernel<1, 2, 8, 2, 2, 1, 4, 5> conv2d_kernel<1, 2, 8, 2, 2, 2, 2, 5>
conv2d_kernel<3, 1, 8, 1, 1, 2, 2, 4> conv2d_kernel<3, 1, 8, 1, 1, 2, 2, 5> conv2d_kernel<3, 1, 8, 2, 2, 1, 4, 5> conv2d_kernel<3, 1, 8, 2, 2, 2, 2, 5>
conv2d_kernel<3, 2, 8, 1, 1, 2, 2, 4> conv2d_kernel<3, 2, 8, 1, 1, 2, 2, 5> conv2d_kernel<3, 2, 8, 2, 2, 1, 4, 5> conv2d_kernel<3, 2, 8, 2, 2, 2, 2, 5>
conv2d_kernel<7, 2, 2, 1, 1, 2, 2, 4> conv2d_kernel<7, 2, 2, 1, 1, 2, 2, 5> conv2d_kernel<7, 2, 2, 2, 2, 1, 4, 5> conv2d_kernel<7, 2, 2, 2, 2, 2, 2, 5>
conv2d_sb_kernel<1, 1, 1, 1, 2, 2, 4, 1, 3> conv2d_sb_kernel<1, 1, 1, 1, 2, 2, 4, 2, 2> conv2d_sb_kernel<1, 1, 1, 1, 2, 2, 4, 2, 4>
conv2d_sb_kernel<1, 1, 1, 1, 2, 2, 5, 1, 3> conv2d_sb_kernel<1, 1, 1, 1, 2, 2, 5, 2, 2> conv2d_sb_kernel<1, 1, 1, 1, 2, 2, 5, 2, 4>
conv2d_sb_kernel<1, 1, 2, 1, 1, 4, 5, 1, 3> conv2d_sb_kernel<1, 1, 2, 1, 1, 4, 5, 2, 2> conv2d_sb_kernel<1, 1, 2, 1, 1, 4, 5, 2, 4>
conv2d_sb_kernel<1, 1, 2, 2, 1, 4, 5, 1, 2> conv2d_sb_kernel<1, 1, 2, 2, 1, 4, 5, 1, 4>
conv2d_sb_kernel<1, 2, 1, 1, 2, 2, 4, 1, 3> conv2d_sb_kernel<1, 2, 1, 1, 2, 2, 4, 2, 2> conv2d_sb_kernel<1, 2, 1, 1, 2, 2, 4, 2, 4>
conv2d_sb_kernel<1, 2, 1, 1, 2, 2, 5, 1, 3> conv2d_sb_kernel<1, 2, 1, 1, 2, 2, 5, 2, 2> conv2d_sb_kernel<1, 2, 1, 1, 2, 2, 5, 2, 4>
conv2d_sb_kernel<1, 2, 2, 1, 1, 4, 5, 1, 3> conv2d_sb_kernel<1, 2, 2, 1, 1, 4, 5, 2, 2> conv2d_sb_kernel<1, 2, 2, 1, 1, 4, 5, 2, 4>
conv2d_sb_kernel<3, 1, 1, 1, 2, 2, 4, 1, 3> conv2d_sb_kernel<3, 1, 1, 1, 2, 2, 4, 2, 2> conv2d_sb_kernel<3, 1, 1, 1, 2, 2, 4, 2, 4>
conv2d_sb_kernel<3, 1, 1, 1, 2, 2, 5, 1, 3> conv2d_sb_kernel<3, 1, 1, 1, 2, 2, 5, 2, 2> conv2d_sb_kernel<3, 1, 1, 1, 2, 2, 5, 2, 4>
conv2d_sb_kernel<3, 1, 2, 1, 1, 4, 5, 1, 3> conv2d_sb_kernel<3, 1, 2, 1, 1, 4, 5, 2, 2> conv2d_sb_kernel<3, 1, 2, 1, 1, 4, 5, 2, 4>
conv2d_sb_kernel<3, 1, 2, 2, 1, 4, 5, 1, 2> conv2d_sb_kernel<3, 1, 2, 2, 1, 4, 5, 1, 4>
conv2d_sb_kernel<3, 2, 1, 1, 2, 2, 4, 1, 2> conv2d_sb_kernel<3, 2, 1, 1, 2, 2, 4, 1, 3> conv2d_sb_kernel<3, 2, 1, 1, 2, 2, 4, 1, 4>
conv2d_sb_kernel<3, 2, 1, 1, 2, 2, 5, 1, 2> conv2d_sb_kernel<3, 2, 1, 1, 2, 2, 5, 1, 3> conv2d_sb_kernel<3, 2, 1, 1, 2, 2, 5, 1, 4>
conv2d_sb_kernel<3, 2, 2, 1, 1, 4, 5, 1, 2> conv2d_sb_kernel<3, 2, 2, 1, 1, 4, 5, 1, 3> conv2d_sb_kernel<3, 2, 2, 1, 1, 4, 5, 1, 4>
conv2d_sb_kernel<5, 1, 1, 1, 1, 4, 4, 1, 3> conv2d_sb_kernel<5, 1, 1, 1, 1, 4, 4, 2, 2>
"""
_KERNEL_RE = re.compile(r"\b(conv2d_sb_kernel|conv2d_kernel|conv_small_cin_kernel)<([0-9, ]+)>")


def kernel_set(text):
    return {f"{n}<{', '.join(a.strip() for a in args.split(','))}>" for n, args in _KERNEL_RE.findall(text)}


def test_table_runs_every_selectable_kernel():
    """The launches of the indexing, small-cin and fusion tables under torch.profiler: the kernel names seen are exactly the 63 instantiations written above,
    so a retuned threshold that drops a configuration from this file's coverage fails here.  (Random device data: only the launch geometry matters.)"""
    from torch.profiler import profile, ProfilerActivity
    want = kernel_set(KERNELS)
    assert len(want) == 63 and want == {M.kernel_label(*k) for k in M.all_instantiations()}
    if DEFAULT_ARITH != "sb":          # E4S_CONV=f32: a plain PreparedConv() is on the fp32 kernel, the two-term 3x3 / 1x1 forms are not on the table's routes
        want = {M.kernel_label(*k) for k in M.table_kernels(DEFAULT_ARITH)}

    def launch(via, a, ks, s, bs, cin, cout, h, w_, pad, plain):
        x = torch.randn((bs, cin, h, w_), device=DEV)
        w = torch.randn((cout, cin, ks, ks), device=DEV) * 0.05
        if via == "conv_sb":
            slabs = lossnet.prep_fwd(w)[0] if a == "sb3" else lossnet.prep_dgrad(w.transpose(0, 1).contiguous())
            return lossnet.conv_sb(x, slabs, k=ks, stride=s, pad=pad)
        ho, wo = M.out_size(h, w_, ks, s, pad)
        res = None if plain else torch.randn((bs, cout, ho, wo), device=DEV)
        return ops.conv2d(x, ops.PreparedConv(exact=EXACT[a]).get(w), s, pad, residual=res)

    launches = M.table_launches()
    launch(*launches[0])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for ln in launches:
            launch(*ln)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    seen = kernel_set("\n".join(names))
    record_parity("conv_variants.coverage.instantiations_named_by_profiler", len(seen), len(want))
    if not seen:
        # a profiler build that strips template arguments (recorded above as 0 named instantiations): the table is held to the mirror of the dispatch rules in
        # tests/conv_model.py, and every launch of the table must show up under the base name of the kernel the mirror predicts
        predicted = {}
        for via, a, ks, s, bs, cin, cout, h, w_, pad, plain in launches:
            eff = effective(via, a, cin, ks)
            base = M.select_kernel(eff, ks, s, bs, cin, cout, h, w_, pad, plain)[0]
            predicted[base] = predicted.get(base, 0) + 1
        counts = {base: sum(e.count for e in prof.key_averages() if re.search(r"\b" + base + r"\b", e.key)) for base in predicted}
        assert counts == predicted, (counts, predicted)
        seen = {M.kernel_label(*k) for k in M.table_kernels(DEFAULT_ARITH)}
    assert seen == want, (sorted(want - seen), sorted(seen - want))


# ------------------------------------------------------------------------------------------------ C. host glue of the loss nets
@pytest.mark.parametrize("k,cin,cout,h,w_", [(3, 24, 40, 13, 37), (1, 40, 24, 9, 35), (5, 20, 33, 19, 21)])
@pytest.mark.parametrize("scaled", [False, True])
def test_prep_dgrad_is_the_float64_data_gradient(k, cin, cout, h, w_, scaled):
    tag = f"dgrad{k}{'s' if scaled else ''}"
    w = M.randn(tag + "w", (cout, cin, k, k), (cin * k * k) ** -0.5).double()
    g = M.randn(tag + "g", (2, cout, h, w_)).double()
    so = (M.randn(tag + "so", (cout,), 0.3) + 1).double() if scaled else None
    si = (M.randn(tag + "si", (cin,), 0.3) + 1).double() if scaled else None
    x = M.randn(tag + "x", (2, cin, h, w_)).double().requires_grad_(True)
    y = F.conv2d(x * si[None, :, None, None] if scaled else x, w, padding=k // 2)
    ((y * so[None, :, None, None] if scaled else y) * g).sum().backward()
    ref = x.grad
    out = lossnet.conv_sb(dev(g.float()), lossnet.prep_dgrad(dev(w.float()), dev(so), dev(si)), k=k)
    assert tuple(out.shape) == tuple(ref.shape)
    d, bar = M.maxdiff(out, ref), CONV_RTOL * max(1.0, ref.abs().max().item())
    record_parity(f"conv_variants.sb.{tag}", d, bar)
    assert d <= bar


@pytest.mark.parametrize("k,cin,cout,h,w_", [(3, 24, 40, 13, 37), (1, 40, 24, 9, 35), (5, 20, 33, 19, 21)])
def test_prep_fwd_with_scale_and_shift(k, cin, cout, h, w_):
    tag = f"fwd{k}"
    w = M.randn(tag + "w", (cout, cin, k, k), (cin * k * k) ** -0.5)
    x = M.randn(tag + "x", (2, cin, h, w_))
    scale, shift = (M.randn(tag + "sc", (cout,), 0.3) + 1).double(), M.randn(tag + "sh", (cout,), 0.3).double()
    ref = F.conv2d(x.double(), w.double(), padding=k // 2) * scale[None, :, None, None] + shift[None, :, None, None]
    slabs, bias = lossnet.prep_fwd(dev(w), dev(scale), dev(shift))
    out = lossnet.conv_sb(dev(x), slabs, bias, k=k)
    # the bar of the arithmetic cases: half the least visible single-product mutant of the three-term split on this very operation
    w_scaled = (w.double() * scale[:, None, None, None]).float()
    bar = M.fp32_class_bar(ref, x, w_scaled, conv_bias=shift.float(), stride=1, pad=k // 2)
    d = M.maxdiff(out, ref)
    record_parity(f"conv_variants.sb3.{tag}", d, bar, f"bar = {bar / ref.abs().max().item():.2e} of max|ref|")
    assert d <= bar


# ------------------------------------------------------------------------------------------------ D. the f16 range report
def test_f16_range_report_and_exact_rerun():
    """An activation that leaves the f16 range after the norm-on-load is reported (an ordinary return path), an O(1) input is not, and the same weights
    under ``ops.mx_exact()`` run the three-term bf16 split: finite and within the fp32-class bar."""
    x = M.randn("rr_x", (2, 32, 13, 37))
    w = M.randn("rr_w", (40, 32, 3, 3), 288 ** -0.5)
    mean, rstd = torch.zeros((2, 32)), torch.ones((2, 32))
    ref = M.reference64(x, w, pad=1, in_norm=(mean, rstd))
    ops.mx_overflowed()
    out = run_ops("f16x3", x, w, pad=1, in_norm=(mean, rstd))
    assert not ops.mx_overflowed()
    assert M.maxdiff(out, ref) <= FP32_RTOL * ref.abs().max().item()
    big = rstd.clone()
    big[1, 5] = 1e5 / x[1, 5].abs().max().item()                 # one plane whose normalised peak is 1e5
    run_ops("f16x3", x, w, pad=1, in_norm=(mean, big))
    assert ops.mx_overflowed()
    assert not ops.mx_overflowed()                                # (reading the report clears it)
    ref_big = M.reference64(x, w, pad=1, in_norm=(mean, big))
    pc = ops.PreparedConv(exact="f16x3")
    with ops.mx_exact():
        out3 = ops.conv2d(dev(x), pc.get(dev(w)), 1, 1, in_norm=(dev(mean), dev(big)))
    assert not ops.mx_overflowed()
    assert torch.isfinite(out3).all().item()
    d, bar = M.maxdiff(out3, ref_big), FP32_RTOL * ref_big.abs().max().item()
    record_parity("conv_variants.sb3.range_rerun", d, bar)
    assert d <= bar


def test_padding_channels_stay_out_of_the_f16_range():
    """cin = 20: the last 16-channel chunk has 12 padding channels, staged from a clamped real channel.  With norm-on-load of an input around 1e5 every real
    operand is O(1); the padding must be an exact zero, not the raw 1e5 (an f16 infinity: a false range report and inf * 0 = NaN in every output)."""
    x = M.randn("pc_x", (2, 20, 9, 37)) * 3e4 + 1e5
    w = M.randn("pc_w", (40, 20, 3, 3), 180 ** -0.5)
    kw = dict(stride=1, pad=1, in_norm=M.host_stats(x))
    ref = M.reference64(x, w, **kw)
    ops.mx_overflowed()
    out = run_ops("f16x3", x, w, **kw)
    reported = ops.mx_overflowed()
    finite = torch.isfinite(out).all().item()
    d, bar = M.maxdiff(out, ref) if finite else float("inf"), FP32_RTOL * ref.abs().max().item()
    record_parity("conv_variants.f16x3.padding_channels", d, bar, f"finite {finite}, range report {reported}")
    assert finite and not reported and d <= bar
    check_all("ops", "padding_channels", ("sb", "sb3", "f32"), x, w, kw)
