"""The bars of tests/test_gpu_conv_variants.py separate right from wrong before any kernel runs: on the CPU model of csrc/conv.hip (tests/conv_model.py)
the full emulation of every arithmetic and stock fp32 ``F.conv2d`` sit inside the bar of each arithmetic case, and every emulation with one product left
out sits at least twice the bar outside it.  Also: the split and fold primitives of the model, and the table of launches against the dispatch rules."""
import pytest
import torch
import torch.nn.functional as F

import conv_model as M

_CASES = {}


def case(name):
    """One arithmetic case with its float64 reference and its bar, computed once."""
    if name not in _CASES:
        x, w, kw, ariths, via = M.arith_case(name)
        ref = M.reference64(x, w, **kw)
        _CASES[name] = (x, w, kw, ariths, ref, M.fp32_class_bar(ref, x, w, **kw))
    return _CASES[name]


NAMES = [c[0] for c in M.ARITH_CASES]


def test_split_terms_are_the_rounded_running_residuals():
    t = torch.cat([M.randn("sp", (4096,)), M.randn("sp2", (64,)) * 1e-3, torch.tensor([0.0, 1.0, -3.0, 65504.0, 1e5, 2.0 ** -20])])
    for dtype, n in ((torch.bfloat16, 3), (torch.float16, 2)):
        terms = M.split_terms(t, n, dtype)
        r = t.clone()
        for k in terms:
            assert torch.equal(k.to(dtype).float(), k)                       # representable in the narrow format
            assert torch.equal(k, r.to(dtype).float())                       # ... and the round-to-nearest-even of what is left
            r = r - k
    hi, lo = M.split_terms(torch.tensor([1e5, 1.0]), 2, torch.float16)
    assert torch.isinf(hi[0]) and hi[1] == 1.0                               # beyond the f16 range: an infinity, as on the device
    b0, b1, b2 = M.split_terms(t[:4096], 3, torch.bfloat16)
    assert (t[:4096] - (b0 + b1 + b2)).abs().max() <= 2.0 ** -24 * t[:4096].abs().max()      # three bf16 terms carry an fp32 significand
    h0, h1 = M.split_terms(t[:4096], 2, torch.float16)
    big = t[:4096].abs() >= 0.125                                            # where the second term is a normal f16
    assert ((t[:4096] - (h0 + h1)).abs()[big] <= 2.0 ** -22 * t[:4096].abs()[big]).all()


def test_fold_matches_batchnorm_and_kexp_range():
    w = M.randn("fw", (48, 32, 3, 3), 0.06)
    bn = M.seeded_bn("f", 48)
    cb = M.randn("fcb", (48,), 0.3)
    x = M.randn("fx", (1, 32, 9, 9)).double()
    wf, b = M.fold64(w, bn, cb)
    gamma, beta, mean, var, eps = (t.double() if isinstance(t, torch.Tensor) else t for t in bn)
    ref = F.batch_norm(F.conv2d(x, w.double(), cb.double(), padding=1), mean, var, gamma, beta, False, 0.0, eps)
    assert (F.conv2d(x, wf, b, padding=1) - ref).abs().max() <= 1e-12
    w32, b32 = M.fold32(w, bn, cb)
    assert w32.dtype == torch.float32 and (w32.double() - wf).abs().max() <= 2.0 ** -22 * wf.abs().max() and (b32.double() - b).abs().max() <= 1e-6
    k = M.f16_kexp(w, bn)
    assert 2.0 ** 9 < float(wf.abs().max()) * 2.0 ** k <= 2.0 ** 10


@pytest.mark.parametrize("name", NAMES)
def test_bar_lets_the_right_arithmetic_and_stock_fp32_pass(name):
    x, w, kw, ariths, ref, bar = case(name)
    scale = ref.abs().max().item()
    d32 = M.maxdiff(M.stock32(x, w, **kw), ref)
    print(f"{name}: bar {bar:.3e} = {bar / scale:.3e} max|ref|; stock fp32 {d32 / scale:.3e}")
    assert d32 <= bar
    for a in ariths:
        d = M.maxdiff(M.emulate(x, w, a, **kw), ref)
        print(f"  {a}: full emulation {d / scale:.3e} max|ref|")
        if a == "sb":
            assert d > bar                       # two bf16 terms are NOT fp32-class: that kernel is held to its emulation instead
            assert d <= 1e-4 * max(1.0, scale)   # ... and to the suite's split-bf16 tolerance against float64
        else:
            assert d <= bar


@pytest.mark.parametrize("name", NAMES)
def test_every_single_product_mutant_is_twice_the_bar_away(name):
    x, w, kw, ariths, ref, bar = case(name)
    # (the bar IS half the least visible mutant of the three-term split, so for that arithmetic this holds by construction, with equality for one product;
    # the assertion carries information for the two-term bf16, two-term f16 and fp32 mutants)
    for a in ariths:
        full = M.emulate(x, w, a, **kw)
        for pr, err in M.mutant_errors(a, ref, x, w, **kw).items():
            print(f"{name} {a} without {pr}: {err / ref.abs().max().item():.3e} max|ref| = {err / bar:.1f} bars")
            assert err >= 2 * bar, (a, pr)
            if a == "sb":                         # the two-term kernel is compared with its emulation: the mutant must be as far from THAT
                assert M.maxdiff(M.emulate(x, w, a, drop=pr, **kw), full) >= 2 * bar, (a, pr)


@pytest.mark.parametrize("name", NAMES)
def test_a_zeroed_lo_plane_of_one_channel_is_outside_the_bar(name):
    x, w, kw, ariths, ref, bar = case(name)
    full = M.emulate(x, w, "sb", **kw)
    for c in (0, x.shape[1] - 1):
        err = M.maxdiff(M.emulate(x, w, "sb", zero_lo_channel=c, **kw), full)
        print(f"{name}: lo plane of channel {c} zeroed: {err / bar:.1f} bars from the emulation, {err / (1e-4 * max(1.0, ref.abs().max().item())):.2f} of CONV_RTOL")
        assert err >= 2 * bar


def test_table_reaches_every_selectable_instantiation():
    """The launches of the GPU file's tables, put through the mirror of the dispatch rules, reach all 63 kernels the dispatchers can select."""
    want = M.all_instantiations()
    assert len(want) == 63
    got = M.table_kernels("sb")
    assert got == want, (sorted(want - got), sorted(got - want))
    chunks = {}
    for via, a, ks, s, bs, cin, cout, h, w, pad, plain in M.table_launches():
        if via == "ops":
            a = M.route(a, cin, ks)
        name, args = M.select_kernel(a, ks, s, bs, cin, cout, h, w, pad, plain)
        if name == "conv2d_sb_kernel" and args[7] == 2:
            chunks.setdefault(args, set()).add(M.cdiv(cin, 16))
    seen = set().union(*chunks.values())
    assert {1, 2, 3, 4, 5} <= seen, seen                                     # the two-stage prefetch: a lone chunk, odd and even counts
    for _, _, ks, s, pad, bs, cin, cout, h, w in M.INDEX_ROWS:
        ho, wo = M.out_size(h, w, ks, s, pad)
        assert cin <= 80 and 2 * bs * cout * ho * wo * cin * ks * ks <= 2.0e9   # float64 references of a few seconds at the most
