"""Every tile and route of the split-bf16 modulated convolution (csrc/modconv_sb.hip, csrc/modconv_upfused.hip) against float64 and against the CPU model of
tests/modconv_model.py, through the ``ops`` wrappers with explicit fp32 ``s``, ``d``, labels and noise.

A. arithmetic cases (K = 144): each route against the float64-accumulated emulation of its own arithmetic at ``fp32_class_bar`` — HALF the error of the least
   visible single-product mutant of a three-term split, which tests/test_modconv_model_cpu.py shows to separate right from wrong on the CPU alone — and against
   float64 at the suite's layer bar.
B. indexing cases: the smallest launches that make the three launchers select each of their 39 kernel instantiations, ragged in every dimension, at the same
   two bars; fused ToRGB images, split-plane and channel-blocked outputs included.
C. one test reads the kernel names of the whole table from torch.profiler and compares them with the list written here.
D. bit-for-bit properties; E. ``style_demod`` against float64; F. the refusals of the three entry points."""
import re

import pytest
import torch

import modconv_model as M
from conftest import record_parity
from e4s2024_amd import _lib, ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ops.MODCONV_MODE != "sb", reason="these kernels are the split-bf16 route (E4S_MODCONV=f32 switches them off)")]
DEV = "cuda:0"
WORST = {}          # kernel label -> worst error / bar so far, against the emulation and against float64


def dev(t):
    return None if t is None else t.to(DEV)


def launch(c, x=None, noise="own", bs=None):
    """One row through its wrapper.  Returns {"out": activation [bs, cout, ho, wo] (None if not wanted), "rgb": fused ToRGB image or None, "raw": the tensor the
    wrapper returned}; split-plane and channel-blocked outputs come back converted (``from_split_planes``: the value still carries ``s_next``)."""
    sl = slice(None) if bs is None else bs
    up_conv = c["up"] and c["route"] == "conv"
    W = dev(c["W"][None])
    blur = dev(c["blur"])
    with torch.no_grad():
        wt, _ = ops.PreparedWeights().get(W, blur if up_conv else None, up_conv, False, tconv=c["route"] != "conv")
    x = dev(c["x"][sl]) if x is None else x
    s, d = dev(c["s"][sl]), dev(None if c["d"] is None else c["d"][sl])
    nz = c["noise"] if isinstance(noise, str) else noise
    if isinstance(noise, str) and nz is not None and nz.shape[0] > 1:
        nz = nz[sl]
    nz, nw, ab = dev(nz), dev(c["noise_weight"]), dev(c["bias"])
    sn = dev(None if c["sn"] is None else c["sn"][sl][:, None])
    res = dict(out=None, rgb=None)
    if c["route"] == "conv":
        rgb = None
        if c["rgb"] is not None:
            r = c["rgb"]
            with torch.no_grad():
                r_wt, _ = ops.PreparedWeights().get(dev(r["w"][None, :, :, None, None]), None, False, False)
            rgb = (r_wt, dev(r["s"][sl][:, None]), dev(r["bias"].reshape(1, 3, 1, 1)), dev(None if r["skip"] is None else r["skip"][sl]), dev(r["upk"]))
        xin = M.to_blocked(x) if c["x_nhwc"] else x
        raw = ops.region_modconv3x3(xin, wt, s, d, dev(None if c["labels"] is None else c["labels"][sl]), nz, nw, ab, c["act"], c["cout"], up_conv, rgb=rgb,
                                    want_out=c["want_out"], x_nhwc=c["x_nhwc"], out_nhwc=c["out_nhwc"], s_next=sn)
        out = raw
        if rgb is not None:
            out, res["rgb"] = raw
    else:
        old = ops.UP_FUSED
        ops.UP_FUSED = c["route"] != "tconv"
        try:
            if c["route"] == "fused_sp":
                xin = ops.to_split_planes(x, s)
            else:
                xin = M.to_blocked(x) if c["x_nhwc"] else x
            out = raw = ops.modconv_up_single(xin, wt, s, d, blur, nz, nw, ab, c["act"], c["cout"], x_nhwc=c["x_nhwc"], out_nhwc=c["out_nhwc"], s_next=sn)
        finally:
            ops.UP_FUSED = old
    res["raw"] = raw
    if out is not None:
        res["out"] = ops.from_split_planes(out) if sn is not None else (M.from_blocked(out) if c["out_nhwc"] else out)
    return res


def kernel_of(row):
    return M.kernel_label(*M.select_kernel(**M.launch_of(row))[:2])


def note_worst(label, kind, ratio):
    key = (label, kind)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    record_parity(f"modconv_variants.worst.{label}.{kind}", WORST[key], 1.0, "worst error / bar of this kernel so far")


def check_row(row):
    """One row against its emulation at ``fp32_class_bar`` and against float64 at the layer bar (the fused ToRGB image at the ToRGB bar); every distance is
    recorded before anything is asserted."""
    c = M.case(row)
    res = launch(c)
    full = res
    if not c["want_out"]:             # a row that wants the image only: asked for both, the same launch must give the same image bits, and its activation is checked too
        full = launch(dict(c, want_out=True))
        assert res["out"] is None and torch.equal(full["rgb"], res["rgb"])
    ref_act, emu_act = M.reference64(c), M.emulate(c)
    label, tag = kernel_of(row), row["id"]
    bad = []
    ho, wo = M.out_hw(c)
    if full["out"] is not None:
        out = full["out"].double().cpu()
        assert tuple(out.shape) == (c["bs"], c["cout"], ho, wo)
        if c["sn"] is not None:
            # split planes hold fl32(act * s_next) as bf16 hi + lo: a value rounded to two bf16 terms is within 2^-16 of itself, on top of the bar
            post = lambda v: M.split_planes_value(c, v, exact=True)       # noqa: E731
            ref, emu = post(ref_act), M.split_planes_value(c, emu_act)
            bar = M.fp32_class_bar(ref, c, post)
            demu = ((out - emu).abs() - 2.0 ** -16 * emu.abs()).clamp(min=0).max().item()
            d64 = ((out - ref).abs() - 2.0 ** -16 * ref.abs()).clamp(min=0).max().item()
        else:
            ref, emu = ref_act, emu_act
            bar = M.fp32_class_bar(ref, c)
            demu, d64 = M.maxdiff(out, emu), M.maxdiff(out, ref)
        lbar = M.layer_bar(ref)
        record_parity(f"modconv_variants.{tag}.vs_emulation", demu, bar, f"{label}; bar = {bar / ref.abs().max().item():.2e} of max|ref|")
        record_parity(f"modconv_variants.{tag}.vs_float64", d64, lbar, label)
        note_worst(label, "vs_emulation", demu / bar)
        note_worst(label, "vs_float64", d64 / lbar)
        if not (torch.isfinite(out).all().item() and demu <= bar and d64 <= lbar):
            bad.append(("activation", demu, bar, d64, lbar))
    if res["rgb"] is not None:
        img = res["rgb"].double().cpu()
        ref_rgb = M.to_rgb64(c, ref_act)
        assert tuple(img.shape) == tuple(ref_rgb.shape) == (c["bs"], 3, ho, wo)
        drgb, rbar = M.maxdiff(img, ref_rgb), M.RGB_TOL * max(1.0, ref_rgb.abs().max().item())
        record_parity(f"modconv_variants.{tag}.rgb_vs_float64", drgb, rbar, label)
        note_worst(label, "rgb_vs_float64", drgb / rbar)
        if not (torch.isfinite(img).all().item() and drgb <= rbar):
            bad.append(("rgb", drgb, rbar))
    assert not bad, bad
    return res


# ------------------------------------------------------------------------------------------------ A. arithmetic
@pytest.mark.parametrize("row", M.ARITH_CASES, ids=[r["id"] for r in M.ARITH_CASES])
def test_arithmetic_against_emulation_and_float64(row):
    """Worst measured share of the bar on an MI355X over the five cases: 0.22 against the emulation (``up_masked``; 0.14 .. 0.22: the fp32 accumulation of the MFMA
    chain, as the fp32-accumulated emulation predicts on the CPU, 0.13 .. 0.15) and 0.028 against float64 at the layer bar.  The emulation has to place two
    roundings as the compiler does — the masked kernels' ``x * s - hi`` and the parity weights' ``v += blur * w`` are contracted into FMAs
    (``modconv_model.split_product``, ``compose32``); with the products rounded first the masked and the composed up cases measured 1.0 .. 2.1 bars."""
    check_row(row)


# ------------------------------------------------------------------------------------------------ B. indexing
@pytest.mark.parametrize("row", M.INDEX_ROWS, ids=[r["id"] for r in M.INDEX_ROWS])
def test_every_tile_against_emulation_and_float64(row):
    """Worst measured share of the bar on an MI355X over the 40 rows: 0.30 against the emulation (``w9_masked_up``; single-region 0.17 .. 0.28, masked
    0.08 .. 0.30, the cin = 130 split-K rows 0.19 .. 0.24) and 0.042 against float64 at the layer bar (``w17_masked_c128_up``)."""
    check_row(row)


@pytest.mark.parametrize("row", M.VARIANT_ROWS, ids=[r["id"] for r in M.VARIANT_ROWS])
def test_every_variant_against_emulation_and_float64(row):
    """Worst measured share of the bar on an MI355X over the 30 rows: 0.35 against the emulation (``fused_15x17_c33_k130``: 1170 products in one fp32
    accumulator, no split-K; the transposed-conv pair 0.11 .. 0.30, the one-launch up kernel 0.11 .. 0.35, its split-plane forms 0.05 .. 0.06, the fused-ToRGB
    and channel-blocked rows 0.18 .. 0.33, split-plane outputs of the masked layer 0.04 .. 0.05), 0.034 against float64 at the layer bar, and the fused ToRGB
    images 0.12 .. 0.21 of the ToRGB bar.
    The fused ToRGB image is held to the float64 ToRGB of the reference activation (no test asserts it bit-equal to ``region_torgb`` of the kernel's own output:
    the two sum the channels in different orders).  The split planes the up kernel is fed (``ops.to_split_planes``) are, bit for bit, the model's."""
    c = M.case(row)
    if c["route"] == "fused_sp":
        planes = ops.to_split_planes(dev(c["x"]), dev(c["s"]))
        assert torch.equal(planes.cpu(), M.split_planes_of(c["x"], c["s"]))
    res = check_row(row)
    if c["rgb"] is not None and not c["want_out"]:
        assert res["out"] is None
    if c["sn"] is not None:
        planes = res["raw"][0] if c["route"] == "conv" else res["raw"]
        assert planes.dtype == torch.int16 and tuple(planes.shape) == (2, c["bs"], c["cout"] // 8) + M.out_hw(c) + (8,)


# ------------------------------------------------------------------------------------------------ C. coverage
# the kernels the three launchers can select: <CB, PB, WC, WP, LOG_TW, MINW, UNI, TCONV, RGB, XN, OSP> of region_modconv_sb_kernel, <CB, MINW, XN, ON, XSP, OSP> of
# up_fused_sb_kernel
KERNELS = """
region_modconv_sb_kernel<2, 2, 1, 4, 6, 2, 1, 0, 0, 0, 0> region_modconv_sb_kernel<1, 2, 1, 4, 6, 2, 1, 0, 0, 0, 0>
region_modconv_sb_kernel<2, 2, 1, 4, 5, 2, 1, 0, 0, 0, 0> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 1, 0, 0, 0, 0>
region_modconv_sb_kernel<1, 2, 2, 2, 4, 2, 1, 0, 0, 0, 0> region_modconv_sb_kernel<1, 1, 2, 2, 3, 2, 1, 0, 0, 0, 0> region_modconv_sb_kernel<1, 1, 2, 2, 2, 2, 1, 0, 0, 0, 0>
region_modconv_sb_kernel<2, 2, 1, 4, 5, 2, 0, 0, 0, 0, 0> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 0, 0, 0, 0, 0>
region_modconv_sb_kernel<1, 2, 2, 2, 4, 2, 0, 0, 0, 0, 0> region_modconv_sb_kernel<1, 1, 2, 2, 3, 2, 0, 0, 0, 0, 0> region_modconv_sb_kernel<1, 1, 2, 2, 2, 2, 0, 0, 0, 0, 0>
region_modconv_sb_kernel<4, 1, 1, 8, 5, 2, 0, 0, 0, 0, 0> region_modconv_sb_kernel<4, 1, 1, 8, 4, 2, 0, 0, 0, 0, 0>
region_modconv_sb_kernel<2, 2, 1, 4, 5, 2, 1, 0, 0, 1, 0> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 1, 0, 0, 1, 0>
region_modconv_sb_kernel<2, 2, 1, 4, 5, 2, 1, 0, 1, 1, 0> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 1, 0, 1, 1, 0>
region_modconv_sb_kernel<2, 2, 1, 4, 6, 2, 1, 0, 1, 0, 0> region_modconv_sb_kernel<1, 2, 1, 4, 6, 2, 1, 0, 1, 0, 0>
region_modconv_sb_kernel<2, 2, 1, 4, 5, 2, 1, 0, 1, 0, 0> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 1, 0, 1, 0, 0>
region_modconv_sb_kernel<4, 1, 1, 8, 5, 2, 0, 0, 1, 0, 0>
region_modconv_sb_kernel<2, 2, 1, 4, 5, 2, 0, 0, 1, 0, 0> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 0, 0, 1, 0, 0>
region_modconv_sb_kernel<4, 1, 1, 8, 5, 2, 0, 0, 1, 0, 1>
region_modconv_sb_kernel<2, 2, 1, 4, 5, 2, 0, 0, 1, 0, 1> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 0, 0, 1, 0, 1>
region_modconv_sb_kernel<2, 1, 1, 4, 5, 2, 1, 1, 0, 0, 0> region_modconv_sb_kernel<1, 2, 1, 4, 5, 2, 1, 1, 0, 0, 0> region_modconv_sb_kernel<1, 1, 2, 2, 4, 2, 1, 1, 0, 0, 0>
modconv_sb_finalize_kernel blur_epilogue_kernel up_fused_dma_kernel
up_fused_sb_kernel<1, 4, 0, 0, 0, 0> up_fused_sb_kernel<1, 4, 1, 0, 0, 0> up_fused_sb_kernel<1, 4, 0, 1, 0, 0> up_fused_sb_kernel<1, 4, 1, 1, 0, 0> up_fused_sb_kernel<1, 4, 0, 1, 1, 1>
"""
N_KERNELS = 39
_TEMPLATED = re.compile(r"\b(region_modconv_sb_kernel|up_fused_sb_kernel)<([^<>]*)>")
_PLAIN = ("modconv_sb_finalize_kernel", "blur_epilogue_kernel", "up_fused_dma_kernel")
_BOOL = {"true": "1", "false": "0"}


def kernel_set(text):
    """Kernel labels named in ``text`` (profiler keys or the list above); a template's bools as 0 / 1."""
    out = set()
    for name, args in _TEMPLATED.findall(text):
        toks = [a.replace("(bool)", "").strip() for a in args.split(",")]
        out.add(f"{name}<{', '.join(_BOOL.get(t, t) for t in toks)}>")
    for name in _PLAIN:
        if re.search(r"\b" + name + r"\b", text):
            out.add(name)
    return out


def test_table_runs_every_selectable_kernel():
    """The launches of the three tables under torch.profiler: the kernel names seen are exactly the 39 instantiations written above — the non-DMA split-plane
    up kernel ``up_fused_sb_kernel<1, 4, false, true, true, true>`` among them — so a retuned threshold that drops a configuration from this file's coverage
    fails here."""
    from torch.profiler import profile, ProfilerActivity
    want = kernel_set(KERNELS)
    assert len(want) == N_KERNELS and want == {M.kernel_label(*k) for k in M.all_instantiations()}
    cases = [M.case(r) for r in M.ALL_ROWS]
    launch(cases[0])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for c in cases:
            launch(c)
        torch.cuda.synchronize()
    events = [(e.key, e.count) for e in prof.key_averages()]
    seen = kernel_set("\n".join(k for k, _ in events))
    templated = {s for s in seen if "<" in s}
    record_parity("modconv_variants.coverage.instantiations_named_by_profiler", len(templated), N_KERNELS - len(_PLAIN))
    if not templated:
        # a profiler build that strips template arguments (recorded above as 0 named instantiations): the table is held to the mirror of the dispatch rules in
        # tests/modconv_model.py, and every launch of the table must show up under the base name of the kernel the mirror predicts
        predicted = {}
        for ln in M.table_launches():
            for name, _ in M.launched(**ln):
                predicted[name] = predicted.get(name, 0) + 1
        counts = {base: sum(n for k, n in events if re.search(r"\b" + base + r"\b", k)) for base in predicted}
        assert counts == predicted, (counts, predicted)
        seen = {M.kernel_label(*k) for k in M.table_kernels()}
    assert seen == want, (sorted(want - seen), sorted(seen - want))


# ------------------------------------------------------------------------------------------------ D. bit-for-bit properties
@pytest.mark.parametrize("name", M.PROPERTY_ROWS)
def test_bitwise_properties(name):
    """Two runs are equal; a batch equals its samples run singly (the split-K factor of these rows does not depend on the batch: asserted on the mirror); an input
    at a 4-byte but not 16-byte aligned address gives the same bits; one noise map equals the same map repeated for every sample."""
    row = M.ROW[name]
    c = M.case(row)
    assert c["bs"] > 1 and c["noise"].shape[0] == c["bs"]
    a = launch(c)["out"]
    assert torch.equal(a, launch(c)["out"])
    ln = M.launch_of(row)
    single = dict(ln, bs=1, workspace=ln["workspace"] // c["bs"])
    assert M.select_kernel(**single) == M.select_kernel(**ln)
    for b in range(c["bs"]):
        assert torch.equal(launch(c, bs=slice(b, b + 1))["out"][0], a[b]), b
    x = dev(c["x"])
    buf = torch.empty(x.numel() + 4, device=DEV)
    xm = buf[1:1 + x.numel()].view(x.shape)
    xm.copy_(x)
    assert xm.data_ptr() % 16 == 4 and xm.is_contiguous()
    assert torch.equal(launch(c, x=xm)["out"], a)
    one = c["noise"][:1]
    assert torch.equal(launch(c, noise=one)["out"], launch(c, noise=one.expand(c["bs"], -1, -1, -1).contiguous())["out"])


def test_empty_batch():
    """bs = 0 gives an empty tensor of the right shape from every entry point (an empty tensor has no storage: the entry points see null pointers)."""
    e = lambda *shape: torch.zeros(shape, device=DEV)       # noqa: E731
    cin, cout, h, w = 16, 24, 9, 36
    W, blur = dev(M.randn("e_W", (1, cout, cin, 3, 3))), dev(M.blur_kernel())
    nw, ab = torch.tensor([0.2], device=DEV), e(cout)
    with torch.no_grad():
        wt, wsq = ops.PreparedWeights().get(W, None, False, True)
        wt_up, _ = ops.PreparedWeights().get(W, blur, True, False)
        wt_t, _ = ops.PreparedWeights().get(W, None, False, False, tconv=True)
        r_wt, _ = ops.PreparedWeights().get(dev(M.randn("e_rw", (1, 3, cout, 1, 1))), None, False, False)
    s, d = e(0, 1, cin), e(0, 1, cout)
    lab = torch.zeros((0, 5, 7), dtype=torch.uint8, device=DEV)
    assert tuple(ops.region_modconv3x3(e(0, cin, h, w), wt, s, d, None, e(1, 1, h, w), nw, ab, True, cout, False).shape) == (0, cout, h, w)
    assert tuple(ops.region_modconv3x3(e(0, cin, h, w), wt, e(0, 3, cin), e(0, 3, cout), lab, None, nw, ab, True, cout, False).shape) == (0, cout, h, w)
    assert tuple(ops.region_modconv3x3(e(0, cin, h, w), wt_up, s, d, None, None, nw, ab, True, cout, True).shape) == (0, cout, 2 * h, 2 * w)
    rgb = (r_wt, e(0, 1, cout), e(1, 3, 1, 1), None, None)
    out, img = ops.region_modconv3x3(e(0, cin, h, w), wt, s, d, None, None, nw, ab, True, cout, False, rgb=rgb)
    assert tuple(out.shape) == (0, cout, h, w) and tuple(img.shape) == (0, 3, h, w)
    out, img = ops.region_modconv3x3(e(0, cin, h, w), wt, e(0, 3, cin), e(0, 3, cout), lab, None, nw, ab, True, cout, False, rgb=rgb, s_next=e(0, 1, cout))
    assert tuple(out.shape) == (2, 0, cout // 8, h, w, 8) and tuple(img.shape) == (0, 3, h, w)
    assert tuple(ops.region_modconv3x3(e(0, cin // 8, h, w, 8), wt, s, d, None, None, nw, ab, True, cout, False, x_nhwc=True, out_nhwc=True).shape) == (0, cout // 8, h, w, 8)
    old = ops.UP_FUSED
    try:
        for fused in (True, False):
            ops.UP_FUSED = fused
            assert tuple(ops.modconv_up_single(e(0, cin, h, w), wt_t, s, d, blur, None, nw, ab, True, cout).shape) == (0, cout, 2 * h, 2 * w)
        ops.UP_FUSED = True
        xsp = ops._alloc_split_planes(0, cin, h, w, DEV)
        assert tuple(ops.modconv_up_single(xsp, wt_t, s, d, blur, None, nw, ab, True, cout, s_next=e(0, 1, cout)).shape) == (2, 0, cout // 8, 2 * h, 2 * w, 8)
    finally:
        ops.UP_FUSED = old
    assert tuple(ops.region_torgb(e(0, cout, h, w), r_wt, e(0, 1, cout), None, e(3), None, None).shape) == (0, 3, h, w)
    s0, d0 = ops.style_demod(e(0, 3, 512), e(cin, 512), e(cin), wsq, cout)
    assert tuple(s0.shape) == (0, 3, cin) and tuple(d0.shape) == (0, 3, cout)
    assert tuple(ops.from_split_planes(xsp).shape) == (0, cin, h, w)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ E. style_demod
@pytest.mark.parametrize("row", M.STYLE_ROWS, ids=["x".join(map(str, r)) for r in M.STYLE_ROWS])
def test_style_demod_against_float64(row):
    """s and d against float64 at elementwise bars from the model (``style_demod_bar``: roundings on the longest path times 2^-24 times the sum of magnitudes; the
    relative error of the sum under the reciprocal square root is halved, ``rsqrtf`` adds 2 ulp).  Worst measured share of the bar on an MI355X: s 0.024, d 0.013
    (the bars count every rounding of the longest path at its worst; the kernels' errors are those of a random walk)."""
    sc = M.style_case(row)
    s, d = ops.style_demod(dev(sc["styles"]), dev(sc["mw"]), dev(sc["mb"]), dev(sc["wsq"]), sc["cout"])
    s64, d64 = M.style_demod64(sc)
    bar_s, bar_d = M.style_demod_bar(sc)
    assert tuple(s.shape) == tuple(s64.shape) and tuple(d.shape) == tuple(d64.shape)
    rs = ((s.double().cpu() - s64).abs() / bar_s).max().item()
    rd = ((d.double().cpu() - d64).abs() / bar_d).max().item()
    tag = "x".join(map(str, row))
    record_parity(f"modconv_variants.style_demod.{tag}.s", rs, 1.0, "worst error / bar")
    record_parity(f"modconv_variants.style_demod.{tag}.d", rd, 1.0, "worst error / bar")
    note_worst("style_kernel", "vs_float64", rs)
    note_worst("demod_kernel", "vs_float64", rd)
    assert rs <= 1.0 and rd <= 1.0, (rs, rd)
    s_only, none = ops.style_demod(dev(sc["styles"]), dev(sc["mw"]), dev(sc["mb"]), None, sc["cout"])
    assert none is None and torch.equal(s_only, s)


# ------------------------------------------------------------------------------------------------ F. refusals
def test_refusals_raise_before_anything_launches():
    """The argument checks of the three entry points no other test reaches: each raises, and the output the call would have written keeps its bits."""
    g = lambda key, *shape: dev(M.randn("rf_" + key, shape))       # noqa: E731
    bs, cin, cout, h, w = 2, 16, 24, 9, 36
    W, blur = g("W", 1, cout, cin, 3, 3), dev(M.blur_kernel())
    with torch.no_grad():
        wt, _ = ops.PreparedWeights().get(W, None, False, False)
        wt_t, _ = ops.PreparedWeights().get(W, None, False, False, tconv=True)
        r_wt, _ = ops.PreparedWeights().get(g("rw", 1, 3, cout, 1, 1), None, False, False)
    x, s, d = g("x", bs, cin, h, w), g("s", bs, 1, cin), g("d", bs, 1, cout)
    s3, d3 = g("s3", bs, 3, cin), g("d3", bs, 3, cout)
    lab = torch.zeros((bs, 5, 7), dtype=torch.uint8, device=DEV)
    nw, ab = torch.tensor([0.2], device=DEV), g("ab", cout)
    rgb = (r_wt, g("rs", bs, 1, cout), g("rb", 1, 3, 1, 1), None, None)
    refused = (RuntimeError, ValueError)
    with pytest.raises(refused):      # channel-blocked input with labels
        ops.region_modconv3x3(M.to_blocked(x), wt, s3, d3, lab, None, nw, ab, True, cout, False, x_nhwc=True)
    with pytest.raises(refused):      # ... and with a fused ToRGB
        ops.region_modconv3x3(M.to_blocked(x), wt, s3, d3, lab, None, nw, ab, True, cout, False, x_nhwc=True, rgb=rgb)
    with pytest.raises(refused):      # fused ToRGB below 32 pixels of width
        ops.region_modconv3x3(x[..., :31].contiguous(), wt, s, d, None, None, nw, ab, True, cout, False, rgb=rgb)
    with torch.no_grad():
        wt_up, _ = ops.PreparedWeights().get(W, blur, True, False)
    with pytest.raises(refused):      # fused ToRGB on an up layer
        ops.region_modconv3x3(x, wt_up, s, d, None, None, nw, ab, True, cout, True, rgb=rgb)
    with pytest.raises(refused):      # fused ToRGB with more output channels than a workgroup tile
        W72 = g("W72", 1, 72, cin, 3, 3)
        with torch.no_grad():
            wt72, _ = ops.PreparedWeights().get(W72, None, False, False)
            r72, _ = ops.PreparedWeights().get(g("rw72", 1, 3, 72, 1, 1), None, False, False)
        ops.region_modconv3x3(x, wt72, s, g("d72", bs, 1, 72), None, None, nw, g("ab72", 72), True, 72, False, rgb=(r72, g("rs72", bs, 1, 72), rgb[2], None, None))
    with pytest.raises(refused):      # split-plane hand-over without the fused ToRGB
        ops.region_modconv3x3(x, wt, s3, d3, lab, None, nw, ab, True, cout, False, s_next=g("sn", bs, 1, cout))
    with pytest.raises(refused):      # split-plane hand-over of a single-region layer
        ops.region_modconv3x3(x, wt, s, d, None, None, nw, ab, True, cout, False, rgb=rgb, s_next=g("sn", bs, 1, cout))
    for nbs in (3, 4):                # noise batch neither 1 nor bs
        with pytest.raises(refused):
            ops.region_modconv3x3(x, wt, s, d, None, g("n", nbs, 1, h, w), nw, ab, True, cout, False)
        with pytest.raises(refused):
            ops.modconv_up_single(x, wt_t, s, d, blur, g("n2", nbs, 1, 2 * h, 2 * w), nw, ab, True, cout)
    with pytest.raises(refused):      # more regions than the kernels hold
        ops.region_modconv3x3(x, wt, g("s17", bs, 17, cin), g("d17", bs, 17, cout), lab, None, nw, ab, True, cout, False)
    with pytest.raises(refused):      # several regions without a label map
        ops.region_modconv3x3(x, wt, s3, d3, None, None, nw, ab, True, cout, False)
    with pytest.raises(refused):      # channel-blocked activations of the up kernel need cin % 16 == 0
        ops.modconv_up_single(g("x20", bs, 3, h, w, 8), wt_t, g("s24", bs, 1, 24), d, blur, None, nw, ab, True, cout, x_nhwc=True)
    # split planes on one side only of the one-launch up kernel: the wrapper always sets both, so the entry point is called as the wrapper calls it
    out = torch.full((bs, cout, 2 * h, 2 * w), 7.0, device=DEV)
    xsp = ops.to_split_planes(x, s)
    call = _lib.lib().call
    for flags, xin in ((ops.X_SP, xsp), (ops.OUT_SP, x)):
        with pytest.raises(RuntimeError, match="split"):
            call("e4s_modconv_up_fused_sb", ops._p(out), ops._p(xin), ops._p(wt_t[0]), ops._p(wt_t[1]), ops._p(s), ops._p(d), ops._p(blur), None, 0, None, ops._p(ab),
                 1 | flags, bs, cin, cout, h, w, ops._p(g("sn2", bs, cout)), ops._stream())
    with pytest.raises(RuntimeError, match="one layout per side"):
        call("e4s_modconv_up_fused_sb", ops._p(out), ops._p(xsp), ops._p(wt_t[0]), ops._p(wt_t[1]), ops._p(s), ops._p(d), ops._p(blur), None, 0, None, ops._p(ab),
             1 | ops.X_SP | ops.X_NHWC, bs, cin, cout, h, w, None, ops._stream())
    torch.cuda.synchronize()
    assert (out == 7.0).all().item()
