"""The bars of tests/test_gpu_modconv_variants.py separate right from wrong before any kernel runs: on the CPU model of the split-bf16 modulated convolution
(tests/modconv_model.py) the float64 reference is the oracle's layer, stock fp32 and the emulation sit inside the layer bar, the fp32-accumulated emulation sits
inside ``fp32_class_bar`` of the emulation, and every mutant sits at least twice its bar outside.  Also: the label sampler, the table of launches against the
mirror of the dispatch rules, and the ``style_demod`` bars."""
import math

import pytest
import torch
import torch.nn.functional as F

import modconv_model as M
from oracle import e4s_oracle as O

IDS = [r["id"] for r in M.ALL_ROWS]
_REF = {}


def ref_of(row):
    """(case, float64 reference, emulation, fp32-class bar) of one row, computed once."""
    if row["id"] not in _REF:
        c = M.case(row)
        ref = M.reference64(c)
        _REF[row["id"]] = (c, ref, M.emulate(c), M.fp32_class_bar(ref, c))
    return _REF[row["id"]]


def oracle_layer(c, dtype):
    """``oracle.e4s_oracle.styled_conv`` on the case: the styles are unit vectors that pick the case's ``s`` out of the modulation weight, the mask is the one-hot
    form of the labels (label 255: no class set)."""
    bs, nr, cin = c["s"].shape
    sdim = bs * nr
    mw = c["s"].reshape(sdim, cin).T.to(dtype)                                                        # equal_linear: style @ (mw / sqrt(sdim)).T
    style = (torch.eye(sdim, dtype=dtype) * math.sqrt(sdim)).reshape(bs, nr, sdim)
    sd = {"conv.weight": c["W"][None].to(dtype), "conv.modulation.weight": mw, "conv.modulation.bias": torch.zeros(cin, dtype=dtype),
          "conv.blur.kernel": c["blur"].to(dtype), "noise.weight": c["noise_weight"].to(dtype), "activate.bias": c["bias"].to(dtype)}
    ho, wo = M.out_hw(c)
    noise = c["noise"].to(dtype) if c["noise"] is not None else torch.zeros((1, 1, ho, wo), dtype=dtype)
    mask = None
    if c["masked"]:
        mask = torch.stack([(c["labels"] == r) for r in range(nr)], 1).to(dtype)
    return O.styled_conv(sd, "", c["x"].to(dtype), style if c["masked"] else style[:, 0], mask, noise, masked=c["masked"], upsample=c["up"])


@pytest.mark.parametrize("row", M.ALL_ROWS, ids=IDS)
def test_reference_is_the_oracle_and_the_bars_let_the_right_arithmetic_pass(row):
    c, ref, emu, bar = ref_of(row)
    lbar = M.layer_bar(ref)
    scale = ref.abs().max().item()
    if c["d"] is not None and c["act"]:                  # (the oracle's layer always demodulates and activates)
        d_or = M.maxdiff(oracle_layer(c, torch.float64), ref)
        assert d_or <= 2.0 ** -23 * scale, d_or              # (the case hands d over rounded to fp32, the oracle forms it in float64)
        assert M.maxdiff(oracle_layer(c, torch.float32), ref) <= lbar
    d32, demu, d32acc = M.maxdiff(M.stock32(c), ref), M.maxdiff(emu, ref), M.maxdiff(M.emulate32(c), emu)
    print(f"{row['id']}: bar {bar:.3e} = {bar / scale:.3e} max|ref|; stock fp32 {d32 / bar:.2f} bars, emulation {demu / lbar:.3f} layer bars = {demu / bar:.1f} bars, "
          f"fp32-accumulated emulation {d32acc / bar:.2f} bars from the emulation")
    assert d32 <= bar and d32 <= lbar
    assert demu <= lbar
    assert demu > bar                                    # two bf16 terms are NOT fp32-class: the kernel is held to its emulation at this bar, not to float64
    assert d32acc <= bar
    assert 4 * bar <= lbar                               # the new bar is the tight one


# ------------------------------------------------------------------------------------------------ mutants
def _applies(name, r):
    up, same = r["up"], not r["up"]
    return {
        "region of the input pixel": r["masked"] and same,
        "labels sampled with round": r["masked"],
        "label 255 counted as region 0": r["masked"],
        "d of the wrong region": r["masked"] and r["d"],
        "up: region of the position": r["masked"] and up,
        "up: blur not flipped": up, "up: blur pad (2, 0)": up, "up: parities swapped": up,
        "noise batch stride 0": r["noise"] == 2 and r["bs"] > 1,
        "noise weight after the activation": r["noise"] > 0 and r["act"],
        "leaky slope 0.01": r["act"], "sqrt(2) gain missing": r["act"],
        "last K chunk lost": r["cin"] > 16,
        "right boundary tap clamped": same,
        "ToRGB skip pad (1, 2)": r["rgb"] == "skip",
        "split planes without s_next": r["s_next"],
    }[name]


@pytest.mark.parametrize("name", [n for n, (_, kind) in M.MUTANTS.items() if kind == "arith"])
def test_every_lost_product_is_twice_the_bar_from_the_emulation(name):
    kw, _ = M.MUTANTS[name]
    for row in M.ARITH_CASES + [M.ROW[n] for n in M.PROPERTY_ROWS]:
        c, ref, emu, bar = ref_of(row)
        err = M.maxdiff(M.emulate(c, **kw), emu)
        print(f"{name} on {row['id']}: {err / bar:.0f} bars from the emulation, {err / M.layer_bar(ref):.2f} layer bars")
        assert err >= 2 * bar, row["id"]


@pytest.mark.parametrize("name", [n for n, (_, kind) in M.MUTANTS.items() if kind == "index"])
def test_every_indexing_mutant_is_twice_the_bar_away(name):
    """Every row of the GPU tables the mutant applies to is tried; it must be two layer bars (ToRGB: two ToRGB bars) from the float64 reference on at least one,
    and is on nearly all: the count is printed."""
    kw, _ = M.MUTANTS[name]
    rows = [r for r in M.ALL_ROWS if _applies(name, r)]
    assert rows
    hit = []
    for row in rows:
        c, ref, emu, bar = ref_of(row)
        if "skip_pad" in kw:
            good = M.to_rgb64(c, ref)
            err, lim = M.maxdiff(M.to_rgb64(c, ref, **kw), good), M.RGB_TOL * max(1.0, good.abs().max().item())
        elif "no_s_next" in kw:
            good = M.split_planes_value(c, ref, exact=True)
            err, lim = M.maxdiff(M.split_planes_value(c, ref, exact=True, **kw), good), M.layer_bar(good) + 2.0 ** -16 * good.abs().max().item()
        else:
            err, lim = M.maxdiff(M.reference64(c, **kw), ref), M.layer_bar(ref)
        assert lim >= bar
        if err >= 2 * lim:
            hit.append(row["id"])
    print(f"{name}: two bars away on {len(hit)} of {len(rows)} rows")
    assert hit
    # the mutants the emulation can take as well give the same distance there: the emulation is the reference up to a hundredth of the layer bar
    if set(kw) <= {"label_round", "none_is_zero", "d_shift", "swap_parity", "lose_last_chunk", "noise_stride0", "noise_after_act", "slope", "gain"}:
        c, ref, emu, bar = ref_of(M.ROW[hit[0]])
        assert M.maxdiff(M.emulate(c, **kw), emu) >= 2 * M.layer_bar(ref)


def test_a_short_split_k_slice_and_a_wrong_tap_exceed_the_tight_bar_by_far():
    """What the layer bar lets through only just and the emulation bar does not: one lost chunk of nine, one clamped tap column."""
    c, ref, emu, bar = ref_of(M.ROW["w7_masked_k130"])
    for kw in (dict(lose_last_chunk=True), dict(clamp_right=True)):
        err = M.maxdiff(M.reference64(c, **kw), ref)
        print(f"{kw}: {err / M.layer_bar(ref):.0f} layer bars, {err / bar:.0f} emulation bars")
        assert err >= 100 * bar


# ------------------------------------------------------------------------------------------------ primitives
def test_label_sampler_is_nearest_interpolation():
    shapes = {(r["lh"], r["lw"]) + M.out_hw(r) for r in M.ALL_ROWS if r["masked"]}
    assert len(shapes) >= 8
    for lh, lw, ho, wo in shapes:
        lab = (torch.arange(lh * lw, dtype=torch.float32) % 251).reshape(1, 1, lh, lw)
        want = F.interpolate(lab, size=(ho, wo), mode="nearest")[0, 0].long()
        iy, ix = M.nearest_src(ho, lh), M.nearest_src(wo, lw)
        assert torch.equal(lab[0, 0].long()[iy][:, ix], want), (lh, lw, ho, wo)
    assert any(lh / ho != lh // ho for lh, lw, ho, wo in shapes)           # ratios that are no integers
    assert not torch.equal(M.nearest_src(19, 21), M.nearest_src(19, 21, rounded=True))


def test_the_contracted_split_differs_from_the_plain_one_at_ties_only():
    x, s = M.randn("spx", (1 << 16,)), M.randn("sps", (1 << 16,), 0.3) + 1
    hi, lo = M.split_product(x, s)
    h0, l0 = M.split_terms(x * s, 2, torch.bfloat16)
    assert torch.equal(hi, h0)
    n = (lo != l0).sum().item()
    print(f"{n} of {x.numel()} second terms differ")
    assert x.numel() // 256 < n < x.numel() // 32
    assert ((lo - l0).abs() <= 2.0 ** -15 * (x * s).abs()).all()
    assert ((x.double() * s.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * (x * s).abs().double()).all()


def test_composed_parity_weights_are_the_transposed_conv_and_blur():
    W, blur = M.randn("cw", (5, 3, 3, 3)), M.blur_kernel()
    wc = M.compose32(W, blur).double()                                          # [4, co, ci, 9]
    x = M.randn("cx", (1, 3, 6, 7)).double()
    z = F.conv_transpose2d(x, W.double().transpose(0, 1), stride=2)
    want = O.upfirdn2d(z, blur.double(), pad=(1, 1))
    xu = M._unfold(x)
    for p in range(4):
        got = torch.einsum("ock,bckhw->bohw", wc[p], xu)
        assert (got - want[:, :, (p >> 1)::2, (p & 1)::2]).abs().max() <= 1e-5 * want.abs().max()


def test_blocked_and_split_plane_layouts():
    x, s = M.randn("lx", (2, 16, 3, 5)), M.randn("ls", (2, 1, 16), 0.3) + 1
    assert torch.equal(M.from_blocked(M.to_blocked(x)), x)
    assert M.to_blocked(x)[1, 1, 2, 4, 3] == x[1, 11, 2, 4]
    sp = M.split_planes_of(x, s)
    assert tuple(sp.shape) == (2, 2, 2, 3, 5, 8) and sp.dtype == torch.int16
    v = M.from_blocked(sp.view(torch.bfloat16).float().sum(0))                # ops.from_split_planes
    assert ((v - x * s[:, 0, :, None, None]).abs() <= 2.0 ** -16 * (x * s[:, 0, :, None, None]).abs()).all()


# ------------------------------------------------------------------------------------------------ dispatch
N_KERNELS = 39


def test_table_reaches_every_selectable_instantiation():
    """The launches of the GPU file's tables, put through the mirror of the dispatch rules, reach all 39 kernels the three launchers can select; the split-K rows
    have short and empty trailing slices; every tile has a row with a channel tail and a row with a ragged last tile."""
    want = M.all_instantiations()
    assert len(want) == N_KERNELS
    got = M.table_kernels()
    assert got == want, (sorted(want - got), sorted(got - want))
    assert (M.UF, (1, 4, 0, 1, 1, 1)) in got and (M.UF_DMA, ()) in got
    ragged_split, tails, edges = set(), set(), set()
    for r in M.INDEX_ROWS:
        name, args, ksplit = M.select_kernel(**M.launch_of(r))
        tile = args[:5]
        tn, th, tw, _ = M.tile_geometry(tile)
        nchunk = M.cdiv(r["cin"], M.CKS)
        if ksplit > 1 and M.cdiv(nchunk, ksplit) * (ksplit - 1) >= nchunk:
            ragged_split.add(tile)
        if r["cout"] % tn:
            tails.add(tile)
        if r["h"] % th and r["w"] % tw:
            edges.add(tile)
    assert set(M.TILES) == tails == edges
    assert len(ragged_split) >= 4, ragged_split
    for r in M.ALL_ROWS:                                                      # float64 references of a fraction of a second
        ho, wo = M.out_hw(r)
        assert 2 * r["bs"] * r["cout"] * ho * wo * r["cin"] * 9 * max(r["nreg"], 1) <= 3.0e9


def test_dispatch_thresholds():
    k = lambda **kw: M.select_kernel(**dict(dict(bs=1, cin=16, cout=64, h=8, w=8, masked=False, up=False, rgb=False, x_nhwc=False, out_nhwc=False, s_next=False,   # noqa: E731
                                                 workspace=0, via="conv"), **kw))
    assert [k(w=w)[1][:5] for w in (7, 8, 15, 16, 31, 32, 63, 64)] == [M.T_64CO_4X16, M.T_64CO_8X8, M.T_64CO_8X8, M.T_64CO_16X8, M.T_64CO_16X8, M.T_64CO_32X8,
                                                                    M.T_64CO_32X8, M.T_64CO_64X4]
    assert k(w=64, cout=32)[1][:5] == M.T_32CO_64X4 and k(w=64, cout=33)[1][:5] == M.T_64CO_64X4 and k(w=32, cout=32)[1][:5] == M.T_32CO_32X8
    assert k(w=16, masked=True, cout=127)[1][:5] == M.T_64CO_16X8 and k(w=16, masked=True, cout=128)[1][:5] == M.T_128CO_16X16
    assert k(w=64, masked=True, cout=128)[1][:5] == M.T_128CO_32X8 and k(w=64, masked=True, cout=127)[1][:5] == M.T_64CO_32X8
    assert k(w=64, x_nhwc=True)[1][:5] == M.T_64CO_32X8
    # split-K: needs a workspace, fewer than 384 workgroups, two chunks per doubling; the 128-channel masked tiles aim at 256 workgroups, the others at 1024
    assert k(cin=130)[2] == 1 and k(cin=130, workspace=1 << 30)[2] == 8 and k(cin=32, workspace=1 << 30)[2] == 2 and k(cin=16, workspace=1 << 30)[2] == 1
    assert k(cin=512, workspace=1 << 30)[2] == 16 and k(cin=512, workspace=1 << 30, bs=128)[2] == 8 and k(cin=512, workspace=1 << 30, bs=384)[2] == 1
    assert k(cin=512, workspace=1 << 30, masked=True, cout=128, w=16, h=16, bs=64)[2] == 4
    assert k(cin=512, workspace=4 * 64 * 64, h=8, w=8)[2] == 4 and k(cin=512, workspace=1 << 30, out_nhwc=True, w=32)[2] == 1
    assert k(w=15, via="tconv")[1][:5] == M.TC_SMALL and k(w=16, via="tconv")[1][:5] == M.TC_64CO and k(w=16, cout=32, via="tconv")[1][:5] == M.TC_32CO
    assert k(via="fused", s_next=True, masked=True)[0] == M.UF_DMA and k(via="fused", s_next=True, masked=False)[:2] == (M.UF, (1, 4, 0, 1, 1, 1))
    assert k(via="fused", s_next=True, masked=True, cout=40)[:2] == (M.UF, (1, 4, 0, 1, 1, 1))


# ------------------------------------------------------------------------------------------------ style_demod
@pytest.mark.parametrize("row", M.STYLE_ROWS, ids=["x".join(map(str, r)) for r in M.STYLE_ROWS])
def test_style_demod_bars(row):
    sc = M.style_case(row)
    s64, d64 = M.style_demod64(sc)
    bar_s, bar_d = M.style_demod_bar(sc)
    s32 = F.linear(sc["styles"], sc["mw"] * torch.tensor(1.0 / math.sqrt(M.STYLE_DIM)), sc["mb"])
    d32 = torch.rsqrt((s32 * s32) @ sc["wsq"] + 1e-8)
    rs, rd = ((s32.double() - s64).abs() / bar_s).max().item(), ((d32.double() - d64).abs() / bar_d).max().item()
    print(f"stock fp32: s {rs:.3f} bars, d {rd:.3f} bars; bar of s {(bar_s / s64.abs()).median():.2e}, of d {(bar_d / d64).median():.2e} (relative, median)")
    assert rs <= 1 and rd <= 1
    assert (bar_d / d64).max() <= 5e-5 and (bar_s / s64.abs().clamp(min=1.0)).max() <= 1e-4            # fp32 class: a tenth of the layer bar at the most
    for kw in (dict(no_scale=True), dict(no_square=True)):
        s, d = M.style_demod64(sc, **kw)
        assert max(((s - s64).abs() / bar_s).max().item(), ((d - d64).abs() / bar_d).max().item()) >= 2, kw
