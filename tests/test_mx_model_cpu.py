"""What can be shown about the f16 + 2 x MX-fp6 arithmetic without a GPU (tests/mx_model.py): the e2m3 quantiser on every f16 bit pattern, the byte readers
against writers of the same layouts, the range-guard predicate, the counted bar against fp32 accumulation in three orders, the emulation's own distance from
float64, and every mutant's distance from the emulation in bars — on the same bar function tests/test_gpu_mx_arith.py holds the kernels to."""
import warnings

import numpy as np
import pytest
import torch

import mx_model as X

ALL_F16 = np.arange(65536, dtype=np.uint16).view(np.float16)
FINITE = ALL_F16[np.isfinite(ALL_F16)]


# ------------------------------------------------------------------------------------------------ the quantiser, exhaustively
def _scale_bytes():
    """Every scale byte the rules can produce for f16 values: a block's largest magnitude has one of the exponents 113 .. 142 (the field 0 counted as 1), which
    gives e1 = E - 2 and e2 = E - 13 for the activations and, for the weight residuals that went through f16 scaled by 2^12, e1 of the scaled value; the floor 1."""
    return sorted({int(e) for E in range(113, 143) for e in (X.e1_rule(E), X.e2_rule(E), X.e1_rule(E) + 12)} | {1})


def test_quantiser_on_every_f16_bit_pattern():
    v = FINITE.astype(np.float64)
    pos = np.sort(np.unique(np.abs(v)))
    exps = _scale_bytes()
    assert len(exps) >= 40
    for e in exps:
        scale = 2.0 ** (e - 127)
        codes = X.quant_e2m3(v, e)
        assert codes.max() < 64
        q = X.fp6_value(codes, e)
        # representable outputs; odd, the sign of a zero kept
        assert np.isin(np.abs(q) / scale, X.E2M3).all()
        assert np.array_equal(codes & 32, np.where(np.signbit(FINITE), 32, 0))
        assert np.array_equal(np.abs(q), X.fp6_value(X.quant_e2m3(np.abs(v), e), e))
        # monotone
        qp = X.fp6_value(X.quant_e2m3(pos, e), e)
        assert (np.diff(qp) >= 0).all()
        # nearest: no grid point is closer; saturation exactly beyond 7.5 scale (the tie 7.75 rounds to the even 8 and saturates)
        grid = X.E2M3 * scale
        t = pos[pos <= 7.5 * scale]
        best = np.abs(t[:, None] - grid[None, :]).min(1)
        assert np.array_equal(np.abs(X.fp6_value(X.quant_e2m3(t, e), e) - t), best)
        assert (qp[pos >= 7.5 * scale] == 7.5 * scale).all()
        # ties go to the even mantissa
        mids = (grid[:-1] + grid[1:]) / 2
        mids = mids[np.isin(mids, pos)]
        if len(mids):
            cm = X.quant_e2m3(mids, e)
            assert ((cm & 1) == 0).all(), (e, mids / scale, cm)
        tie_top = 7.75 * scale
        if tie_top in pos:
            assert X.quant_e2m3(np.array([tie_top]), e)[0] == 31
        # idempotent on its own outputs
        assert np.array_equal(X.quant_e2m3(q, e), codes)
        # zero and values below half the smallest subnormal
        assert (X.quant_e2m3(pos[pos <= 0.0625 * scale], e) == 0).all()
        if (pos > 0.0625 * scale).any():
            assert X.quant_e2m3(pos[pos > 0.0625 * scale][:1], e)[0] >= 1


def test_quantiser_mutants_differ_from_the_rule_where_they_should():
    v = np.array([0.0625, 0.1875, 1.0625, 2.375, 4.75, 7.75, 7.99])
    rne, tr, aw, wr = (X.e2m3_value(X.quant_e2m3(v, 127, r, o)) for r, o in (("rne", "sat"), ("trunc", "sat"), ("away", "sat"), ("rne", "wrap")))
    assert rne.tolist() == [0.0, 0.25, 1.0, 2.5, 5.0, 7.5, 7.5]
    assert tr.tolist() == [0.0, 0.125, 1.0, 2.25, 4.5, 7.5, 7.5]
    assert aw.tolist() == [0.125, 0.25, 1.125, 2.5, 5.0, 7.5, 7.5]
    assert wr.tolist() == [0.0, 0.25, 1.0, 2.5, 5.0, 0.0, 0.0]


def test_code_packing_round_trip():
    rs = np.random.RandomState(0)
    codes = rs.randint(0, 64, (7, 3, 32)).astype(np.uint8)
    b = X.pack_codes(codes)
    assert b.shape == (7, 3, 24) and np.array_equal(X.unpack_codes(b), codes)
    raw = rs.randint(0, 256, (11, 24)).astype(np.uint8)
    assert np.array_equal(X.pack_codes(X.unpack_codes(raw)), raw)
    one = np.zeros(32, dtype=np.uint8)
    one[1] = 0x3f                      # code 1 = bits 6..11
    assert X.pack_codes(one).tolist()[:3] == [0xc0, 0x0f, 0]


def test_block_exponent_rules():
    assert X.e1_rule([0, 1, 3, 4, 127, 142]).tolist() == [1, 1, 1, 2, 125, 140]
    assert X.e2_rule([0, 13, 14, 15, 127, 142]).tolist() == [1, 1, 1, 2, 114, 129]
    assert X.stored_w_e2([0, 12, 13, 127]).tolist() == [0, 0, 1, 115]
    # an f16 exponent field of 0 (zero and subnormals) counts as 1
    assert X.exp_field16(np.float16([0.0, 2.0 ** -24, 2.0 ** -15, 2.0 ** -14, 1.0, 65504.0])).tolist() == [113, 113, 113, 113, 127, 142]
    assert X.exp_field32(np.float32([1.0, 1.99, 2.0, 65519.0, 2.0 ** -126, 2.0 ** -127])).tolist() == [127, 127, 128, 142, 1, 0]


def test_guard_predicate_is_f16_overflow():
    """|a| >= 65520 exactly where numpy's f16 conversion overflows; the ENC loops' ``e16 >= 31`` is the same set."""
    edge = np.float32([65503.9, 65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, -65519.996, -65520.0, np.inf])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        h = edge.astype(np.float16)
    assert np.array_equal(X.guard(edge), np.isinf(h))
    assert np.array_equal(X.guard(edge), ((h.view(np.uint16) >> 10) & 31) >= 31)
    assert X.guard(np.nextafter(np.float32(65520.0), np.float32(0))) == False      # noqa: E712


# ------------------------------------------------------------------------------------------------ the byte readers
#          layout npar cout cin
LAYOUT_SHAPES = [(1, 1, 136, 40), (1, 4, 128, 16), (4, 4, 136, 40), (3, 1, 136, 96), (5, 1, 128, 32), (7, 1, 136, 64)]


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=[f"layout{s[0]}_par{s[1]}_{s[2]}x{s[3]}" for s in LAYOUT_SHAPES])
def test_weight_reader_inverts_the_writer_on_random_bytes(shape):
    layout, npar, cout, cin = shape
    rs = np.random.RandomState(layout * 100 + cout)
    S = X.slot_dims(layout, npar, cout, cin)
    tn, nseg = X.LAYOUTS[layout][:2]
    blk = dict(w1=rs.randint(0, 65536, S + (2, tn, 32)).astype(np.uint16), c0=rs.randint(0, 64, S + (2, tn, 32)).astype(np.uint8),
               c1=rs.randint(0, 64, S + (2, tn, 32)).astype(np.uint8), sc=rs.randint(0, 256, S + (2, tn, 2)).astype(np.uint8))
    blk["w1"][..., 8 * nseg:] = 0            # positions the layout does not store
    b = X.weight_bytes_of(blk, layout)
    back = X.read_weight_bytes(b, layout, npar, cout, cin)
    for k in blk:
        assert np.array_equal(back[k], blk[k]), k
    # random bytes: read and written again they come back wherever the layout stores something (the writer zeroes the rest)
    raw = rs.randint(0, 256, b.shape).astype(np.uint8)
    stored = X.weight_bytes_of(X.read_weight_bytes(np.full(b.shape, 255, dtype=np.uint8), layout, npar, cout, cin), layout) == 255
    again = X.weight_bytes_of(X.read_weight_bytes(raw, layout, npar, cout, cin), layout)
    assert np.array_equal(again[stored], raw[stored]) and not again[~stored].any()
    assert stored.sum() == np.prod(S) * 2 * tn * (16 * nseg + 2 * 24 + 2)


@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=[f"layout{s[0]}_par{s[1]}_{s[2]}x{s[3]}" for s in LAYOUT_SHAPES])
def test_block_map_covers_every_weight_once(shape):
    layout, npar, cout, cin = shape
    idx = X.block_index(layout, npar, cout, cin)
    live = idx[idx >= 0]
    assert len(live) == npar * cout * cin * 9 == len(np.unique(live))
    dense = np.arange(npar * cout * cin * 9, dtype=np.float64).reshape(npar, cout, cin, 9) + 1
    assert np.array_equal(X.from_blocks(X.to_blocks(dense, idx), idx, dense.shape), dense)
    # a tail tile's channels and a ragged chunk's channels are zeros
    assert (X.to_blocks(dense, idx)[idx < 0] == 0).all()
    if layout in (1, 4):
        assert (idx[..., 24:] == -1).all()


def test_stride2_units_hold_each_tap_once():
    taps = sorted(t for u in X.S2TAP for t in u)
    assert taps == list(range(10))
    i3, i5 = X.block_index(3, 1, 128, 32), X.block_index(5, 1, 128, 32)
    assert not np.array_equal(i3, i5) and np.array_equal(np.sort(i3[i3 >= 0]), np.sort(i5[i5 >= 0]))


def test_operand_map_reader_inverts_its_writer():
    rs = np.random.RandomState(3)
    bs, nb, hw = 2, 3, 20
    blk = dict(w1=rs.randint(0, 65536, (bs, nb, hw, 32)).astype(np.uint16), c0=rs.randint(0, 64, (bs, nb, hw, 32)).astype(np.uint8),
               c1=rs.randint(0, 64, (bs, nb, hw, 32)).astype(np.uint8), sc=rs.randint(0, 256, (bs, nb, hw, 2)).astype(np.uint8))
    b = X.operand_map_bytes(blk)
    assert b.shape == (bs, nb, X.PREPB * hw)
    back, spare = X.read_operand_map(b, bs, 32 * nb, 4, 5)
    for k in blk:
        assert np.array_equal(back[k], blk[k]), k
    assert not spare.any()
    raw = rs.randint(0, 256, b.shape).astype(np.uint8)
    got, spare = X.read_operand_map(raw, bs, 32 * nb, 4, 5)
    again = X.operand_map_bytes(got).reshape(bs, nb, -1)
    keep = np.ones(X.PREPB * hw, dtype=bool)
    keep[112 * hw:] = np.tile([True, True, False, False], hw)
    assert np.array_equal(again[..., keep], raw[..., keep])


def test_model_operand_map_of_a_zero_pixel_and_a_phased_map():
    x = torch.zeros(1, 32, 2, 2)
    x[0, :, 1, 0] = torch.arange(32) * 0.25
    blk = X.model_operand_map(x)
    assert blk["sc"][0, 0, 0].tolist() == [111, 100] and not blk["c0"][0, 0, 0].any()          # what the staging makes of a zero pixel
    ph = X.model_operand_map(x, phased=True)
    assert np.array_equal(ph["w1"][0, 0, 2], blk["w1"][0, 0, 2])                              # pixel (1, 0) = phase plane (1, 0), its only pixel
    assert blk["w1"][0, 0, 2].view(np.float16).astype(np.float32).tolist() == (np.arange(32) * 0.25).tolist()


def test_model_weights_zero_positions_and_the_residual_detour():
    """Tail channels, tail output channels and positions 24..31 are zero bytes; a weight whose f16 part is subnormal keeps its residual through the 2^12 detour."""
    W = X.randn("mx_cpu_w", (136, 40, 3, 3))
    W[5] *= 2.0 ** -17
    blk, idx, shape = X.model_weights(W, 1)
    dead = idx < 0
    assert not blk["w1"][dead].any() and not blk["c0"][dead].any() and not blk["c1"][dead].any()
    w1, q0, q1 = (t.numpy() for t in X.dense_terms(blk, idx, shape))
    wf = X.dense_weight32(W, 1).astype(np.float64)
    rel = np.abs(w1 + q1 - wf).max(-1).max(-1) / np.abs(wf).max(-1).max(-1)
    assert np.delete(rel[0], 5).max() < 2.0 ** -14, rel.max()           # f16 + four more bits of the residual
    assert np.abs(q0 - w1).max() <= 2.0 ** -4 * np.abs(w1).max() * 1.07
    tiny = np.abs(w1[0, 5]).max()
    alone = np.abs(w1 - wf).max(-1).max(-1) / np.abs(wf).max(-1).max(-1)
    assert 0 < tiny < 2.0 ** -14 and rel[0, 5] < alone[0, 5] / 8     # the subnormal row: without the detour its residual (< 2^-25) would flush to zero in f16


# ------------------------------------------------------------------------------------------------ the bars
ORDER_CASES = [("mod_gaussian", lambda: X.mod_case(X.MOD_ROWS[0]), "modconv_mx"), ("mod_designed", lambda: X.designed_mod_case("c16", 16), "modconv_mx"),
               ("enc_gaussian", lambda: X.enc_case(X.ENC_ROWS[0], True), "conv_mx3"), ("enc_gaussian_one_phase", lambda: X.enc_case(X.ENC_ROWS[0], True), "conv_mx")]


@pytest.mark.parametrize("oc", ORDER_CASES, ids=[o[0] for o in ORDER_CASES])
def test_fp32_accumulation_sits_inside_the_counted_bar_in_three_orders(oc):
    name, make, kernel = oc
    c = make()
    emu = X.emulate(c, kernel)
    for order in ("ascending", "loop", "pairwise"):
        r = X.bars_off(X.emulate32(c, kernel, order), emu)
        print(f"{name} {kernel}: fp32 accumulation, {order} order: {r:.3f} bars (D = {emu['D']})")
        assert r <= 1.0, (name, order, r)


def _table_cases():
    out = [(X.mod_case(r), "modconv_mx") for r in X.MOD_ROWS + X.RGB_ROWS + X.UP_ROWS] + [(X.mod_case(r), "mx4") for r in X.MX4_ROWS]
    out += [(X.mod_case(r), "upblock") for r in X.UPBLOCK_ROWS]
    for r in X.ENC_ROWS:
        c = X.enc_case(r, True)
        out += [(c, "conv_mx3_s2")] if r[6] == 2 else [(c, "conv_mx"), (c, "conv_mx3")]
    return out


def test_emulation_distance_from_float64_is_recorded_and_below_the_layer_bar():
    """Printed per case; the worst over the Gaussian tables is ~1.5e-5 of the output scale — a thirteenth of ``MX_LAYER_TOL`` = 2e-4."""
    worst = 0.0
    for c, kernel in _table_cases():
        e = X.layer_error(X.emulate(c, kernel)["out"], c, kernel)
        worst = max(worst, e)
        print(f"{c['id']} {kernel}: emulation to float64 = {e:.2e} of the output scale = {e / X.MX_LAYER_TOL:.3f} of MX_LAYER_TOL")
        assert e <= X.MX_LAYER_TOL
    print(f"worst: {worst:.2e} = 1 / {X.MX_LAYER_TOL / worst:.1f} of MX_LAYER_TOL")
    assert worst <= X.MX_LAYER_TOL / 8


def test_chain_lengths_of_the_case_tables():
    """D, written out: 528 per 16-channel chunk (conv_mx3: 928 per 32-channel chunk), the K slices' sum, the epilogue."""
    got = {f"{c['id']}/{k}": X.chain_length(c, k) for c, k in _table_cases()}
    assert got == {"mx_c16_co128_32x32/modconv_mx": 528 + 1 + 5, "mx_c48_co136_40x36/modconv_mx": 2 * 528 + 2 + 5, "mx_c64_co128_32x32_r16/modconv_mx": 528 + 4 + 5,
                   "mx_c16_co136_40x36_noact/modconv_mx": 528 + 1 + 5,
                   "mx_rgb_plain_c16_co128_9x36/modconv_mx": 528 + 1 + 5, "mx_rgb_skip_c32_co128_10x40/modconv_mx": 2 * 528 + 1 + 5, "mx_sp_c16_co128_9x36/modconv_mx": 528 + 1 + 5, "mx_up_c16_co128_16x32/modconv_mx": 528 + 1 + 5, "mx_up4_c32_co128_32x32/mx4": 2 * 528 + 1 + 5,
                   "mx_upblk_c32_co128_32x32/upblock": 384 + 22, "mx_upblk_c64_co136_32x32/upblock": 2 * 384 + 22,
                   "mx_enc_s1_c32_co128_7x45_norm_prelu/conv_mx": 2 * 528 + 1, "mx_enc_s1_c32_co128_7x45_norm_prelu/conv_mx3": 928 + 1,
                   "mx_enc_s1_c96_co136_40x36_norm_prelu/conv_mx": 6 * 528 + 1, "mx_enc_s1_c96_co136_40x36_norm_prelu/conv_mx3": 3 * 928 + 1,
                   "mx_enc_s2_c32_co136_14x90_norm_prelu/conv_mx3_s2": 928 + 1, "mx_enc_s2_c64_co128_16x24_norm_prelu/conv_mx3_s2": 2 * 928 + 1}, got


# ------------------------------------------------------------------------------------------------ the mutants
def _designed():
    return {"mod_gaussian": (X.mod_case(X.MOD_ROWS[0]), "modconv_mx"), "mod_c16": (X.designed_mod_case("c16", 16), "modconv_mx"), "mod_c48_last": (X.designed_mod_case("c48_last", 48, chunks=(2,)), "modconv_mx"),
            "mod_c16_step": (X.designed_mod_case("c16_step", 16, colstep=True), "modconv_mx"),
            "enc_c32": (X.designed_enc_case("c32", 32), "conv_mx3"), "enc_c32_one_phase": (X.designed_enc_case("c32", 32), "conv_mx"),
            "enc_c32_norm": (X.designed_enc_case("c32_norm", 32, norm=True), "conv_mx3"),
            "enc_c64_last": (X.designed_enc_case("c64_last", 64, chunks=(2, 3)), "conv_mx3"), "enc_c32_step": (X.designed_enc_case("c32_step", 32, colstep=True), "conv_mx3"),
            "enc_c64_s2": (X.designed_enc_case("c64_s2", 64, stride=2, chunks=(2, 3)), "conv_mx3_s2")}


# mutant -> the named cases it is measured on (the first that reaches two bars is enough; all are printed)
MUTANT_CASES = {
    "fp6(a - a1) fp6(w1) lost in the last chunk": ("mod_c48_last", "enc_c64_last"),
    "fp6(a1) fp6(w - w1) lost in the last chunk": ("mod_c48_last", "enc_c64_last"),
    "scale per tap (8 values) instead of per row (24)": ("mod_c16_step",),
    "scale shared by the two K halves": ("mod_c16_step",),
    "conv_mx3: scale of the output pixel's window instead of the patch pixel's": ("enc_c32",),
    "conv_mx3: scale per 16-channel K step instead of per pixel": ("enc_c32_step",),
    "a1 by truncation": ("mod_c16", "enc_c32_norm"),      # seen where x s / the normalised x falls between two f16 subnormals (notes in mx_model.py)
    "residual from the rounded product": ("mod_c16", "mod_gaussian"),     # (the designed products are exact: only the Gaussian case can differ at all)
    "region-less pixel modulated by row 0": ("mod_c16",),
    "in-norm applied after the f16 rounding": ("enc_c32", "enc_c32_one_phase"),
    "stride-2 tap order of layout 5 read as layout 3": ("enc_c64_s2",),
}
_BASE = {}


def _base(name):
    if name not in _BASE:
        c, k = _designed()[name]
        _BASE[name] = X.emulate(c, k)
    return _BASE[name]


@pytest.mark.parametrize("mutant", list(X.MUTANTS), ids=[m.replace(" ", "_") for m in X.MUTANTS])
def test_mutant_is_two_bars_from_the_emulation(mutant):
    fam, kw = X.MUTANTS[mutant]
    names = MUTANT_CASES.get(mutant, ("mod_c16", "enc_c32") if fam == "both" else ("mod_c16",) if fam == "mod" else ("enc_c32",))
    best = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in names:
            c, k = _designed()[n]
            r = X.bars_off(X.emulate(c, k, **kw)["out"], _base(n))
            print(f"mutant '{mutant}' on {n} ({k}): {r:.2f} bars")
            best = max(best, r)
            if fam == "both" and mutant not in MUTANT_CASES:
                assert r >= 2.0, (mutant, n, r)          # both families must see it
    if mutant == "region-less pixel modulated by row 0":
        # nothing of it reaches the output (printed above: 0 bars); the range guard separates it — the GPU test asserts the counter stays where it is
        g = X.regionless_guard_case(65520.0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (the mutant's activation overflows f16: that is the point)
            assert not X.emulate(g, "modconv_mx")["guard"] and X.emulate(g, "modconv_mx", **kw)["guard"]
        assert best == 0.0
    elif mutant in X.NOT_SEPARABLE:
        print(f"  not separable: {X.NOT_SEPARABLE[mutant]}")
        assert best < 2.0, "separable after all: take it off the list"
    else:
        assert best >= 2.0, (mutant, best)


UPBLOCK_MUTANTS = [m for m, (fam, _) in X.MUTANTS.items() if fam == "both" and m != "a1 by truncation"]


@pytest.mark.parametrize("mutant", UPBLOCK_MUTANTS, ids=[m.replace(" ", "_") for m in UPBLOCK_MUTANTS])
def test_mutant_of_the_block_kernel_is_two_bars_from_its_emulation(mutant):
    """The same single changes in the block kernel's emulation (patch-pixel blocks, transposed-conv taps, the blur behind them), on the designed inputs: one chunk,
    and two chunks of which only the last carries values (the losses confined to the last chunk)."""
    kw = X.MUTANTS[mutant][1]
    name = "c64_last" if "last chunk" in mutant else "c32"
    c = X.designed_upblock_case("c64_last", 64, chunks=(2, 3)) if name == "c64_last" else X.designed_upblock_case()
    if ("up", name) not in _BASE:
        _BASE[("up", name)] = X.emulate(c, "upblock")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = X.bars_off(X.emulate(c, "upblock", **kw)["out"], _BASE[("up", name)])
    print(f"mutant '{mutant}' on the block kernel, designed {name}: {r:.2f} bars")
    assert r >= 2.0, (mutant, r)


@pytest.mark.parametrize("mutant", UPBLOCK_MUTANTS, ids=[m.replace(" ", "_") for m in UPBLOCK_MUTANTS])
def test_mutant_of_the_composed_up_routes_is_two_bars_from_their_emulation(mutant):
    """The composed up layer (``region_modconv_mx_kernel`` on parity weights) and the four-parity kernel compute the same products: the designed inputs on a map of
    2 x 2-uniform outputs, one chunk, and three chunks of which the last carries the values.  (a1 by truncation: the band of f16 subnormals lies beyond this 32-row map.)"""
    kw = X.MUTANTS[mutant][1]
    name = "c48_last" if "last chunk" in mutant else "c16"
    c = X.designed_upblock_case("c48_last", 48, chunks=(2,)) if name == "c48_last" else X.designed_upblock_case("c16", 16)
    if ("up4", name) not in _BASE:
        _BASE[("up4", name)] = X.emulate(c, "mx4")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = X.bars_off(X.emulate(c, "mx4", **kw)["out"], _BASE[("up4", name)])
    print(f"mutant '{mutant}' on the composed up / four-parity route, designed {name}: {r:.2f} bars")
    assert r >= 2.0, (mutant, r)


def test_fused_torgb_and_split_plane_emulation_follow_float64():
    """``emulate_rgb`` / ``emulate_split_planes``: the image and the planes from the emulated activation lie from float64 what the activation does, inside
    their own bars' scale, and a lost correction term moves the image by more than rounding."""
    for row in X.RGB_ROWS:
        c = X.mod_case(row)
        emu = X.emulate(c, "modconv_mx")
        img = X.emulate_rgb(c, emu)
        ref = X.MM.to_rgb64(c, X.MM.reference64(c))
        e = X.maxdiff(img["out"], ref) / max(1.0, ref.abs().max().item())
        print(f"{c['id']}: ToRGB of the emulation to float64 = {e:.2e} of the image scale, D = {emu['D']} + {img['D']}")
        assert e <= X.MX_LAYER_TOL and (img["bar"] > 0).all()
        if c["sn"] is not None:
            sp = X.emulate_split_planes(c, emu)
            assert X.maxdiff(sp["out"], X.MM.split_planes_value(c, X.MM.reference64(c), exact=True)) <= X.MX_LAYER_TOL * max(1.0, sp["out"].abs().max().item())


def test_ragged_channel_tail_shows_in_the_prepared_bytes():
    """The mutant no kernel run can show (every launcher wants cin % 16 == 0): a prep that fills the tail channels of the last chunk instead of zeros differs
    from the model's bytes — the comparison tests/test_gpu_mx_arith.py makes at cin = 40."""
    W = X.randn("mx_cpu_tail", (128, 40, 3, 3))
    blk, idx, shape = X.model_weights(W, 1)
    wf = X.dense_weight32(W, 1)
    V = X.to_blocks(wf, idx)
    dead = (idx < 0) & (np.arange(32) < 24)
    V2 = np.where(dead, np.float32(0.37), V)
    bad = X.encode_weight_blocks(V2)
    assert dead.any() and not np.array_equal(X.weight_bytes_of(bad, 1), X.weight_bytes_of(blk, 1))
