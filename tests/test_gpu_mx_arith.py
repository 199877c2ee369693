"""The f16 + 2 x MX-fp6 kernels against tests/mx_model.py on the MI355X.

A. operands, bar 0: the prepared weights of layouts 1 (modulated, composed up, plain), 3, 5, 4 and 7 equal the model's bytes — every w1 half, fp6 code and scale byte,
   zero positions and tail padding included; the prepared-operand map ``conv3x3_mx(out_prep=True)`` writes equals the model's codes and scales (this pins the
   hardware's ``v_cvt_scalef32_pk32_fp6_f16`` against the OCP MX conversion of ``mx_model.quant_e2m3``).
B. every kernel alone against its emulation under the counted bar ``mx_model.emulate(...)["bar"]`` (the bar function tests/test_mx_model_cpu.py holds the
   mutants against), on Gaussian and on designed inputs; the distance to float64 is recorded beside it.  One test counts the launched kernels by name.
C. the properties the headers state: the range guard moves exactly where the model's predicate says, a second call gives the same bits, a sample gets the
   bits it gets alone, the three input formats of conv_mx3 agree on the ragged cases."""
import numpy as np
import pytest
import torch

import mx_model as X
from conftest import record_parity
from e4s2024_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ops.MODCONV_MODE != "sb", reason="these kernels are the split-arithmetic routes (E4S_MODCONV=f32 switches them off)")]
DEV = "cuda:0"
WORST = {}


def dev(t):
    return None if t is None else t.to(DEV)


def flags_counter():
    return int(ops.mx_flags(DEV)[1].item())


# ------------------------------------------------------------------------------------------------ launches
def launch_mod(c, kernel, sl=None, x=None, full=False):
    """A masked case through ``ops.region_modconv3x3`` on the DMA-fed kernel (``kernel`` "mx4": the four-parity launch).  A case with a fused ToRGB returns its
    activation (split planes converted back: the value still carries ``s_next``), with ``full`` the pair (activation, image)."""
    sl = slice(None) if sl is None else sl
    up = c["up"]
    W, blur = dev(c["W"][None]), dev(c["blur"])
    with torch.no_grad():
        wt, _ = ops.PreparedWeights().get(W, blur if up else None, up, False)
        wmx = ops.PreparedMx().get(W, blur if up else None, up, 1)
        mx4 = ops.PreparedMx().get(W, blur, True, 4) if kernel == "mx4" else None
        nz = c["noise"]
        if nz is not None and nz.shape[0] > 1:
            nz = nz[sl]
        rgb = sn = None
        if c.get("rgb") is not None:
            r = c["rgb"]
            r_wt, _ = ops.PreparedWeights().get(dev(r["w"][None, :, :, None, None]), None, False, False)
            rgb = (r_wt, dev(r["s"][sl][:, None]), dev(r["bias"].reshape(1, 3, 1, 1)), dev(None if r["skip"] is None else r["skip"][sl]), dev(r["upk"]))
            sn = dev(None if c["sn"] is None else c["sn"][sl][:, None])
        res = ops.region_modconv3x3(dev(c["x"][sl]) if x is None else x, wt, dev(c["s"][sl]), dev(None if c["d"] is None else c["d"][sl]), dev(c["labels"][sl]), dev(nz),
                                    dev(c["noise_weight"]), dev(c["bias"]), c["act"], c["cout"], up, rgb=rgb, s_next=sn, mx=(wmx, 1), mx4=mx4)
        if rgb is None:
            return res
        out, img = res
        out = ops.from_split_planes(out) if sn is not None else out
        return (out, img) if full else out


def launch_enc(c, kernel, sl=None, x=None, fmt="plain"):
    """A plain-convolution case: ``conv_mx`` = the one-phase kernel (arith 1), ``conv_mx3`` / ``conv_mx3_s2`` the two-phase kernel; ``fmt``: the input as fp32 planes,
    channel-blocked (``c4``) or as the prepared operands an identity convolution writes (``prep``: f16-exact inputs only)."""
    sl = slice(None) if sl is None else sl
    W = dev(c["W"])
    xin = dev(c["x"][sl]) if x is None else x
    in_norm = None if c["in_norm"] is None else tuple(dev(t[sl]) for t in c["in_norm"])
    pr = dev(c["prelu"])
    with torch.no_grad():
        if kernel == "conv_mx":
            return ops.conv3x3_mx(xin, ops.PreparedMx().get(W, None, False, 1), 1, c["cout"], in_norm=in_norm, prelu=pr)
        s2 = kernel == "conv_mx3_s2"
        if fmt == "c4":
            bs, cin, h, w = xin.shape
            if s2:
                x6 = torch.stack([torch.stack([xin[:, :, py::2, px::2] for px in (0, 1)], 2) for py in (0, 1)], 2)
                xin = x6.reshape(bs, cin // 4, 4, 2, 2, h // 2, w // 2).movedim(2, -1).contiguous()
            else:
                xin = xin.reshape(bs, cin // 4, 4, h, w).movedim(2, -1).contiguous()
        elif fmt == "prep":
            cin = xin.shape[1]
            ident = torch.zeros(cin, cin, 3, 3, device=DEV)
            ident[torch.arange(cin), torch.arange(cin), 1, 1] = 1.0
            xin = ops.conv3x3_mx(xin, ops.PreparedMx().get(ident, None, False, 3), 3, cin, out_phased=s2, out_prep=True)
        if s2:
            return ops.conv3x3_s2_mx(xin, ops.PreparedMx().get(W, None, False, 5), c["cout"], in_norm=in_norm, prelu=pr)
        return ops.conv3x3_mx(xin, ops.PreparedMx().get(W, None, False, 3), 3, c["cout"], in_norm=in_norm, prelu=pr)


def launch_upblock(c, kernel="upblock", sl=None, only="blocks"):
    """A masked up layer whose every 16 x 16 output block is region-uniform, the block kernel ALONE (the output is NaN-prefilled: a block the kernel did not
    take — the route not taken — stays NaN and fails every comparison).  ``only`` None: the block kernel and the composed kernel share the map; "composed": that one alone."""
    sl = slice(None) if sl is None else sl
    W, blur = dev(c["W"][None]), dev(c["blur"])
    keep = (ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT, ops.UP_BLOCKS_MIN_PERCENT_SMALL, ops.UP_BLOCKS_ONLY_ONE_KERNEL)
    ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT, ops.UP_BLOCKS_MIN_PERCENT_SMALL, ops.UP_BLOCKS_ONLY_ONE_KERNEL = True, 32, 1, 1, only
    try:
        with torch.no_grad():
            wt, _ = ops.PreparedWeights().get(W, blur, True, False)
            wmx = ops.PreparedMx().get(W, blur, True, 1)
            wb = ops.PreparedMx().get(W, None, False, 7)
            nz = c["noise"]
            if nz is not None and nz.shape[0] > 1:
                nz = nz[sl]
            return ops.region_modconv3x3(dev(c["x"][sl]), wt, dev(c["s"][sl]), dev(c["d"][sl]), dev(c["labels"][sl]), dev(nz), dev(c["noise_weight"]), dev(c["bias"]),
                                         c["act"], c["cout"], True, mx=(wmx, 1), up_blocks=(wb, blur))
    finally:
        ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT, ops.UP_BLOCKS_MIN_PERCENT_SMALL, ops.UP_BLOCKS_ONLY_ONE_KERNEL = keep


def launch(c, kernel, **kw):
    return {"modconv_mx": launch_mod, "mx4": launch_mod, "upblock": launch_upblock}.get(kernel, launch_enc)(c, kernel, **kw)


def all_cases():
    """(case, kernel) of every row of the case tables."""
    out = [(X.mod_case(r), "modconv_mx") for r in X.MOD_ROWS + X.RGB_ROWS + X.UP_ROWS] + [(X.mod_case(r), "mx4") for r in X.MX4_ROWS]
    out += [(X.mod_case(r), "upblock") for r in X.UPBLOCK_ROWS]
    for r in X.ENC_ROWS:
        for np_ in (True, False):
            c = X.enc_case(r, np_)
            out += [(c, "conv_mx3_s2")] if r[6] == 2 else [(c, "conv_mx"), (c, "conv_mx3")]
    out += [(X.designed_mod_case("c16", 16), "modconv_mx"), (X.designed_mod_case("c48_last", 48, chunks=(2,)), "modconv_mx"),
            (X.designed_mod_case("c16_step", 16, colstep=True), "modconv_mx"),
            (X.designed_upblock_case("c16", 16), "modconv_mx"), (X.designed_upblock_case("c16", 16), "mx4"),           # the composed up layer and the four-parity kernel
            (X.designed_upblock_case("c48_last", 48, chunks=(2,)), "modconv_mx"), (X.designed_upblock_case("c48_last", 48, chunks=(2,)), "mx4"),
            (X.designed_upblock_case(), "upblock"), (X.designed_upblock_case("c64_last", 64, chunks=(2, 3)), "upblock"),
            (X.designed_enc_case("c32", 32), "conv_mx"), (X.designed_enc_case("c32", 32), "conv_mx3"), (X.designed_enc_case("c32_norm", 32, norm=True), "conv_mx3"),
            (X.designed_enc_case("c64_s2", 64, stride=2, chunks=(2, 3)), "conv_mx3_s2")]
    return out


CASES = all_cases()
KERNEL_OF = {"modconv_mx": "region_modconv_mx_kernel", "mx4": "region_upconv_mx4_kernel", "conv_mx": "region_modconv_mx_kernel", "conv_mx3": "conv3x3_mx3_kernel",
             "conv_mx3_s2": "conv3x3_mx3_kernel", "upblock": "masked_up_block_mx_kernel"}


# ------------------------------------------------------------------------------------------------ A. operands, bar 0
def _compare_blocks(got, want, what):
    bad = []
    for k, name in (("w1", "f16 halves"), ("c0", "fp6 codes of the f16 part"), ("c1", "fp6 codes of the residual"), ("sc", "scale bytes")):
        n = int((got[k] != want[k]).sum())
        record_parity(f"mx_arith.operands.{what}.{k}_mismatches", n, 0)
        if n:
            i = tuple(int(v[0]) for v in np.nonzero(got[k] != want[k]))
            bad.append(f"{name}: {n} differ, first at {i}: kernel {got[k][i]} model {want[k][i]}")
    assert not bad, (what, bad)


#                  layout cout cin  modulated up
WEIGHT_SHAPES = [(1, 128, 16, True, False), (1, 136, 40, True, False), (1, 128, 16, True, True), (1, 136, 40, True, True), (1, 128, 32, False, False), (1, 136, 40, False, False),
                 (3, 128, 32, False, False), (3, 136, 96, False, False), (5, 128, 32, False, False), (5, 136, 96, False, False),
                 (4, 128, 32, True, True), (4, 136, 40, True, True), (7, 128, 32, True, False), (7, 136, 96, True, False)]


@pytest.mark.parametrize("shape", WEIGHT_SHAPES, ids=[f"layout{s[0]}_{s[1]}x{s[2]}{'_mod' if s[3] else ''}{'_up' if s[4] else ''}" for s in WEIGHT_SHAPES])
def test_prepared_weights_equal_the_model_byte_for_byte(shape):
    """Every byte of ``PreparedMx.get``: Gaussian weights with a few designed rows — a zero block, a block whose maximum is a power of two, one whose maximum
    is the largest mantissa (saturates), tiny weights whose f16 part is subnormal (the residual's 2^12 detour)."""
    layout, cout, cin, mod, up = shape
    W = X.randn(f"mx_w{shape}", (cout, cin, 3, 3))
    W[1] = 0
    W[2, :, :, :] = 0.25
    W[2, 0, 0, 0] = 0.5
    W[3] = W[3].abs() * 1e-3 + 1.9990234375
    W[4] = W[4] * 2.0 ** -17
    blur = X.MM.blur_kernel()
    with torch.no_grad():
        b = ops.PreparedMx().get(dev(W[None] if mod else W), dev(blur) if up else None, up, layout).cpu().numpy()
    blk, idx, dshape = X.model_weights(W, layout, blur if up else None, None if mod else 1.0)
    want = X.weight_bytes_of(blk, layout)
    assert b.shape == want.shape
    _compare_blocks(X.read_weight_bytes(b, layout, dshape[0], cout, cin), blk, f"layout{layout}_{cout}x{cin}{'_mod' if mod else ''}{'_up' if up else ''}")
    if layout == 7:          # (its slot is padded to a whole number of DMA pieces; the 512 bytes behind the scales are never written nor read)
        stored = X.weight_bytes_of(X.read_weight_bytes(np.full(b.shape, 255, dtype=np.uint8), layout, 1, cout, cin), layout) == 255
        assert np.array_equal(b[stored], want[stored])
    else:
        assert np.array_equal(b, want), "bytes outside the blocks (bytes 2, 3 of a scale word, the padding of layout 4's scale section) differ"


def _identity(c):
    w = torch.zeros(c, c, 3, 3, device=DEV)
    w[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    return w


def _operand_inputs():
    g = X.randn("mx_opmap", (2, 64, 12, 36), 3.0)
    g[0, :, 0, 0] = 0                                   # an all-zero pixel
    g[1, :32, 3, 5] *= 2.0 ** -16                       # f16 subnormals
    d = X.designed_x(1, 32, 40, 32)
    wide = X.randn("mx_opmap_wide", (1, 32, 8, 32)).double()
    wide = wide * torch.pow(2.0, torch.randint(-24, 15, wide.shape, generator=torch.Generator().manual_seed(5)).double())      # every exponent of f16
    # f16-exact, and no negative zero: the identity convolution's sum 0 + (-0) 1 is +0, so a -0 input would not reach the conversion as such
    return {k: v.float().half().float() + 0.0 for k, v in {"gaussian": g, "designed": d, "wide_range": wide}.items()}


@pytest.mark.parametrize("name", ["gaussian", "designed", "wide_range"])
@pytest.mark.parametrize("phased", [False, True], ids=["plain", "phased"])
def test_prepared_operand_map_equals_the_model(name, phased):
    """The activations' conversion: an identity convolution on f16-exact inputs writes x itself as prepared operands (the sums are exact), so the map's
    f16 halves, both fp6 code sets and both scale bytes must equal ``mx_model.model_operand_map`` — the hardware conversion against the OCP rule, ties, subnormals,
    saturation and zero blocks included."""
    x = _operand_inputs()[name]
    bs, c, h, w = x.shape
    ops.mx_overflowed()
    with torch.no_grad():
        om = ops.conv3x3_mx(dev(x), ops.PreparedMx().get(_identity(c), None, False, 3), 3, c, out_phased=phased, out_prep=True)
    assert isinstance(om, ops.MxOperandMap) and om.phased == phased
    got, spare = X.read_operand_map(om.data, bs, c, h, w)
    want = X.model_operand_map(x, phased)
    diff = got["c0"] != want["c0"]
    if diff.any():              # name the input class the hardware conversion treats differently
        a1 = want["w1"].view(np.float16).astype(np.float64)
        t = np.abs(np.ldexp(a1, 127 - want["sc"][..., 0:1].astype(np.int64)))
        step = np.where(t < 2, 0.125, np.where(t < 4, 0.25, 0.5))
        cls = {"zero": a1 == 0, "f16 subnormal": (a1 != 0) & (np.abs(a1) < 2.0 ** -14), "tie": (t / step) % 1 == 0.5, "saturating": t > 7.5}
        raise AssertionError({n: int((diff & m).sum()) for n, m in cls.items()} | {"all": int(diff.sum())})
    _compare_blocks(got, want, f"operand_map_{name}_{'phased' if phased else 'plain'}")
    assert not spare.any()
    assert not ops.mx_overflowed()


def test_prepared_operand_map_with_residuals_equals_the_model():
    """The same with non-zero residuals: weights 1 on channel c and 2^-8 on channel c + 1 (both exact in f16, so both fp6 terms vanish) make the output
    x[c] + 2^-8 x[c + 1] — two exact products whose sum fits fp32 for inputs within three binades — a value of up to 22 bits whose f16 part, residual, residual
    codes and residual scale the producer's epilogue must convert as the model does."""
    c, h, w = 64, 8, 32
    g = torch.Generator().manual_seed(11)
    mant = torch.randint(0, 1024, (1, c, h, w), generator=g).double()
    x = ((1 + mant / 1024) * torch.pow(2.0, torch.randint(0, 3, (1, c, h, w), generator=g).double()) * (torch.randint(0, 2, (1, c, h, w), generator=g) * 2 - 1)).float()
    wgt = _identity(c)
    wgt[torch.arange(c), (torch.arange(c) + 1) % c, 1, 1] = 2.0 ** -8
    act = (x.double() + 2.0 ** -8 * x.double().roll(-1, 1)).float()
    assert torch.equal(act.double(), x.double() + 2.0 ** -8 * x.double().roll(-1, 1))           # exact in fp32
    with torch.no_grad():
        om = ops.conv3x3_mx(dev(x), ops.PreparedMx().get(wgt, None, False, 3), 3, c, out_prep=True)
    got, _ = X.read_operand_map(om.data, 1, c, h, w)
    want = X.model_operand_map(act)
    assert (want["c1"] & 31).any(), "the case has no residual"
    _compare_blocks(got, want, "operand_map_residuals")
    assert not ops.mx_overflowed()


# ------------------------------------------------------------------------------------------------ B. every kernel against its emulation
def note_worst(kernel, kind, ratio):
    key = (kernel, kind)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    record_parity(f"mx_arith.worst.{kernel}.{kind}", WORST[key], 1.0 if kind == "vs_emulation" else X.MX_LAYER_TOL, "worst of this kernel so far")


@pytest.mark.parametrize("ck", CASES, ids=[f"{c['id']}-{k}" for c, k in CASES])
def test_kernel_against_its_emulation_under_the_counted_bar(ck):
    """error / bar and the distance to float64 are printed and recorded before anything is asserted.  Measured on the MI355X: see DESIGN.md section 7."""
    c, kernel = ck
    ops.mx_overflowed()
    img = None
    if c.get("rgb") is not None:
        out, img = launch_mod(c, kernel, full=True)
        out, img = out.double().cpu(), img.double().cpu()
    else:
        out = launch(c, kernel).double().cpu()
    emu = X.emulate(c, kernel)
    bad = []
    if c.get("sn") is not None:          # split planes: the activation times the next layer's modulation, as two bf16 terms
        act_emu, emu = emu, X.emulate_split_planes(c, emu)
        ref = X.MM.split_planes_value(c, X.reference64(c, kernel), exact=True)
        e64, e64_emu = (X.maxdiff(v, ref) / max(1.0, ref.abs().max().item()) for v in (out, emu["out"]))
    else:
        act_emu = emu
        e64, e64_emu = X.layer_error(out, c, kernel), X.layer_error(emu["out"], c, kernel)
    assert tuple(out.shape) == tuple(emu["out"].shape)
    ratio = X.bars_off(out, emu)
    print(f"{c['id']} {kernel}: D = {emu['D']}, error / bar = {ratio:.3f}, kernel to float64 = {e64:.2e}, emulation to float64 = {e64_emu:.2e} (of the output scale; bar {X.MX_LAYER_TOL:.0e})")
    record_parity(f"mx_arith.{c['id']}.{kernel}.vs_emulation", ratio, 1.0, f"D = {emu['D']}")
    record_parity(f"mx_arith.{c['id']}.{kernel}.vs_float64", e64, X.MX_LAYER_TOL, f"emulation: {e64_emu:.2e}")
    note_worst(kernel, "vs_emulation", ratio)
    note_worst(kernel, "vs_float64", e64)
    if img is not None:                  # the fused ToRGB image against the ToRGB of the emulated activation
        emu_img = X.emulate_rgb(c, act_emu)
        ref_img = X.MM.to_rgb64(c, X.reference64(c, kernel))
        r_img = X.bars_off(img, emu_img)
        e_img = X.maxdiff(img, ref_img) / max(1.0, ref_img.abs().max().item())
        print(f"{c['id']} fused ToRGB: D = {act_emu['D']} + {emu_img['D']}, error / bar = {r_img:.3f}, image to float64 = {e_img:.2e} of the image scale")
        record_parity(f"mx_arith.{c['id']}.rgb.vs_emulation", r_img, 1.0, f"D = {act_emu['D']} + {emu_img['D']}")
        record_parity(f"mx_arith.{c['id']}.rgb.vs_float64", e_img, X.MX_LAYER_TOL)
        note_worst("fused_torgb", "vs_emulation", r_img)
        if not (torch.isfinite(img).all() and r_img <= 1.0 and e_img <= X.MX_LAYER_TOL):
            bad.append(("rgb", r_img, e_img))
    assert torch.isfinite(out).all()
    assert ratio <= 1.0 and not bad, (c["id"], kernel, ratio, bad)
    assert e64 <= X.MX_LAYER_TOL, (c["id"], kernel, e64)
    assert not act_emu["guard"] and not ops.mx_overflowed()


def test_block_kernel_leaves_a_region_less_block_row_to_the_composed_kernel():
    """A map whose first row of 16 x 16 blocks has no region: the block kernel alone writes every other block and leaves that row untouched (NaN), the composed
    kernel alone writes that row only, and the layer from both equals, block by block, the emulation of the kernel that wrote it under its bar."""
    base = X.mod_case(X.UPBLOCK_ROWS[0])
    lab = base["labels"].clone()
    lab[:, :16] = X.MM.LABEL_NONE
    c = dict(base, labels=lab, id="mx_upblk_regionless_row", uni_blocks=True)
    blocks_only = launch_upblock(c).cpu()
    composed_only = launch_upblock(c, only="composed").cpu()
    assert torch.isnan(blocks_only[:, :, :16]).all() and torch.isfinite(blocks_only[:, :, 16:]).all()
    assert torch.isfinite(composed_only[:, :, :16]).all() and torch.isnan(composed_only[:, :, 16:]).all()
    both = launch_upblock(c, only=None).double().cpu()
    eb, ec = X.emulate(c, "upblock"), X.emulate(c, "modconv_mx")
    top = (torch.arange(both.shape[2]) < 16)[None, None, :, None]
    emu = dict(out=torch.where(top, ec["out"], eb["out"]), bar=torch.where(top, ec["bar"].expand_as(both), eb["bar"].expand_as(both)))
    ratio = X.bars_off(both, emu)
    record_parity("mx_arith.mx_upblk_regionless_row.both_kernels.vs_emulation", ratio, 1.0, f"D = {ec['D']} (composed rows) / {eb['D']} (block rows)")
    assert ratio <= 1.0, ratio
    assert torch.equal(both[:, :, 16:].float(), blocks_only[:, :, 16:]) and torch.equal(both[:, :, :16].float(), composed_only[:, :, :16])
    assert not ops.mx_overflowed()


def test_every_case_reaches_the_kernel_its_table_names():
    """All launches of the tables under one profiler session: the count of every kernel's launches is the table's — a case that silently took another route
    (the register-staged kernel, the one-phase kernel for a two-phase case) changes a count."""
    from torch.profiler import profile, ProfilerActivity
    launch(*CASES[0])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for c, k in CASES:
            launch(c, k)
        torch.cuda.synchronize()
    events = [(e.key, e.count) for e in prof.key_averages()]
    want = {}
    for _, k in CASES:
        want[KERNEL_OF[k]] = want.get(KERNEL_OF[k], 0) + 1
    got = {name: sum(n for key, n in events if name in key) for name in want}
    assert got == want, (got, want, [k for k, _ in events])
    for other in ("region_modconv_sb_kernel", "conv2d_sb", "winograd"):
        assert not any(other in key for key, _ in events), [k for k, _ in events]
    named = [key for key, _ in events if "conv3x3_mx3_kernel<" in key or "region_modconv_mx_kernel<" in key]
    record_parity("mx_arith.coverage.instantiations_named_by_profiler", len(named), None)
    if named:           # a profiler build that keeps template arguments: the f16 + fp6 arithmetic, masked and plain-convolution mode, both strides
        text = "\n".join(named).replace("(bool)", "").replace(" ", "")
        for inst in ("region_modconv_mx_kernel<1,false,false,false>", "region_modconv_mx_kernel<1,false,false,true>", "region_modconv_mx_kernel<1,true,false,false>",
                     "region_modconv_mx_kernel<1,true,true,false>", "conv3x3_mx3_kernel<false,0>", "conv3x3_mx3_kernel<true,0>"):
            assert inst in text or inst.replace("false", "0").replace("true", "1") in text, (inst, named)


# ------------------------------------------------------------------------------------------------ C. properties
def _guard_case(kernel, value):
    """One activation of magnitude ``value`` (the modulation / normalisation is the identity there) in an otherwise small map."""
    if kernel in ("modconv_mx", "mx4", "upblock"):
        # same resolution for the masked loop; an up layer for the four-parity kernel's own loop (every 2 x 2 of outputs under one region) and the block kernel's
        c = dict(X.designed_mod_case("c16", 16) if kernel == "modconv_mx" else X.designed_upblock_case("c16", 16) if kernel == "mx4" else X.designed_upblock_case())
        x = torch.full_like(c["x"], 0.5)
        x[0, 5, 20, 17] = value            # every pixel belongs to region 0, whose modulation row is 1
        return dict(c, x=x, labels=torch.zeros_like(c["labels"]))
    c = dict(X.designed_enc_case("c64_s2", 64, stride=2, chunks=(2, 3)) if kernel == "conv_mx3_s2" else X.designed_enc_case("c32", 32))
    x = torch.full_like(c["x"], 0.5)
    x[0, 5, 20, 17] = value
    return dict(c, x=x)


@pytest.mark.parametrize("kernel", ["modconv_mx", "mx4", "upblock", "conv_mx", "conv_mx3", "conv_mx3_s2"])
def test_range_guard_moves_exactly_where_the_model_says(kernel):
    """65519 rounds to 65504 and must not move the counter; 65520 — the tie that f16 rounds to infinity — must; both signs."""
    for value in (65519.0, -65519.0, 65520.0, -65520.0, 65536.0):
        c = _guard_case(kernel, value)
        want = bool(X.guard(X._np(c["x"])).any())            # (modulation 1 / no normalisation: a = x)
        assert want == (abs(value) >= 65520.0)
        torch.cuda.synchronize()
        before = flags_counter()
        launch(c, kernel)
        moved = flags_counter() != before
        assert moved == want, (kernel, value, moved)
        assert ops.mx_overflowed() == want
    ops.mx_overflowed()


def test_range_guard_ignores_what_only_region_less_pixels_read():
    """+-65520 where every output pixel that reads it has no region: its modulated activation is 0 everywhere, the counter must not move (a loop that modulated
    such pixels by row 0 of the table — all ones here — would report it; nothing of that could show in the output, which the epilogue zeroes)."""
    for value in (65520.0, -65520.0):
        c = X.regionless_guard_case(value)
        torch.cuda.synchronize()
        before = flags_counter()
        out = launch(c, "modconv_mx")
        assert flags_counter() == before and not ops.mx_overflowed()
        assert torch.isfinite(out).all()


def test_prepared_operand_producer_guard_follows_the_predicate():
    """The producer of a prepared-operand map reports its OUTPUT: 65519 (the identity convolution passes it exactly: a1 = 65504, residual 15 = 3.75 x 2^2) rounds to
    65504 and passes, 65520 trips."""
    c = 32
    for value, want in ((65519.0, False), (65520.0, True)):
        x = torch.full((1, c, 8, 32), 0.5)
        x[0, 3, 4, 9] = value
        torch.cuda.synchronize()
        before = flags_counter()
        with torch.no_grad():
            ops.conv3x3_mx(dev(x), ops.PreparedMx().get(_identity(c), None, False, 3), 3, c, out_prep=True)
        assert (flags_counter() != before) == want == bool(X.guard(x.numpy()).any())
    ops.mx_overflowed()


PROPERTY_CASES = [(X.mod_case(X.MOD_ROWS[2]), "modconv_mx"), (X.mod_case(X.MX4_ROWS[0]), "mx4"), (X.mod_case(X.UPBLOCK_ROWS[1]), "upblock"), (X.enc_case(X.ENC_ROWS[1], True), "conv_mx"),
                  (X.enc_case(X.ENC_ROWS[1], True), "conv_mx3"), (X.enc_case(X.ENC_ROWS[3], True), "conv_mx3_s2")]


@pytest.mark.parametrize("ck", PROPERTY_CASES, ids=[f"{c['id']}-{k}" for c, k in PROPERTY_CASES])
def test_second_call_and_single_sample_give_the_same_bits(ck):
    c, kernel = ck
    a = launch(c, kernel)
    b = launch(c, kernel)
    assert torch.equal(a, b), "a second call changed the bits"
    if c["bs"] > 1:
        last = c["bs"] - 1
        alone = launch(c, kernel, sl=slice(last, last + 1))
        assert torch.equal(alone[0], a[last]), "a sample's bits depend on its neighbours in the batch"
    ops.mx_overflowed()


@pytest.mark.parametrize("row", X.ENC_ROWS, ids=[r[0] for r in X.ENC_ROWS])
def test_three_input_formats_of_conv_mx3_give_the_same_bits(row):
    """fp32 planes, channel-blocked and prepared-operand inputs on the ragged cases (the prepared form takes no normalisation: f16-exact inputs, plain)."""
    kernel = "conv_mx3_s2" if row[6] == 2 else "conv_mx3"
    c = X.enc_case(row, True)
    assert torch.equal(launch_enc(c, kernel, fmt="c4"), launch_enc(c, kernel))
    p = X.enc_case(row, False)
    prep_ok = (p["h"] * p["w"]) % 4 == 0          # (a real restriction of the prepared-operand output)
    record_parity(f"mx_arith.formats.{row[0]}.prepared_form_run", int(prep_ok), None, "1: run; 0: h w % 4 != 0 (the ragged stride-1 prepared case is the 10 x 38 test below)")
    if prep_ok:
        xh = dev(p["x"].half().float())
        assert torch.equal(launch_enc(p, kernel, x=xh, fmt="prep"), launch_enc(p, kernel, x=xh))
        assert torch.equal(launch_enc(p, kernel, x=xh, fmt="c4"), launch_enc(p, kernel, x=xh))
    ops.mx_overflowed()


def test_ragged_prepared_operand_input_at_stride_1_gives_the_same_bits():
    """The 7 x 45 row cannot take the prepared form (h w % 4 != 0): a ragged stride-1 map that can — 10 x 38, a partial tile in both directions, an output-channel
    tail — through the three input formats."""
    g = torch.Generator().manual_seed(38)
    c = dict(cout=136, in_norm=None, prelu=None, W=torch.randn(136, 32, 3, 3, generator=g) / 17.0)
    xh = dev((torch.randn(2, 32, 10, 38, generator=g) * 2).half().float())
    plain = launch_enc(c, "conv_mx3", x=xh)
    assert torch.equal(launch_enc(c, "conv_mx3", x=xh, fmt="prep"), plain) and torch.equal(launch_enc(c, "conv_mx3", x=xh, fmt="c4"), plain)
    assert not ops.mx_overflowed()
