"""Every gradient kernel of the synthesis path alone (csrc/modconv_bwd.hip, csrc/gemm_sb.hip, csrc/mconv_dgrad.hip, csrc/linear.hip), against the float64
references of tests/grad_model.py, each case within the bar that tests/test_grad_model_cpu.py has shown to let stock float32 pass and to keep every mutant
outside.  One launch per case through ``lib().call`` on the C entry (so that chunk sizes, strides, alignments and null outputs are the case's own, not the ones
``ops_grad`` always passes); ``style_tables_bwd`` and ``grouped_linear`` also through their ``ops`` wrappers.  The split-bf16 operations are held three ways:
element-wise against float64, against the float64-accumulated emulation of their split under the class bar, and under the project's 3e-5 of max|ref|.  Every
figure goes to ``record_parity`` as ``gradkern.<op>.<case>.<output>`` (value = error / bar, tol 1; bar 0: the number of differing elements, tol 0) before it is
asserted, the worst per operation as ``gradkern.<op>.worst_err_over_bar``.

Operation (its cases: ``grad_model.CASES``) -> kernels it launches:
  mconv_unfold        mconv_unfold_kernel<1|3>
  unfold2d            unfold2d_kernel<1|3>
  mconv_scale         mconv_scale_kernel
  mconv_fold          mconv_fold4_kernel, mconv_fold_kernel<3>, mconv_fold_kernel<1>  (``grad_model.fold_route`` says which)
  style_tables_bwd    tables_bwd_s_kernel, tables_bwd_w_kernel, tables_bwd_mod_kernel
  gemm_sb             gemm_sb_kernel<*, *>, gemm_sb_skinny_kernel, gemm_sb_finalize_kernel, gemm_sb_finalize_wide_kernel
  mconv_wgrad         mconv_wgrad_kernel<1|3, 32|64|128> and the finalize kernels
  mconv_dgrad         mconv_dgrad_kernel
  grouped_linear      grouped_linear_kernel<vector | scalar>
  grouped_linear_bwd  grouped_linear_wgrad_kernel, grouped_linear_dgrad_kernel, grouped_linear_dgrad_finish_kernel
  small_map           small_map_kernel, small_map_fixed_kernel<36, 9, plain | grouped>
Beside the bars: what the kernels' headers promise bit for bit (a second call gives the same bits; a batch gives each sample the bits it gets alone; an empty
batch returns at once), poisoned outputs and guards behind them, and the refusals that come before a launch."""
import ctypes

import numpy as np
import pytest
import torch

import grad_model as M
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64
GUARD = 64
_WORST = {}


def dev(a, off=False):
    """On the device (None stays None); ``off``: as a view one float past a 16-byte boundary."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to(DEV)
    big = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    big[1:] = t.reshape(-1).to(DEV)
    return big[1:].view(t.shape)


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """An output filled with POISON with GUARD more floats of it behind: ``ok()`` says the guard is untouched."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.whole = torch.full((n + GUARD,), M.POISON, dtype=torch.float32, device=DEV)
        self.t = self.whole[:n].view(shape)

    def ok(self):
        return bool((self.whole[self.t.numel():] == M.POISON).all())

    def untouched(self):
        return bool((self.whole == M.POISON).all())


def _call(name, *args):
    """The entry point on the current stream; tensors are passed as they are, so that each lives until the call has been made."""
    from e4s2024_amd import ops
    from e4s2024_amd._lib import lib
    conv = [a.t if isinstance(a, Guarded) else a for a in args]
    lib().call(name, *[ops._p(a) if isinstance(a, torch.Tensor) else a for a in conv], ops._stream())


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _finish(outs):
    """{name: Guarded} -> {name: numpy}; every guard is intact."""
    torch.cuda.synchronize()
    for k, g in outs.items():
        assert g.ok(), f"{k}: written past its end"
    return {k: host(g.t) for k, g in outs.items()}


# ------------------------------------------------------------------------------------------------ one launch per operation
def run_unfold(inp, sample=None):
    x, s, lab = inp["x"], inp["s"], inp["lab"]
    if sample is not None:
        x, s, lab = x[sample:sample + 1], s[sample:sample + 1], None if lab is None else lab[sample:sample + 1]
    bs, cin, h, w = x.shape
    ks, up = inp["ks"], inp["up"]
    cols = Guarded(up * up, bs, cin * ks * ks, h * w)
    _call("e4s_mconv_unfold", cols, dev(x), dev(s), dev(lab), bs, cin, h, w, ks, inp["nreg"], up)
    return _finish({"cols": cols})


def run_unfold2d(inp):
    bs, C, hi, wi = inp["x"].shape
    ks, ho, wo = inp["ks"], inp["ho"], inp["wo"]
    cols = Guarded(bs, C * ks * ks, ho * wo)
    _call("e4s_unfold2d", cols, dev(inp["x"]), bs, C, hi, wi, ho, wo, ks, inp["stride"], inp["pad"])
    return _finish({"cols": cols})


def run_scale(inp, sample=None, chunk_px=None, noise_bs=None):
    gy, out, d, lab, noise = inp["gy"], inp["out"], inp["d"], inp["lab"], inp["noise"]
    if sample is not None:
        b = slice(sample, sample + 1)
        gy, out, d, lab = gy[b], None if out is None else out[b], None if d is None else d[b], None if lab is None else lab[b]
        noise = noise[b] if noise is not None and noise.shape[0] > 1 else noise
    bs, cout, H, W = gy.shape
    up, nreg = inp["up"], inp["nreg"]
    chunk = chunk_px or inp["chunk_px"]
    nchunk = M.cdiv(H * W, max(chunk, 1))
    outs = {"gz": Guarded(up * up, bs, cout, (H // up) * (W // up)), "dbias": Guarded(nchunk, bs, cout)}
    if inp["want_q"]:
        outs["q"] = Guarded(nchunk, bs, nreg, cout)
    if noise is not None:
        outs["dnw"] = Guarded(nchunk, bs, cout)
    _call("e4s_mconv_scale", outs["gz"], outs.get("q"), outs["dbias"], outs.get("dnw"), dev(gy), dev(out), dev(d), dev(lab), dev(noise),
          (0 if noise is None else noise.shape[0]) if noise_bs is None else noise_bs, dev(inp["nw"]), dev(inp["bias"]), int(inp["act"]), bs, cout, H // up, W // up, nreg, up, chunk)
    return _finish(outs)


def run_fold(inp, sample=None, chunk_px=None, u_off=False):
    U_, x, s, lab = inp["U_"], inp["x"], inp["s"], inp["lab"]
    if sample is not None:
        b = slice(sample, sample + 1)
        U_, x, s, lab = U_[:, b], x[b], s[b], None if lab is None else lab[b]
    bs, cin, h, w = x.shape
    chunk = chunk_px or inp["chunk_px"]
    outs = {}
    if inp["want_dx"]:
        outs["dx"] = Guarded(bs, cin, h, w)
    if inp["want_ds"]:
        outs["ds_part"] = Guarded(M.cdiv(h * w, max(chunk, 1)), bs, inp["nreg"], cin)
    _call("e4s_mconv_fold", outs.get("dx"), outs.get("ds_part"), dev(U_, off=u_off), dev(x), dev(s), dev(lab), bs, cin, h, w, inp["ks"], inp["nreg"], inp["up"], chunk)
    return _finish(outs)


def run_tables(inp):
    """``e4s_style_tables_bwd`` on the entry: absent gradients are null pointers, outputs nobody asks for as well."""
    import math
    styles, weight = inp["styles"], inp["weight"]
    bs, nreg, sdim = styles.shape
    cout, cin, k = weight.shape[1], weight.shape[2], weight.shape[-1]
    s, d, wsq = M.tables_given(**inp)
    have_s = inp["gs"] is not None or inp["gd"] is not None
    have_w = inp["gws"] is not None or inp["gd"] is not None
    outs = {}
    if have_s:
        outs.update(g_styles=Guarded(bs, nreg, sdim), g_mod_w=Guarded(cin, sdim), g_mod_b=Guarded(cin))
    if have_w:
        outs["g_weight"] = Guarded(1, cout, cin, k, k)
    scratch = Guarded(bs * nreg * (cout + cin))
    _call("e4s_style_tables_bwd", outs.get("g_styles"), outs.get("g_mod_w"), outs.get("g_mod_b"), outs.get("g_weight"), scratch, dev(inp["gs"]), dev(inp["gd"]), dev(inp["gws"]),
          dev(styles), dev(inp["mod_w"]), dev(s), dev(d), dev(weight), dev(wsq), 1.0 / math.sqrt(cin * k * k), inp["ms"], inp["lr"], bs * nreg, sdim, cin, cout, k * k)
    res = _finish(outs)
    assert scratch.ok()
    return res


def run_tables_ops(inp):
    """The same through ``ops.style_tables_saved`` and autograd (``d = None``: no demodulation)."""
    from e4s2024_amd import ops
    s, d, wsq = M.tables_given(**inp)
    leaves = [dev(inp[k]).requires_grad_() for k in ("styles", "weight", "mod_w", "mod_b")]
    with_d = inp["gd"] is not None
    s_out, ws, d_out = ops.style_tables_saved(*leaves, dev(s), dev(d) if with_d else None, dev(wsq), inp["ms"], inp["lr"])
    outs, gouts = [s_out, ws], [dev(inp["gs"]), dev(inp["gws"])]
    if with_d:
        outs.append(d_out)
        gouts.append(dev(inp["gd"]))
    g = torch.autograd.grad(outs, leaves, gouts)
    torch.cuda.synchronize()
    return dict(zip(("g_styles", "g_weight", "g_mod_w", "g_mod_b"), [host(t) for t in g]))


def run_gemm(inp, sample=None):
    a, b, M_, N_, K = inp["a"], inp["b"], inp["M"], inp["N"], inp["K"]
    batch = inp["batch"]
    if sample is not None:
        a, b, batch = a[min(sample, a.shape[0] - 1)][None], b[min(sample, b.shape[0] - 1)][None], 1
    c = Guarded(batch, M_, N_)
    ks = inp["ksplit"]
    ws = Guarded(ks * batch * M_ * N_) if inp["ws"] else None
    _call("e4s_gemm_sb", c, dev(a), dev(b), M_, N_, K, int(inp["a_kc"]), int(inp["b_kc"]), a.shape[2], b.shape[2], 0 if a.shape[0] == 1 and batch > 1 else a.shape[1] * a.shape[2],
          0 if b.shape[0] == 1 and batch > 1 else b.shape[1] * b.shape[2], M_ * N_, batch, ws, 0 if ws is None else ws.t.numel())
    res = _finish({"c": c})
    assert ws is None or ws.ok()
    return res


def run_wgrad(inp):
    G, bs, cout, P = inp["gz"].shape
    _, cin, h, w = inp["x"].shape
    ks = inp["ks"]
    n = cin * ks * ks
    dw = Guarded(G * bs, cout, n)
    ws = Guarded(inp["ksplit"] * G * bs * cout * n)
    _call("e4s_mconv_wgrad", dw, dev(inp["gz"]), dev(inp["x"]), dev(inp["s"]), dev(inp["lab"]), bs, cin, cout, h, w, ks, inp["nreg"], inp["up"], ws, ws.t.numel())
    res = _finish({"dw": dw})
    assert ws.ok()
    return res


def run_dgrad(inp):
    from e4s2024_amd._lib import lib
    G, bs, cout, P = inp["gz"].shape
    _, cin, h, w = inp["x"].shape
    ntile = lib().cdll.e4s_mconv_dgrad_tiles(h, w)
    assert ntile == M.cdiv(h, 6) * (1 if w == 32 else M.cdiv(w, 30))
    outs = {}
    if inp["want_dx"]:
        outs["dx"] = Guarded(bs, cin, h, w)
    if inp["want_ds"]:
        outs["part"] = Guarded(ntile, bs, inp["nreg"], cin)
    _call("e4s_mconv_dgrad", outs.get("dx"), outs.get("part"), dev(inp["gz"]), dev(inp["wg"]), dev(inp["x"]), dev(inp["s"]), dev(inp["lab"]), bs, cin, cout, h, w, inp["nreg"], inp["up"])
    res = _finish(outs)
    if "part" in res:
        res["ds"] = res.pop("part").astype(f64).sum(0)                  # (the caller's sum over the tiles, here without a rounding of its own)
    return res


def run_linear(inp, sample=None):
    from e4s2024_amd import ops
    x = inp["x"] if sample is None else inp["x"][sample:sample + 1]
    bs, groups, _ = x.shape
    o = inp["W"][0].shape[0]
    route = inp["route"]
    W = [dev(w) for w in inp["W"]]
    bias = None if inp["bias"] is None else [dev(b) for b in inp["bias"]]
    wide = Guarded(bs, groups, o + 8) if route["outslice"] else Guarded(bs, groups, o)
    out = wide.t[:, :, 3:3 + o] if route["outslice"] else wide.t
    xd = dev(x, off=route["xoff"] == 1)
    if route["xoff"] == 2:                                               # rows in + 1 floats apart: an odd stride
        spaced = torch.zeros(bs, groups, x.shape[2] + 1, dtype=torch.float32, device=DEV)
        spaced[:, :, :-1] = xd
        xd = spaced[:, :, :-1]
    got = ops.grouped_linear(xd, W, bias, scale=inp["scale"], bias_mul=inp["bias_mul"], act=inp["act"], slope=inp["slope"],
                             addend=dev(inp["addend"]), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and wide.ok()
    if route["outslice"]:
        rest = torch.ones_like(wide.t, dtype=torch.bool)
        rest[:, :, 3:3 + o] = False
        assert bool((wide.t[rest] == M.POISON).all()), "written outside the slice"
    return {"out": host(out)}


def run_linbwd(inp):
    gy, x, W = inp["gy"], inp["x"], inp["W"]
    bs, g, i = x.shape
    o = W[0].shape[0]
    want = inp["want"]
    outs = {}
    if "dW" in want:
        outs["dW"] = Guarded(g, o, i)
    if "db" in want:
        outs["db"] = Guarded(g, o)
    if "dx" in want:
        outs["dx"] = Guarded(bs, g, i)
    scratch = Guarded(inp["osplit"] * bs * g * i)
    Wd = [dev(w) for w in W]
    xd = dev(x)
    _call("e4s_grouped_linear_bwd", outs.get("dW"), outs.get("db"), outs.get("dx"), scratch, dev(gy), xd, _ptrs(Wd), xd if inp["h_prev"] is not None else None, inp["scale"],
          inp["bias_mul"], inp["slope"], bs, g, i, o, inp["osplit"])
    res = _finish(outs)
    assert scratch.ok()
    return res


def run_small(inp):
    J, K = inp["Tm"].shape
    src = inp["src"]
    n = src.size // (J if inp["trans"] else K)
    shape = (n, K) if inp["trans"] else ((J // 9, n, 9) if inp["grouped"] else (J, n))
    out = Guarded(*shape)
    _call("e4s_small_map", out, dev(inp["Tm"]), dev(src), J, K, n, int(inp["trans"]), int(inp["grouped"]))
    return _finish({"out": out})


RUN = {"mconv_unfold": run_unfold, "unfold2d": run_unfold2d, "mconv_scale": run_scale, "mconv_fold": run_fold, "style_tables_bwd": run_tables, "gemm_sb": run_gemm,
       "mconv_wgrad": run_wgrad, "mconv_dgrad": run_dgrad, "grouped_linear": run_linear, "grouped_linear_bwd": run_linbwd, "small_map": run_small}


def run(op, inp, name=None, **kw):
    if op == "mconv_fold" and name is not None:
        kw.setdefault("u_off", bool(M.case(op, name)["u_off"]))          # (the case that reaches the scalar kernel by a misaligned U)
    return RUN[op](inp, **kw)


# ------------------------------------------------------------------------------------------------ the bars
def hold(op, name, got, ref, bar, tag=""):
    """Records error / bar of every output of ``got`` (bar 0: the count of differing elements) and asserts it."""
    bad = []
    for k, g in got.items():
        b = np.broadcast_to(np.asarray(bar[k], f64), np.shape(ref[k]))
        key = f"gradkern.{op}.{name}.{k}{tag}"
        if not b.any():
            ndiff = int((np.asarray(g, f64) != ref[k]).sum()) if np.shape(g) == np.shape(ref[k]) else -1
            record_parity(key, ndiff, 0.0, "elements that differ from the float32 expression")
            if ndiff != 0:
                bad.append((k, ndiff))
            continue
        r = M.ratio({k: g}, ref, bar)
        record_parity(key, r, 1.0, f"max |err| {np.abs(np.asarray(g, f64) - ref[k]).max():.3e}")
        _WORST[op] = max(_WORST.get(op, 0.0), r)
        record_parity(f"gradkern.{op}.worst_err_over_bar", _WORST[op], 1.0)
        if not r <= 1.0:
            bad.append((k, r))
    assert not bad, (op, name, tag, bad)


def hold_split(op, name, got, inp, ref):
    """A split-bf16 output against the float64-accumulated emulation under the class bar, and against float64 under 3e-5 of max|ref| (descaled where the
    case scales its rows and columns by powers of two)."""
    emu, cbar = M.built_class(op, name)
    bad = []
    for k, g in got.items():
        gd, rd, ed = M.descaled(np.asarray(g, f64), inp), M.descaled(ref[k], inp), M.descaled(emu[k], inp)
        r_emu = np.abs(gd - ed).max() / cbar[k]
        r_out = np.abs(gd - rd).max() / np.abs(rd).max()
        record_parity(f"gradkern.{op}.{name}.{k}.vs_emulate", r_emu, 1.0, f"class bar {cbar[k]:.3e}")
        record_parity(f"gradkern.{op}.{name}.{k}.rel_vs_fp64", r_out, M.OUTER)
        _WORST[op + ".outer"] = max(_WORST.get(op + ".outer", 0.0), r_out / M.OUTER)
        record_parity(f"gradkern.{op}.worst_rel_vs_fp64_over_3e-5", _WORST[op + ".outer"], 1.0)
        if not (r_emu <= 1.0 and r_out <= M.OUTER):
            bad.append((k, r_emu, r_out))
    assert not bad, (op, name, bad)


def same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == f32 else a[k], b[k].view(np.uint32) if b[k].dtype == f32 else b[k]) for k in a)


ALL = [(op, name) for op in M.CASES for name in M.case_names(op)]


@pytest.mark.parametrize("op,name", ALL, ids=[f"{o}-{n}" for o, n in ALL])
def test_kernel_against_float64_within_the_bar_of_its_case(op, name):
    inp, ref, bar = M.built(op, name)
    got = run(op, inp, name)
    assert set(got) == set(ref), (set(got), set(ref))
    assert all(np.isfinite(v).all() and not (v == M.POISON).any() for v in got.values()), "an element was not written"
    hold(op, name, got, ref, bar)
    if op in M.SPLIT_OPS:
        hold_split(op, name, got, inp, ref)
    assert same_bits(got, run(op, inp, name)), "a second call gives other bits"


def test_pixels_of_no_region_get_a_zero_gradient_and_still_count_in_the_sums():
    """``mconv_scale``: a label in [nreg, 16) or 255 gives gz == 0 exactly; with every label that of no region, dbias and dnw are what they are with every
    pixel in region 0 of a unit d (bit for bit: the sums do not look at the label) and q is all zeros."""
    name = "17x19.act1.d.noiseB.bias.up1.r5.q.c256"
    inp, _, _ = M.built("mconv_scale", name)
    got = run_scale(inp)
    stray = (inp["lab"] >= inp["nreg"]).reshape(inp["lab"].shape[0], 1, -1)
    assert stray.any() and (inp["lab"] == 255).any() and ((inp["lab"] >= inp["nreg"]) & (inp["lab"] < 16)).any()
    gz = got["gz"][0]
    assert not gz[np.broadcast_to(stray, gz.shape)].any() and gz[np.broadcast_to(~stray, gz.shape)].all()
    none = run_scale(dict(inp, lab=np.full_like(inp["lab"], 255)))
    zero = run_scale(dict(inp, lab=np.zeros_like(inp["lab"])))
    assert not none["gz"].any() and not none["q"].any()
    assert np.array_equal(none["dbias"], zero["dbias"]) and np.array_equal(none["dnw"], zero["dnw"]) and np.array_equal(none["dbias"], got["dbias"])


# ------------------------------------------------------------------------------------------------ routes and wrappers held to each other
VEC = [c["name"] for c in M.CASES["mconv_fold"] if c["route"] == "vec"]


@pytest.mark.parametrize("name", VEC)
def test_fold_vector_route_against_the_scalar_route(name):
    """The same case through mconv_fold4_kernel (the case's own launch), through mconv_fold_kernel<3> by a 256-pixel chunk and by a U one float past a 16-byte
    boundary: dx and the chunk-summed ds within the sum of the two routes' bars; the two scalar launches' dx bit for bit (dx does not depend on the chunking)."""
    c = M.case("mconv_fold", name)
    inp, ref, bar = M.built("mconv_fold", name)
    vec = run("mconv_fold", inp)
    by_chunk = run_fold(inp, chunk_px=256)
    by_align = run_fold(inp, u_off=True)
    inp256 = dict(inp, chunk_px=256, D=dict(dx=c["D"]["dx"], ds_part=M.depth("fold_ds", up=c["up"], ks=3, chunk_px=256, px=c["h"] * c["w"])))
    ref256, bar256 = M.fold_ref(**inp256), M.fold_bar(**inp256)
    hold("mconv_fold", name, by_chunk, ref256, bar256, ".scalar_by_chunk")
    hold("mconv_fold", name, by_align, ref, bar, ".scalar_by_alignment")
    tot = lambda d: {k: (v.astype(f64).sum(0) if k == "ds_part" else v.astype(f64)) for k, v in d.items()}               # noqa: E731
    both = {k: tot(bar)[k] + tot(bar256)[k] for k in vec}
    hold("mconv_fold", name, tot(by_chunk), tot(vec), both, ".scalar_vs_vector")
    if "dx" in vec:
        assert np.array_equal(by_chunk["dx"], by_align["dx"])


@pytest.mark.parametrize("name", [c["name"] for c in M.CASES["style_tables_bwd"] if c["have"] in ("all", "nogd")])
def test_style_tables_through_the_autograd_function(name):
    inp, ref, bar = M.built("style_tables_bwd", name)
    got = run_tables_ops(inp)
    hold("style_tables_bwd", name, got, ref, bar, ".ops")
    assert same_bits(got, run_tables(inp)), "ops.style_tables_saved and the entry disagree"


@pytest.mark.parametrize("name", M.case_names("mconv_wgrad"))
def test_implicit_weight_gradient_equals_unfold_then_gemm(name):
    """``e4s_mconv_wgrad`` against ``e4s_mconv_unfold`` / ``e4s_unfold2d`` followed by ``e4s_gemm_sb``: the same split of the same float32 operands, apart only in
    the order of their float32 sums, so within half a class bar of each other (the share tests/test_grad_model_cpu.py allows float32 accumulation)."""
    from e4s2024_amd import ops
    inp, ref, bar = M.built("mconv_wgrad", name)
    got = run_wgrad(inp)["dw"]
    x, gz = dev(inp["x"]), dev(inp["gz"])
    G, bs, cout, P = inp["gz"].shape
    if inp["s"] is not None:
        cols = ops._mconv_unfold(x, dev(inp["s"]), dev(inp["lab"]), inp["ks"], inp["up"])
    else:
        cols = ops.unfold2d(x, inp["ks"], 1, inp["ks"] // 2, x.shape[2], x.shape[3])[None]
    pair = host(ops.gemm_sb(gz.reshape(G * bs, cout, P), cols.reshape(G * bs, -1, P), True, True))
    hold("mconv_wgrad", name, {"dw": pair}, ref, bar, ".unfold_gemm")
    _, cbar = M.built_class("mconv_wgrad", name)
    r = np.abs(got.astype(f64) - pair).max() / cbar["dw"]
    record_parity(f"gradkern.mconv_wgrad.{name}.dw.vs_unfold_gemm", r, 0.5)
    assert r <= 0.5


@pytest.mark.parametrize("name", M.case_names("mconv_dgrad"))
def test_fused_data_gradient_against_the_unfused_pair(name):
    from e4s2024_amd import ops, ops_grad
    inp, ref, bar = M.built("mconv_dgrad", name)
    fused = run_dgrad(inp)
    keep = ops.DGRAD_FUSED
    ops.DGRAD_FUSED = False
    try:
        dx, ds, _ = ops_grad._mconv_input_grads(dev(inp["gz"]), dev(inp["wg"]), dev(inp["x"]), dev(inp["s"]), dev(inp["lab"]), inp["up"], inp["want_dx"], inp["want_ds"], False)
    finally:
        ops.DGRAD_FUSED = keep
    pair = {k: host(v).astype(f64) for k, v in (("dx", dx), ("ds", ds)) if v is not None}
    hold("mconv_dgrad", name, pair, ref, bar, ".unfused")
    for k in fused:
        r = np.abs(fused[k].astype(f64) - pair[k]).max() / np.abs(ref[k]).max()
        record_parity(f"gradkern.mconv_dgrad.{name}.{k}.rel_vs_unfused", r, M.OUTER)
        assert r <= M.OUTER


def test_local_mlps_and_equal_linear_gradients_against_float64():
    """``_LocalMLPsGrad`` and ``_EqualLinearGrad`` (the two callers of ``e4s_grouped_linear_bwd``) once each against float64 autograd of the reference's
    LocalMLP (networks.py:23-49) and EqualLinear (model.py:154-162), under the bars of the kernels they chain: the float32 hidden value carries the forward
    kernel's roundings into dW2, the float32 gradient of the hidden layer carries the second layer's into dW0, db0 and dx (D adds up along the chain, the
    magnitudes are those of the whole chain in absolute values, the slope taken as 1)."""
    import math
    import torch.nn.functional as F
    from e4s2024_amd import ops
    from e4s2024_amd.ops_grad import equal_linear_grad, local_mlps_grad
    bs, n, i0, hid, o2, slope, lr = 3, 5, 1028, 36, 13, 0.2, 0.6
    x, g = M.arr("mlpx", (bs, n, i0)), M.arr("mlpg", (bs, n, o2))
    W0, b0 = [M.arr(f"mlpw0{k}", (hid, i0)) for k in range(n)], [M.arr(f"mlpb0{k}", (hid,)) for k in range(n)]
    W2, b2 = [M.arr(f"mlpw2{k}", (o2, hid)) for k in range(n)], [M.arr(f"mlpb2{k}", (o2,)) for k in range(n)]
    sc0, sc2 = 1.0 / math.sqrt(i0), 1.0 / math.sqrt(hid)
    # float64
    leaves = [M.T(np.stack(a)).requires_grad_() for a in (W0, b0, W2, b2)] + [M.T(x).requires_grad_()]
    h = F.leaky_relu(torch.einsum("goi,bgi->bgo", leaves[0], leaves[4]) * sc0 + leaves[1][None] * lr, slope)
    y = torch.einsum("goi,bgi->bgo", leaves[2], h) * sc2 + leaves[3][None] * lr
    want = [M.N(t) for t in torch.autograd.grad((y * M.T(g)).sum(), leaves)]
    # bars: U x (roundings) x sum|terms| of each gradient in absolute values, the hidden layer's terms carrying both layers' roundings
    al = [M.T(np.abs(np.stack(a))).requires_grad_() for a in (W0, b0, W2, b2)] + [M.T(np.abs(x)).requires_grad_()]
    ha = torch.einsum("goi,bgi->bgo", al[0], al[4]) * sc0 + al[1][None] * lr
    ya = torch.einsum("goi,bgi->bgo", al[2], ha) * sc2 + al[3][None] * lr
    mags = [M.N(t) for t in torch.autograd.grad((ya * M.T(np.abs(g))).sum(), al)]
    D_h = M.depth("linear", n=i0, vec=True) + 6                         # the forward h
    D_gy0 = M.depth("lin_dx", out=o2, osplit=32)                        # dL/dh through layer 2
    Ds = [D_gy0 + bs + 1, D_gy0 + bs + 1, D_h + bs + 1, bs + 1, D_gy0 + M.depth("lin_dx", out=hid, osplit=8)]
    # the device
    xd = dev(x).requires_grad_()
    params = [[dev(a).requires_grad_() for a in grp] for grp in (W0, b0, W2, b2)]
    with torch.no_grad():
        hd = ops.grouped_linear(xd, params[0], params[1], scale=sc0, bias_mul=lr, act=1, slope=slope)
        od = ops.grouped_linear(hd, params[2], params[3], scale=sc2, bias_mul=lr, act=0)
    out = local_mlps_grad(xd, od, hd, params[0], params[1], params[2], params[3], sc0, sc2, lr, lr, slope)
    grads = torch.autograd.grad(out, [t for grp in params for t in grp] + [xd], dev(g))
    torch.cuda.synchronize()
    got = [np.stack([host(t) for t in grads[k * n:(k + 1) * n]]) for k in range(4)] + [host(grads[4 * n])]
    for nm, a, r, m, D in zip(("dW0", "db0", "dW2", "db2", "dx"), got, want, mags, Ds):
        hold("local_mlps_grad", f"b{bs}.n{n}.in{i0}.hid{hid}.out{o2}", {nm: a}, {nm: r}, {nm: D * M.U * m})
    # EqualLinear: one group, bs <= 8
    bs, i, o = 8, 512, 24
    x, w, b, g = M.arr("eqx", (bs, i)), M.arr("eqw", (o, i)), M.arr("eqb", (o,)), M.arr("eqg", (bs, o))
    sc = 1.0 / math.sqrt(i)
    lv = [M.T(a).requires_grad_() for a in (x, w, b)]
    want = [M.N(t) for t in torch.autograd.grad(((lv[0] @ lv[1].t() * sc + lv[2] * lr) * M.T(g)).sum(), lv)]
    la = [M.T(np.abs(a)).requires_grad_() for a in (x, w, b)]
    mags = [M.N(t) for t in torch.autograd.grad(((la[0] @ la[1].t() * sc + la[2] * lr) * M.T(np.abs(g))).sum(), la)]
    ld = [dev(a).requires_grad_() for a in (x, w, b)]
    grads = torch.autograd.grad(equal_linear_grad(ld[0], ld[1], ld[2], sc, lr), ld, dev(g))
    torch.cuda.synchronize()
    for nm, a, r, m, D in zip(("dx", "dW", "db"), grads, want, mags, (M.depth("lin_dx", out=o, osplit=8), bs + 1, bs + 1)):
        hold("equal_linear_grad", f"b{bs}.in{i}.out{o}", {nm: host(a)}, {nm: r}, {nm: D * M.U * m})


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("op,name", [("mconv_unfold", "b2.c3.5x7.k3.up2.r16.stray"), ("mconv_scale", "17x19.act1.d.noiseB.bias.up2.r16.q.c512"),
                                     ("mconv_scale", "27x19.act1.d.noise1.bias.up1.r5.q.c256.3chunks"), ("mconv_fold", "3x4.k3.up2.r5.lab.vec.both"),
                                     ("mconv_fold", "9x7.k3.up2.r5.lab.w7.both"), ("gemm_sb", "kc_mc.200x70x100.b3.share_a.ktail"), ("gemm_sb", "kc_kc.8x257x64.b2.skinny"),
                                     ("gemm_sb", "mc_mc.70x50x40.b2.lda"), ("grouped_linear", "b17.g16.in260.out7.act1.vec"), ("grouped_linear", "b16.g2.in30.out7.act1.nobias.scalar")])
def test_a_sample_in_a_batch_gets_the_bits_it_gets_alone(op, name):
    inp, _, _ = M.built(op, name)
    assert op != "gemm_sb" or inp["ksplit"] == 1                         # (a split depends on the batch: fewer workgroups, more slices)
    whole = run(op, inp, name)
    batch_axis = {"mconv_unfold": {"cols": 1}, "mconv_scale": {"gz": 1, "q": 1, "dbias": 1, "dnw": 1}, "mconv_fold": {"dx": 0, "ds_part": 1}, "gemm_sb": {"c": 0},
                  "grouped_linear": {"out": 0}}[op]
    nb = whole[next(iter(batch_axis))].shape[batch_axis[next(iter(batch_axis))]]
    assert nb > 1
    for b in range(nb):
        alone = run(op, inp, name, sample=b)
        for k, ax in batch_axis.items():
            if k in whole:
                assert np.array_equal(np.take(whole[k], [b], ax), alone[k]), (k, b)


def test_an_empty_batch_returns_at_once():
    """bs = 0 (``small_map``: N = 0): status 0 and not one element written."""
    out, t = Guarded(64), torch.zeros(64, dtype=torch.float32, device=DEV)
    lab = torch.zeros(64, dtype=torch.uint8, device=DEV)
    _call("e4s_unfold2d", out, t, 0, 2, 4, 4, 4, 4, 3, 1, 1)
    _call("e4s_mconv_unfold", out, t, t, lab, 0, 2, 4, 4, 3, 5, 1)
    _call("e4s_mconv_scale", out, out, out, out, t, t, t, lab, t, 1, t, t, 1, 0, 2, 4, 4, 5, 1, 256)
    _call("e4s_mconv_fold", out, out, t, t, t, lab, 0, 2, 4, 4, 3, 5, 1, 1024)
    _call("e4s_gemm_sb", out, t, t, 4, 4, 4, 1, 1, 4, 4, 16, 16, 16, 0, out, 64)
    _call("e4s_mconv_wgrad", out, t, t, t, lab, 0, 2, 2, 1, 16, 3, 5, 1, out, 64)
    _call("e4s_mconv_dgrad", out, out, t, t, t, t, lab, 0, 2, 2, 1, 32, 5, 1)
    _call("e4s_grouped_linear", out, 8, 4, t, 8, 4, _ptrs([t, t]), None, None, 1.0, 1.0, 0, 0.2, 0, 2, 4, 4)
    _call("e4s_small_map", out, t, t, 5, 7, 0, 0, 0)
    torch.cuda.synchronize()
    assert out.untouched()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch():
    """Each refusal is the library's own error, and the outputs are as they were."""
    out, t = Guarded(4096), torch.zeros(4096, dtype=torch.float32, device=DEV)
    lab = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    refused = [
        ("chunk_px must be a multiple of 256", "e4s_mconv_scale", (out, None, out, None, t, None, None, lab, None, 0, None, None, 0, 1, 2, 17, 19, 5, 1, 300)),
        ("chunk_px must be a multiple of 256", "e4s_mconv_scale", (out, None, out, None, t, None, None, lab, None, 0, None, None, 0, 1, 2, 17, 19, 5, 1, 0)),
        ("chunk_px must be a multiple of 256", "e4s_mconv_fold", (out, out, t, t, t, lab, 1, 2, 5, 8, 3, 5, 1, 384)),
        ("noise needs its weight and batch 1 or bs", "e4s_mconv_scale", (out, None, out, out, t, None, None, lab, t, 2, t, None, 0, 3, 2, 4, 4, 5, 1, 256)),
        ("noise needs its weight and batch 1 or bs", "e4s_mconv_scale", (out, None, out, out, t, None, None, lab, t, 1, None, None, 0, 3, 2, 4, 4, 5, 1, 256)),
        ("w must be a multiple of 16", "e4s_mconv_wgrad", (out, t, t, t, lab, 1, 2, 2, 2, 24, 3, 5, 1, None, 0)),
        ("up = 2 is the masked composed form", "e4s_mconv_wgrad", (out, t, t, None, None, 1, 2, 2, 2, 16, 3, 1, 2, None, 0)),
        ("several regions need a label map", "e4s_mconv_wgrad", (out, t, t, t, None, 1, 2, 2, 2, 16, 3, 5, 1, None, 0)),
        ("grouped_linear_bwd: bad size", "e4s_grouped_linear_bwd", (out, out, out, out, t, t, _ptrs([t]), None, 1.0, 1.0, 0.2, 9, 1, 8, 4, 8)),
        ("grouped_linear_bwd: bad size", "e4s_grouped_linear_bwd", (out, out, out, out, t, t, _ptrs([t]), None, 1.0, 1.0, 0.2, 2, 1, 6, 4, 8)),
        ("grouped layout is built for J = 36, K = 9", "e4s_small_map", (out, t, t, 5, 7, 16, 0, 1)),
        ("leading dimension smaller than the row", "e4s_gemm_sb", (out, t, t, 8, 8, 8, 1, 1, 4, 8, 64, 64, 64, 1, None, 0)),
        ("the per-region sums and the activation gradient need the forward output", "e4s_mconv_scale", (out, None, out, None, t, None, None, lab, None, 0, None, None, 1, 1, 2, 4, 4, 5, 1, 256)),
    ]
    for msg, entry, args in refused:
        with pytest.raises(RuntimeError, match=msg.replace("(", r"\(").replace(")", r"\)")):
            _call(entry, *args)
    torch.cuda.synchronize()
    assert out.untouched()
