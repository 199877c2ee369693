"""The streaming kernels between the convolutions (csrc/norm.hip, ``gate_add_up_kernel`` and ``tensor2im_kernel`` of csrc/parser.hip) through their ``ops``
wrappers against the float64 references of tests/glue_model.py, each case within the bar that tests/test_glue_model_cpu.py has shown to let stock float32 pass and
to keep every mutant at least two bars away.  One launch or two per case; the worst error / bar per operation goes to ``record_parity``.  Also: ``se_gate``
equals two ``vec_fc`` calls and the statistics-emitting ``norm_gate_add`` equals the separate launches bit for bit at these shapes, and the wrappers refuse
vectors of the wrong dtype, stride or length before they launch."""
import numpy as np
import pytest
import torch

import glue_model as M
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = [(op, name) for op in M.CASES for name in M.case_names(op)]
_WORST = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _bn(bn):
    gamma, beta, mean, var, eps = bn
    m = torch.nn.BatchNorm2d(len(gamma), eps=eps)
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(gamma))
        m.bias.copy_(torch.from_numpy(beta))
        m.running_mean.copy_(torch.from_numpy(mean))
        m.running_var.copy_(torch.from_numpy(var))
    return m.eval().to(DEV)


def _nga_args(inp):
    return dict(mean=dev(inp["mean"]), rstd=dev(inp["rstd"]), gate=dev(inp["gate"]), shortcut=dev(inp["shortcut"]),
                sc_stats=None if inp["sc_stats"] is None else (dev(inp["sc_stats"][0]), dev(inp["sc_stats"][1])), sc_stride=inp["ss"], prelu=dev(inp["prelu"]))


def run(op, inp):
    """The case through the ``ops`` wrapper: {output name: numpy array}, named as the model names them."""
    from e4s2024_amd import ops
    if op == "plane_stats":
        x = dev(inp["x"])
        if inp["mode"] == "mean":
            return {"mean": host(ops.plane_stats(x))}
        res = ops.plane_stats(x, inp["eps"], want_nmean=inp["mode"] == "nmean")
        return dict(zip(("mean", "rstd", "nmean"), (host(t) for t in res)))
    if op == "vec_fc":
        return {"y": host(ops.vec_fc(dev(inp["x"]), dev(inp["w"]), bn=None if inp["bn"] is None else _bn(inp["bn"]), act=inp["act"]))}
    if op == "se_gate":
        return {"gate": host(ops.se_gate(dev(inp["pooled"]), dev(inp["w1"]), dev(inp["w2"])))}
    if op.startswith("norm_gate_add"):
        res = ops.norm_gate_add(dev(inp["x"]), stats_eps=inp["stats_eps"], self_eps=inp["self_eps"], **_nga_args(inp))
        if inp["stats_eps"] is None:
            return {"out": host(res)}
        return dict(zip(("out", "omean", "orstd"), (host(t) for t in res)))
    if op == "masked_avg_pool":
        return {"out": host(ops.masked_avg_pool(dev(inp["feats"]), dev(inp["labels"]), inp["nreg"]))}
    if op == "bilinear_resize":
        return {"out": host(ops.bilinear_resize(dev(inp["x"]), inp["size"], align_corners=inp["align"]))}
    if op == "gate_add_upsample":
        return {"out": host(ops.gate_add_upsample(dev(inp["feat"]), gate=dev(inp["gate"]), add_map=dev(inp["add_map"]), add_vec=dev(inp["add_vec"]), up=inp["up"]))}
    if op == "tensor2im_u8":
        return {"out": host(ops.tensor2im_u8(dev(inp["img"])))}
    raise KeyError(op)


@pytest.mark.parametrize("op,name", ALL, ids=[f"{o}-{n}" for o, n in ALL])
def test_kernel_within_the_bar_of_its_float64_reference(op, name):
    inp, ref, bar = M.built(op, name)
    got = run(op, inp)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    if op == "plane_stats" and inp["mode"] == "nmean":
        _, ref, bar = M.with_emitted(inp, got)              # nmean belongs to the (mean, rstd) emitted with it, which have bars of their own
    for k, r in ref.items():
        assert got[k].shape == r.shape and (got[k].dtype == np.uint8) == (op == "tensor2im_u8"), (k, got[k].shape, got[k].dtype)
    per = {k: M.ratio({k: got[k]}, {k: ref[k]}, {k: bar[k]}) for k in ref}
    worst = max(per.values())
    print(f"{op} {name}: " + ", ".join(f"{k} at {v:.3f} of its bar" for k, v in per.items()))
    _WORST[op] = max(_WORST.get(op, 0.0), worst)
    record_parity(f"glue.{op}.worst_err_over_bar", _WORST[op], tol=1.0, note="worst error / bar over the cases run so far (tests/glue_model.py)")
    assert worst <= 1.0, (op, name, per)


@pytest.mark.parametrize("name", M.case_names("se_gate"))
def test_se_gate_is_two_vec_fc_calls_bit_for_bit(name):
    from e4s2024_amd import ops
    inp = M.built("se_gate", name)[0]
    p, w1, w2 = dev(inp["pooled"]), dev(inp["w1"]), dev(inp["w2"])
    two = ops.vec_fc(ops.vec_fc(p, w1, act=ops.ACT_RELU), w2, act=ops.ACT_SIGMOID)
    assert torch.equal(ops.se_gate(p, w1, w2), two)


@pytest.mark.parametrize("name", M.case_names("norm_gate_add_stats"))
def test_statistics_emitting_form_is_the_separate_launches_bit_for_bit(name):
    """``norm_gate_add(stats_eps=...)`` against ``norm_gate_add`` + ``plane_stats`` of its result: ``out`` and ``mean`` bit for bit (the same thread -> element
    mapping and the same sums), at the ragged plane sizes too."""
    from e4s2024_amd import ops
    inp = M.built("norm_gate_add_stats", name)[0]
    x, args = dev(inp["x"]), _nga_args(inp)
    sep = ops.norm_gate_add(x, **args)
    mean = ops.plane_stats(sep, inp["stats_eps"])[0]
    out, om, _ = ops.norm_gate_add(x, stats_eps=inp["stats_eps"], **args)
    assert torch.equal(out, sep) and torch.equal(om, mean)


# ------------------------------------------------------------------------------------------------ the wrappers' checks
def _bad(n):
    """Three tensors that are NOT a contiguous float32 vector of ``n`` elements, each with at least 4 n bytes behind its pointer (whatever a wrapper without the
    check would hand to a kernel stays inside an allocation): float64, a strided view, one element too many."""
    return {"float64": torch.ones(n, dtype=torch.float64, device=DEV), "strided": torch.ones(2 * n, device=DEV)[::2], "too long": torch.ones(n + 1, device=DEV)}


@pytest.mark.parametrize("arg", ["gate", "mean", "rstd", "sc_mean", "sc_rstd", "prelu"])
def test_norm_gate_add_refuses_a_malformed_vector(arg):
    from e4s2024_amd import ops
    bs, C, h, w = 2, 3, 4, 4
    good = lambda n: torch.ones(n, device=DEV)                   # noqa: E731
    x, sc = torch.zeros(bs, C, h, w, device=DEV), torch.zeros(bs, C, h, w, device=DEV)
    n = C if arg == "prelu" else bs * C
    for kind, bad in _bad(n).items():
        v = {k: good(C if k == "prelu" else bs * C) for k in ("gate", "mean", "rstd", "sc_mean", "sc_rstd", "prelu")}
        v[arg] = bad
        with pytest.raises((TypeError, ValueError), match=arg.replace("_", ".")):
            ops.norm_gate_add(x, v["mean"], v["rstd"], v["gate"], sc, (v["sc_mean"], v["sc_rstd"]), 1, v["prelu"])
        for form in (dict(stats_eps=1e-5), dict(stats_eps=1e-5, self_eps=1e-5)):
            if "self_eps" in form and arg in ("mean", "rstd"):
                continue
            m, r = (None, None) if "self_eps" in form else (v["mean"], v["rstd"])
            with pytest.raises((TypeError, ValueError), match=arg.replace("_", ".")):
                ops.norm_gate_add(x, m, r, v["gate"], sc, (v["sc_mean"], v["sc_rstd"]), 1, v["prelu"], **form)
    assert ops.norm_gate_add(x, good(bs * C).view(bs, C), good(bs * C).view(bs, C, 1, 1), good(bs * C), sc, (good(bs * C), good(bs * C)), 1, good(C)).shape == x.shape


@pytest.mark.parametrize("arg", ["gate", "add_vec"])
def test_gate_add_upsample_refuses_a_malformed_vector(arg):
    from e4s2024_amd import ops
    bs, C = 2, 3
    feat = torch.zeros(bs, C, 4, 5, device=DEV)
    for kind, bad in _bad(bs * C).items():
        v = {"gate": torch.ones(bs * C, device=DEV), "add_vec": torch.ones(bs, C, device=DEV)}
        v[arg] = bad
        with pytest.raises((TypeError, ValueError), match=arg):
            ops.gate_add_upsample(feat, gate=v["gate"], add_vec=v["add_vec"], up=2)


def test_vec_fc_se_gate_and_masked_avg_pool_check_their_shapes():
    from e4s2024_amd import ops
    w = torch.zeros(5, 8, 1, 1, device=DEV)
    for shape in ((2, 9), (2, 7, 2), (2, 8, 1, 1), (3, 8, 2)):                      # each at least bs * cin floats
        with pytest.raises(ValueError, match="vec_fc"):
            ops.vec_fc(torch.zeros(shape, device=DEV), w)
    with pytest.raises(ValueError, match="se_gate"):
        ops.se_gate(torch.zeros(2, 8, 1, 1, device=DEV), torch.zeros(2, 8, device=DEV), torch.zeros(8, 2, device=DEV))
    feats = torch.zeros(2, 4, 8, 8, device=DEV)
    for lab in (torch.zeros(3, 16, 16, dtype=torch.uint8, device=DEV), torch.zeros(2, 1, 16, 16, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError, match="masked_avg_pool"):
            ops.masked_avg_pool(feats, lab, 12)
