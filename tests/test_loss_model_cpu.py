"""The bars of tests/test_gpu_loss_kernels.py separate right from wrong before any kernel runs: on the CPU model of the loss-term kernels
(tests/loss_model.py) stock float32 PyTorch and the float32 emulation of every kernel's own chain and tree sit inside the bar of every case, and every
mutant of an operation sits at least twice the bar outside it on at least one case of that operation's table.  Prints which case kills which mutant.
The tie rule of the pooling backward ("the first maximum in row-major window order") is checked against float64 CPU autograd of ``max_pool2d``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_model as M

ALL = [(op, name) for op in M.CASES for name in M.case_names(op)]


def test_case_tables_hold_the_depths_read_from_the_code():
    assert M.depth("conv1") == 363 + 1 and M.depth("dgrad") == 576 + 2 and M.depth("slices", 13) == 2 + 8 and M.depth("block", 257) == 2 + 8
    assert M.depth("hblock", 20000) == 32 + 8 and M.depth("wave", 1024) == 16 + 6 and M.depth("lin_t", 5) == 2 + 3 and M.depth("px", 9000, 3) == 48 + 8 + 2
    for op in M.CASES:
        assert len(set(M.case_names(op))) == len(M.CASES[op]), op
        assert set(M.MUTANTS[op]), op
        for name in M.case_names(op):
            M.built(op, name)                                        # (the builders assert D == depth(...))
    # the cosine heads' input pairs are what their names say
    for op in ("id_head", "id_head_multi"):
        for c in M.CASES[op]:
            cos = M.built(op, c["name"])[1]["stats"][:, :, 2:2 + 2 * c["k"]:2][[t for t, D in enumerate(c["Ds"]) if D > 1]]
            assert c["kind"] != "equal" or (cos > 1 - 1e-4).all(), (c["name"], cos)
            assert c["kind"] != "orthogonal" or (np.abs(cos) < 1e-6).all(), (c["name"], cos)
    # every sample of every case of the SE backward has a hidden unit on either side of the ReLU (H = 1: the two samples between them)
    for name in M.case_names("id_se_bwd"):
        inp = M.built("id_se_bwd", name)[0]
        z = M.se_given(inp["r"], inp["fc1"], inp["fc2"])[0].astype(np.float64) @ inp["fc1"].astype(np.float64).T
        assert M.se_signs_mixed(z), name
    # the chain-and-tree emulation is a sum: exact on small integers, whatever the order
    for n in (1, 255, 257, 4100):
        v = (np.arange(n) % 7).astype(np.float64)
        assert M.chain_tree32(v[None])[0] == v.sum()


def test_the_written_out_forms_the_mutants_change_are_the_references():
    """``dgrad_direct`` (a transposed convolution) and ``resample_direct`` (window matrices) without a change equal the autograd / adaptive_avg_pool2d references."""
    for name in M.case_names("lpips_conv1_dgrad"):
        inp, ref, _ = M.built("lpips_conv1_dgrad", name)
        assert np.abs(M.dgrad_direct(**inp)["gx"] - ref["gx"]).max() <= 1e-12 * max(1.0, np.abs(ref["gx"]).max()), name
    for name in M.case_names("id_resample"):
        inp, ref, _ = M.built("id_resample", name)
        assert np.abs(M.resample_direct(**inp)["out"] - ref["out"]).max() <= 1e-13, name
    for name in M.case_names("id_se_bwd"):                            # the mutants' written-out backward, unchanged, is the autograd reference
        inp, ref, _ = M.built("id_se_bwd", name)
        got = M.se_ref(mutant="none", **inp)
        assert all(np.abs(got[k] - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()) for k in ref), name


@pytest.mark.parametrize("k,s,shapes", [(3, 2, M.POOL3), (2, 2, [(h, w) for _, h, w in M.POOL2])])
def test_first_maximum_in_row_major_order_is_what_autograd_of_max_pool2d_does(k, s, shapes):
    for h, w in shapes:
        a = M.quant(f"tie{k}.{h}.{w}", (2, 3, h, w))
        ho, wo = (h - k) // s + 1, (w - k) // s + 1
        win = lambda p, i, j: a.reshape(6, h, w)[p, s * i:s * i + k, s * j:s * j + k]           # noqa: E731
        assert any((win(p, i, j) == win(p, i, j).max()).sum() > 1 for p in range(6) for i in range(ho) for j in range(wo)), "no tie in any window"
        g = M.ints(f"tieg{k}.{h}.{w}", (2, 3, ho, wo)) + np.float32(0.5)
        x = torch.from_numpy(a).double().requires_grad_()
        want = torch.autograd.grad(F.max_pool2d(x, k, s), x, torch.from_numpy(g).double())[0].numpy()
        assert np.array_equal(M.route_first_max(a, g, k, s).astype(np.float64), want), (h, w)
        assert not np.array_equal(M.route_first_max(a, g, k, s, last=True).astype(np.float64), want), (h, w)


@pytest.mark.parametrize("op,name", ALL, ids=[f"{o}-{n}" for o, n in ALL])
def test_stock_float32_and_the_kernel_tree_sit_inside_the_bar(op, name):
    _, make, ref_fn, bar_fn, stock, emulate = M.OPS[op]
    inp, ref, bar = M.built(op, name)
    for label, fn in (("stock float32", stock), ("kernel tree in float32", emulate)):
        if fn is None:
            continue
        got = fn(**inp)
        assert set(got) <= set(ref)
        r = M.ratio(got, ref, M.STOCK_BAR[op](**inp) if fn is stock and op in M.STOCK_BAR else bar)
        print(f"{op} {name}: {label} at {r:.3f} of the bar")
        assert r <= 1.0, (op, name, label, r)


@pytest.mark.parametrize("op", list(M.CASES))
def test_every_mutant_is_twice_the_bar_away_on_some_case(op):
    killed = {}
    for name in M.case_names(op):
        inp, ref, bar = M.built(op, name)
        for mname, mut in M.MUTANTS[op].items():
            r = M.ratio(mut(**inp), ref, bar)
            if r >= 2.0 and (mname not in killed or r > killed[mname][1]):
                killed[mname] = (name, r)
    for mname in M.MUTANTS[op]:
        if mname in killed:
            print(f"{op}: '{mname}' is killed by {killed[mname][0]} at {killed[mname][1]:.3g} bars")
    missing = [m for m in M.MUTANTS[op] if m not in killed]
    assert not missing, (op, missing)
