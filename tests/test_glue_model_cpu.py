"""The bars of tests/test_gpu_glue.py separate right from wrong before any kernel runs: on the CPU model of the glue kernels (tests/glue_model.py) stock
float32 PyTorch and the float32 emulation of every kernel's own summation tree sit inside the bar of every case, and every mutant of an operation sits at
least twice the bar outside it on at least one case of that operation's table.  Prints which case kills which mutant."""
import numpy as np
import pytest

import glue_model as M

ALL = [(op, name) for op in M.CASES for name in M.case_names(op)]


def _triple(op, name, got=None):
    """(inputs, reference, bar) of a case; plane_stats in the 'nmean' mode refers to the (mean, rstd) that came with the nmean under test."""
    inp, ref, bar = M.built(op, name)
    if op == "plane_stats" and inp["mode"] == "nmean" and got is not None:
        return M.with_emitted(inp, got)
    return inp, ref, bar


def test_case_tables_hold_the_depths_read_from_the_code():
    assert M.depth("block", 1020) == 1 + 2 + 6 + 3 + 1 and M.depth("block", 1028) == 2 + 2 + 6 + 3 + 1 and M.depth("block", 49) == 1 + 6 + 3 + 1
    assert M.depth("wave", 1024) == 4 + 2 + 6 + 1 and M.depth("big", 65536) == 16 + 2 + 6 + 16 + 1 and M.depth("dot", 130) == 3 + 1 + 6
    for op in M.CASES:
        assert len(set(M.case_names(op))) == len(M.CASES[op])
        for name in M.case_names(op):
            M.built(op, name)                                        # (the builders assert D == depth(kind, size))
    # the tree emulation is a sum: exact on small integers, whatever the order
    for kind in ("block", "wave", "big"):
        for n in (4, 49, 1020, 1028, 4100):
            v = (np.arange(n) % 7).astype(np.float32)
            assert M.tree_sum32(v, kind) == v.sum(dtype=np.float64)


@pytest.mark.parametrize("op,name", ALL, ids=[f"{o}-{n}" for o, n in ALL])
def test_stock_float32_and_the_kernel_tree_sit_inside_the_bar(op, name):
    _, make, ref_fn, bar_fn, stock, emulate = M.OPS[op]
    inp = M.built(op, name)[0]
    call = {k: v for k, v in inp.items() if k not in ("D", "D2", "emitted", "exact")}
    for label, fn in (("stock float32", stock), ("kernel tree in float32", emulate)):
        if fn is None:
            continue
        got = fn(**call)
        _, ref, bar = _triple(op, name, got)
        r = M.ratio(got, ref, bar)
        print(f"{op} {name}: {label} at {r:.3f} of the bar")
        assert r <= 1.0, (op, name, label, r)


@pytest.mark.parametrize("op", list(M.CASES))
def test_every_mutant_is_twice_the_bar_away_on_some_case(op):
    emulate = M.OPS[op][5]
    killed = {}
    for name in M.case_names(op):
        inp, ref, bar = M.built(op, name)
        if op == "plane_stats" and inp["mode"] == "nmean":
            # nmean is defined by the float32 (mean, rstd) emitted with it: the kernel tree's here
            inp, ref, bar = M.with_emitted(inp, emulate(**{k: v for k, v in inp.items() if k not in ("D", "emitted")}))
        for mname, mut in M.MUTANTS[op].items():
            r = M.ratio(mut(**inp), ref, bar)
            if r >= 2.0 and (mname not in killed or r > killed[mname][1]):
                killed[mname] = (name, r)
    for mname in M.MUTANTS[op]:
        if mname in killed:
            print(f"{op}: '{mname}' is killed by {killed[mname][0]} at {killed[mname][1]:.3g} bars")
    missing = [m for m in M.MUTANTS[op] if m not in killed]
    assert not missing, (op, missing)
