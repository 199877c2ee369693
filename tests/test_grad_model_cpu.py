"""The bars of tests/test_gpu_grad_kernels.py separate right from wrong before any kernel runs: on the CPU model of the synthesis path's gradient kernels
(tests/grad_model.py) stock float32 sits inside the bar of every case, the float32 emulation of a kernel's own order inside half of it, the split-bf16 emulation
inside its class bar of float64, and every mutant of an operation outside the bar of at least one case of that operation's table (the margin is printed).
The written-out forms the mutants change are held against the autograd references, and the mirror of the split-K rule against the numbers in the sources."""
import os
import re

import numpy as np
import pytest

import grad_model as M

ALL = [(op, name) for op in M.CASES for name in M.case_names(op)]
SPLIT = [(op, name) for op in M.SPLIT_OPS for name in M.case_names(op)]


def test_case_tables_hold_the_depths_read_from_the_code():
    assert M.depth("scale", chunk_px=256, px=323) == 1 + 10 and M.depth("scale", chunk_px=8192, px=323) == 2 + 10 and M.depth("scale", chunk_px=8192, px=1 << 20) == 32 + 10
    assert M.depth("fold_dx", up=2, ks=3) == 36 and M.depth("fold_ds", up=2, ks=3, chunk_px=1024, px=4096) == 9 + 16 + 10
    assert M.depth("mfma", K=1056, ksplit=8) == 3 * 66 + 8 and M.depth("linear", n=260, vec=True) == 8 + 7 and M.depth("linear", n=30, vec=False) == 1 + 7
    assert M.depth("lin_dx", out=13, osplit=32) == 1 + 32 + 2 and M.depth("tables", cout=300, gd=True, n=5) == 310 + 2 + 5
    for op in M.CASES:
        assert len(set(M.case_names(op))) == len(M.CASES[op]), op
        assert set(M.MUTANTS[op]), op
        for name in M.case_names(op):
            M.built(op, name)                                        # (the builders assert D == depth(...))
    # the wave order is a sum: exact on small integers
    for n in (1, 255, 257, 1292):
        v = (np.arange(n) % 7).astype(np.float32)
        assert M.wave_tree32(v[None])[0] == v.sum()
    # the routes the fold cases name are the ones the launch rule gives, and each kernel has a case
    assert {M.fold_route(c) for c in M.CASES["mconv_fold"]} == {"mconv_fold4_kernel", "mconv_fold_kernel<3>", "mconv_fold_kernel<1>"}


def test_the_split_k_rule_of_the_model_is_the_one_in_both_sources():
    """``ksplit_rule`` against the ``while`` of e4s_gemm_sb / e4s_mconv_wgrad and the loops of ops_grad.gemm_sb / mconv_wgrad, by the numbers in them; the ``ksplit``
    a case states is what the rule gives."""
    want = (512, 4, 1024)
    for path, anchor in (("e4s2024_amd/csrc/gemm_sb.hip", 'extern "C" int e4s_gemm_sb'), ("e4s2024_amd/csrc/gemm_sb.hip", 'extern "C" int e4s_mconv_wgrad'),
                         ("e4s2024_amd/ops_grad.py", "def gemm_sb("), ("e4s2024_amd/ops_grad.py", "def mconv_wgrad(")):
        assert M.split_numbers(path, anchor) == want, (path, anchor)
    # the Python loops stop at ops.GEMM_SPLITK_CAP_FLOATS of partial products as well; the workspace they then hand over stops the C loop at the same split
    shift = re.search(r"^GEMM_SPLITK_CAP_FLOATS\s*=\s*(\d+)\s*<<\s*(\d+)", open(os.path.join(M.ROOT, "e4s2024_amd/ops.py")).read(), re.M)
    cap = int(shift.group(1)) << int(shift.group(2))
    assert cap == 64 << 20
    for c in M.CASES["gemm_sb"]:
        tiles, nchunk = M.gemm_tiles(c["M"], c["N"], c["a_kc"], c["b_kc"]), M.cdiv(c["K"], 32)
        py = M.ksplit_rule(tiles, nchunk, c["batch"], c["M"], c["N"], cap if c["ws"] else 0)
        assert py == c["ksplit"] == M.ksplit_rule(tiles, nchunk, c["batch"], c["M"], c["N"], py * c["batch"] * c["M"] * c["N"] if py > 1 else 0), c["name"]
    for c in M.CASES["mconv_wgrad"]:
        n, batch = c["cin"] * c["ks"] ** 2, c["up"] ** 2 * c["bs"]
        py = M.ksplit_rule(M.cdiv(c["cout"], 128) * M.cdiv(n, 128), M.cdiv(c["h"] * c["w"], 32), batch, c["cout"], n, cap)          # ops_grad counts 128-row tiles
        assert py == c["ksplit"] == M.ksplit_rule(M.wgrad_tiles(c["cout"], n), M.cdiv(c["h"] * c["w"], 32), batch, c["cout"], n, max(1, py * batch * c["cout"] * n)), c["name"]
    by_note = {c["name"]: c["ksplit"] for c in M.CASES["gemm_sb"]}
    assert by_note["kc_kc.128x128x1056.b1.emptyslice"] == 8 and by_note["kc_kc.128x128x1056.b1.nows"] == 1 and by_note["kc_kc.128x128x4100.b1.wide"] == 32 and by_note["kc_kc.128x128x4064.b1.wide16"] == 16
    assert by_note["kc_kc.3x288x4096.b2.skinny.split"] == 32 and by_note["kc_kc.8x257x64.b2.skinny"] == 1 and by_note["kc_kc.9x257x64.b2.notskinny"] == 1
    # K = 1056: 33 chunks in 8 slices of 5: the last slice starts past the end; K = 4100: 129 chunks in 32 slices of 5: the last six do (128 <= 129 admits the
    # doubling to 32); K = 4064: 127 chunks in 16 slices of 8, none empty.  All three sum at least 16 slices of at most 65536 outputs: the wide finalize kernel
    assert 7 * M.cdiv(33, 8) >= 33 and 26 * M.cdiv(129, 32) >= 129 and 15 * M.cdiv(127, 16) < 127
    wg = {c["name"]: c["ksplit"] for c in M.CASES["mconv_wgrad"]}
    assert wg["k3.cin20.cout40.16x16.up1.r16.masked.b1.all16.split"] == 2 and wg["k3.cin20.cout40.33x16.up1.r5.masked.b1.stray.tail16.split"] == 4


def test_the_written_out_forms_the_mutants_change_are_the_references():
    for name in M.case_names("mconv_fold"):
        inp, ref, _ = M.built("mconv_fold", name)
        got = M.fold_direct(**inp)
        assert set(got) == set(ref) and all(np.abs(got[k] - ref[k]).max() <= 1e-12 * max(1.0, np.abs(ref[k]).max()) for k in ref), name
    for name in M.case_names("style_tables_bwd"):                      # (the written-out form starts from s, d, wsq rounded to float32, as the kernel does)
        inp, ref, bar = M.built("style_tables_bwd", name)
        got = M.tables_direct(**inp)
        assert set(got) == set(ref) and M.ratio(got, ref, bar) <= 0.25, name


@pytest.mark.parametrize("op,name", ALL, ids=[f"{o}-{n}" for o, n in ALL])
def test_stock_float32_sits_inside_the_bar_and_the_kernel_order_inside_half_of_it(op, name):
    _, make, ref_fn, bar_fn, stock, emulate32 = M.OPS[op]
    inp, ref, bar = M.built(op, name)
    for label, fn, lim in (("stock float32", stock, 1.0), ("kernel order in float32", emulate32, 0.5)):
        if fn is None:
            continue
        got = fn(**inp)
        assert set(got) <= set(ref)
        r = M.ratio(got, ref, bar)
        print(f"{op} {name}: {label} at {r:.3f} of the bar")
        assert r <= lim, (op, name, label, r)


@pytest.mark.parametrize("op,name", SPLIT, ids=[f"{o}-{n}" for o, n in SPLIT])
def test_the_split_emulation_sits_inside_its_class_bar_and_the_outer_bar(op, name):
    inp, ref, bar = M.built(op, name)
    emu, cbar = M.built_class(op, name)
    emu32 = M.OPS[op][5]
    for k in emu:
        e = np.abs(M.descaled(emu[k], inp) - M.descaled(ref[k], inp)).max()
        scale = np.abs(M.descaled(ref[k], inp)).max()
        print(f"{op} {name} {k}: emulation at {e / cbar[k]:.3f} of the class bar {cbar[k]:.3e}; the class bar is {cbar[k] / (M.OUTER * scale):.2f} of the outer bar")
        assert e <= cbar[k] and M.ratio({k: emu[k]}, ref, bar) <= 1.0, (op, name, k)
        if emu32 is not None:
            e32 = np.abs(M.descaled(emu32(**inp)[k].astype(np.float64), inp) - M.descaled(emu[k], inp)).max()
            print(f"{op} {name} {k}: float32 accumulation at {e32 / cbar[k]:.3f} of the class bar")
            assert e32 <= 0.5 * cbar[k], (op, name, k)


@pytest.mark.parametrize("op", list(M.CASES))
def test_every_mutant_is_outside_the_bar_of_some_case(op):
    """A mutant is killed by the element-wise bar against float64 or, on the split-bf16 operations, by the class bar against the emulation."""
    killed = {}
    for name in M.case_names(op):
        inp, ref, bar = M.built(op, name)
        for mname, mut in M.MUTANTS[op].items():
            got = mut(**inp)
            r = M.ratio(got, ref, bar)
            if op in M.SPLIT_OPS:
                emu, cbar = M.built_class(op, name)
                r = max(r, max(np.abs(M.descaled(got[k], inp) - M.descaled(emu[k], inp)).max() / cbar[k] for k in got))
            if r > 1.0 and (mname not in killed or r > killed[mname][1]):
                killed[mname] = (name, r)
    for mname in M.MUTANTS[op]:
        if mname in killed:
            print(f"{op}: '{mname}' is killed by {killed[mname][0]} at {killed[mname][1]:.3g} bars")
    missing = [m for m in M.MUTANTS[op] if m not in killed]
    assert not missing, (op, missing)
