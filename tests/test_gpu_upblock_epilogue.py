"""The epilogue of the region-uniform block kernel of the masked up layers (csrc/modconv_upblock_mx.hip) keeps every bit of the record in
tests/golden/upblock_epilogue_bits.json on the branches the other records of this kernel do not reach.

The record was made by tests/golden/make_upblock_epilogue_bits.py on the commit BEFORE the epilogue gave a thread four adjacent outputs of one channel (two 16-byte
LDS reads per pre-blur row, one 16-byte store per output row, a re-pitched pre-blur tile, the blur taps through LDS).  Every output is still one fmaf chain from 0
over its 16 taps in row-major order, then fmaf(a, d, bias) + noise, then the leaky ReLU and the gain — so SHA-256 of the output bytes and the move of the guard
counter are compared for equality.  Cases (make_upblock_epilogue_bits.CASES, all at cin = 32 = one chunk, the entry point called directly): act = 0; no noise;
one noise plane shared by a batch of 2; no activation bias; no demodulation; cout = 72 (a tile of 8 channels: half of one 16-channel pass) and 16; two block rows
on both image borders at batch 2 with an idle group per sample; the output as a view 4, 8 and 12 bytes past a 16-byte boundary inside a buffer of NaNs (the
four-byte store path: equal to the aligned run byte for byte, compared directly and through the record; the NaNs on both sides intact).  Every case runs twice and
asserts that the block kernel's entry point was called once."""
import importlib.util
import json
import os

import numpy as np
import pytest

from e4s2024_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ops.MODCONV_MODE != "sb" or ops.MX_MODE < 2, reason="the block kernel is the f16 + fp6 route of the split-arithmetic kernels")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_upblock_epilogue_bits", os.path.join(GOLDEN, "make_upblock_epilogue_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)
BY_NAME = {c[0]: c for c in bits.CASES}


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "upblock_epilogue_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def aligned_runs():
    """name of an aligned case -> its output bytes on this library (computed once, shared by the three misaligned cases)."""
    return {al: bits.run_case_bytes(BY_NAME[al])[1] for al in sorted(set(bits.ALIGNED_OF.values()))}


def test_the_record_covers_every_case(record):
    assert sorted(record) == sorted(c[0] for c in bits.CASES)
    for c in bits.CASES:
        assert record[c[0]]["guard"] == 0 and not record[c[0]]["overflowed"] and record[c[0]]["calls"] == 1, c[0]
    for name, al in bits.ALIGNED_OF.items():
        assert record[name] == record[al], name
    # the cases differ from one another where it matters: no two of the other records are equal
    rest = [record[c[0]]["sha256"] for c in bits.CASES if c[0] not in bits.ALIGNED_OF]
    assert len(set(rest)) == len(rest)


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_output_bits_and_guard_counter_equal_the_record(record, aligned_runs, case):
    got, out = bits.run_case_bytes(case)
    again = bits.run_case(case)
    print(case[0], got, again)
    assert got == again, "two runs of one library disagree"
    assert got["calls"] == 1, "the block kernel's entry point was not called once"
    if case[0] in bits.ALIGNED_OF:          # (run_case has checked the NaNs on both sides of the output)
        assert np.array_equal(out.view(np.uint32), aligned_runs[bits.ALIGNED_OF[case[0]]].view(np.uint32)), "a misaligned output changes the result"
    assert got == record[case[0]]
