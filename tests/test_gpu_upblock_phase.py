"""The region-uniform block kernel of the masked up layers (csrc/modconv_upblock_mx.hip) keeps every bit of the record in tests/golden/upblock_phase_bits.json
at more than one 32-channel chunk.

The record was made by tests/golden/make_upblock_phase_bits.py on the commit BEFORE the kernel's staging was spread over all waves of a group, its positions were
re-mapped to lanes, its operand reads moved one MFMA group ahead and its barrier into the middle of a unit.  None of that changes a value — every accumulator still
takes chunk -> unit -> f16 (d, j) -> fp6 term in that order — so SHA-256 of the output bytes and the move of the guard counter are compared for equality.  tests/golden/mx_stage_bits.json sees this kernel at one chunk only; the cases here
(make_upblock_phase_bits.CASES) run 2, 3 and 8 chunks (the weight ring wraps, a conversion between chunks, an odd unit count), a partial tile of output channels,
two block rows on all four image borders at batch 2 with per-sample noise, pairs with one mixed block (the idle group) and with two (the early return), region-less
pixels, and ``x`` as a view into a buffer of NaNs (compared with the stand-alone run AND the record).  Every case asserts that the block kernel did run."""
import importlib.util
import json
import os

import pytest

from e4s2024_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ops.MODCONV_MODE != "sb" or ops.MX_MODE < 2, reason="the block kernel is the f16 + fp6 route of the split-arithmetic kernels")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_upblock_phase_bits", os.path.join(GOLDEN, "make_upblock_phase_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "upblock_phase_bits.json")) as f:
        return json.load(f)


def test_the_record_covers_every_case(record):
    assert sorted(record) == sorted(c[0] for c in bits.CASES)
    for c in bits.CASES:
        assert record[c[0]]["guard"] == 0 and not record[c[0]]["overflowed"], c[0]
        # a case whose layer stayed composed would test nothing
        assert record[c[0]]["blocks"] == 1 and record[c[0]]["calls"] == 1, c[0]


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_output_bits_and_guard_counter_equal_the_record(record, case):
    got = bits.run_case(case)
    print(case[0], got)
    assert got["blocks"] == 1 and got["calls"] == 1, "the layer did not take the block route"
    if case[8]:
        alone = bits.run_case(case, poison=False)
        print(case[0], "stand-alone", alone)
        assert got == alone, "what lies beside x in memory reached the output"
    assert got == record[case[0]]
