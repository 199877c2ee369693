"""The staging of the masked f16 + 2 x MX-fp6 kernels (csrc/modconv_mx_tile.h, csrc/modconv_mx4.hip, csrc/modconv_upblock_mx.hip) keeps every bit of the record
in tests/golden/mx_stage_bits.json.

The record was made by tests/golden/make_mx_stage_bits.py on the commit BEFORE the patch loads went through a buffer descriptor (an out-of-image patch pixel is a
lane whose offset lies beyond the descriptor's range: the hardware returns 0 where a select used to zero a clamped load).  That changes no value, nor may any
later change to how pixels without a region get their zero modulation, so SHA-256 of the output bytes and the move of the guard counter are compared for equality.  The cases
(make_mx_stage_bits.CASES) are the ones tests/golden/mx_bits.json cannot see: all 16 table rows in use next to region-less pixels; ``x`` as a view into a buffer
of NaNs at batch 2 (what lies beside an image must never reach the output: compared with the stand-alone run AND the record); the block kernel together with the
composed kernel on an up layer that does take the block route; the plain-convolution variant with and without instance-norm statistics."""
import importlib.util
import json
import os

import pytest

from e4s2024_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ops.MODCONV_MODE != "sb", reason="these kernels are the split-arithmetic routes (E4S_MODCONV=f32 switches them off)")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_mx_stage_bits", os.path.join(GOLDEN, "make_mx_stage_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "mx_stage_bits.json")) as f:
        return json.load(f)


def test_the_record_covers_every_case(record):
    assert sorted(record) == sorted(c[0] for c in bits.CASES)
    for c in bits.CASES:
        assert record[c[0]]["guard"] == 0 and not record[c[0]]["overflowed"], c[0]
        # a block-kernel case whose layer stayed composed would test nothing
        assert record[c[0]].get("blocks") == (1 if c[1] == "blk" else None), c[0]


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_output_bits_and_guard_counter_equal_the_record(record, case):
    got = bits.run_case(case)
    print(case[0], got)
    if case[10]:
        alone = bits.run_case(case, poison=False)
        print(case[0], "stand-alone", alone)
        assert got == alone, "what lies beside x in memory reached the output"
    assert got == record[case[0]]
