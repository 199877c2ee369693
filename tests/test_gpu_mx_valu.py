"""The masked f16 + 2 x MX-fp6 kernels (csrc/modconv_mx_tile.h, csrc/modconv_mx4.hip) keep every bit of the record in tests/golden/mx_bits.json.

The record was made by tests/golden/make_mx_bits.py on the commit BEFORE the K loop's operand preparation was rewritten for fewer vector-ALU instructions (packed
multiplies, one three-operand maximum per pair, fp6 operands read straight into their tuples): that rewrite changes no value — a = x * s in fp32, a1 = f16(a) RNE,
the mix-fma residual, the block exponent from the fp32 maximum, the overflow threshold 65520 and the MFMA order are what they were — so SHA-256 of the output bytes
and the move of the guard counter (``flags[1]``) are compared for equality, not within a tolerance.  Cases (make_mx_bits.CASES): same-resolution layers with ragged
tiles in both directions and two / three chunks, the fused-ToRGB + split-plane variant, a composed up layer, the four-parity kernel on maps where all / some / no
tiles qualify; region maps of 12 i.i.d. regions, with region-less (255) pixels, and of one region; and inputs whose products x * s sit on 65504, just below
65520, exactly 65520, on values f16 rounds across a power of two, and in all-zero patches."""
import importlib.util
import json
import os

import pytest

from e4s2024_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ops.MODCONV_MODE != "sb", reason="these kernels are the split-arithmetic routes (E4S_MODCONV=f32 switches them off)")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_mx_bits", os.path.join(GOLDEN, "make_mx_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "mx_bits.json")) as f:
        return json.load(f)


def test_the_record_covers_every_case(record):
    assert sorted(record) == sorted(c[0] for c in bits.CASES)
    # the overflow cases moved the guard counter when the record was made, no other case did: the planted values reach the kernels
    for c in bits.CASES:
        assert (record[c[0]]["guard"] > 0) == (c[8] == "overflow"), c[0]
        assert record[c[0]]["overflowed"] == (c[8] == "overflow"), c[0]


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_output_bits_and_guard_counter_equal_the_record(record, case):
    got = bits.run_case(case)
    print(case[0], got)
    assert got == record[case[0]]
