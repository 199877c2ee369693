"""The half-composed up layer (csrc/modconv_uphc.hip) keeps every bit of the record in tests/golden/uphc_bits.json.

The record was made by tests/golden/make_uphc_bits.py on the commit BEFORE the persistent kernel's tile went from 16 rows x 16 columns (14 kept) to 8 rows x 32
columns (30 kept) and its epilogue lost its copies and 64-bit store addresses.  Every output is still the same products accumulated in the same order (chunk, row
parity, input row, tap, hi*hi / hi*lo / lo*hi), the same four-tap fmaf chain across the columns, fmaf(o, d, bias) + noise, leaky ReLU, gain and the next layer's
modulation with their three roundings, and the same bf16 hi / lo split — so SHA-256 of the hi plane, of the lo plane and of the 16 zero bytes behind them are compared
for equality.  Cases (make_uphc_bits.CASES): widths 14, 15, 28 - 32, 37, 60, 61; heights 7, 8, 9, 16, 17; 2 / 4 / 8 chunks; 1 - 3 channel tiles; batch 1 - 3; noise
per sample, shared and absent; activation on and off; no activation bias; the asymmetric rank-1 blur; 600 tiles on one launch (several items per workgroup); 270
and 360 tiles with 2 and 3 channel tiles each (the tiles left over after the walk's full rounds are handed out by item, one and two per workgroup).  The output
buffer starts as 0x5a5a everywhere, the tail included."""
import importlib.util
import json
import os

import pytest

from e4s2024_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (ops.UP_HC and ops.MODCONV_MODE == "sb"), reason="the half-composed route is switched off (E4S_UP_HC / E4S_MODCONV)")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_uphc_bits", os.path.join(GOLDEN, "make_uphc_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "uphc_bits.json")) as f:
        return json.load(f)


def test_the_record_covers_every_case(record):
    assert sorted(record) == sorted(c[0] for c in bits.CASES)
    for name, rec in record.items():
        assert rec["tail"] == bits.ZERO_TAIL, name
    hashes = [rec[k] for rec in record.values() for k in ("hi", "lo")]
    assert len(set(hashes)) == len(hashes)
    # the edges the cases are there for
    widths, heights = {c[4] for c in bits.CASES}, {c[3] for c in bits.CASES}
    assert {14, 15, 29, 30, 31, 32, 37, 61} <= widths and {7, 8, 9, 17} <= heights
    assert {c[1] for c in bits.CASES} >= {32, 64, 128} and {c[2] for c in bits.CASES} >= {32, 64, 96} and {c[5] for c in bits.CASES} == {1, 2, 3}
    assert {c[6] for c in bits.CASES} == {"per_sample", "shared", None} and {c[7] for c in bits.CASES} == {True, False} and {c[8] for c in bits.CASES} == {True, False}
    assert any(((c[3] + 7) // 8) * ((c[4] + 29) // 30) * c[5] > 2 * 256 for c in bits.CASES)


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_output_bits_equal_the_record(record, case):
    got = bits.run_case(case)
    again = bits.run_case(case)
    print(case[0], got, again)
    assert got == again, "two runs of one library disagree"
    assert got == record[case[0]]
