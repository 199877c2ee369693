"""The chain's same-resolution convolutions (csrc/modconv_chain.hip, ``e4s_chain_conv3x3``) keep every bit of the record in tests/golden/chain_bits.json.

The record was made by tests/golden/make_chain_bits.py on the commit BEFORE the kernel's K loop began to carry a tap's second-row activation fragments over to the
next input row and its epilogue went to packed pairs, one read of each per-channel table for both pixel rows and 16-byte split-plane stores behind a half-wave
exchange.  Every output is still the same products accumulated in the same order (chunk, tap, hi*hi / hi*lo / lo*hi), fl(fma(acc, d, noise) + bias) — the form
the compiler's contraction gave the first kernel, which kept two roundings only for accumulator registers 14 and 15 of the 32 -> 32 variant; the new epilogue
writes both forms out as instructions — leaky ReLU, gain and the next layer's modulation with their roundings, the bf16 split hi = bf16(fl(v * s)),
lo = bf16(fma(v, s, -hi)), and the same ToRGB chain (channel ascending within a lane, the two half-waves added, then skip + bias) — so SHA-256 of the hi plane,
of the lo plane, of the 16 zero bytes behind them and of the image are compared for equality.
Cases (make_chain_bits.CASES): both built variants (32 -> 32 + ToRGB, 64 -> 64 + ToRGB + split planes); 16 x 32 (one tile on all four borders), 32 x 32 and 16 x 64
(two tiles either way), 48 x 96; batch 1 - 3; noise per sample, shared and absent; skip image present and absent; activation on and off; no activation bias;
600 tiles on one launch (a workgroup walks three and reloads its per-sample tables).  The output buffers start as 0x5a5a everywhere, the tail included."""
import importlib.util
import json
import os

import pytest

from e4s2024_amd import ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ops.MODCONV_MODE != "sb", reason="these kernels are the split-arithmetic routes (E4S_MODCONV=f32 switches them off)")]

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_chain_bits", os.path.join(GOLDEN, "make_chain_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "chain_bits.json")) as f:
        return json.load(f)


def test_the_record_covers_every_case(record):
    assert sorted(record) == sorted(c[0] for c in bits.CASES)
    for c in bits.CASES:
        rec = record[c[0]]
        assert sorted(rec) == (["hi", "lo", "rgb", "tail"] if c[1] == 64 else ["rgb"]), c[0]
        assert rec.get("tail", bits.ZERO_TAIL) == bits.ZERO_TAIL, c[0]
    hashes = [v for rec in record.values() for k, v in rec.items() if k != "tail"]
    assert len(set(hashes)) == len(hashes)
    # the paths the cases are there for, per variant
    for c in (32, 64):
        cs = [x for x in bits.CASES if x[1] == c]
        assert {(x[2], x[3]) for x in cs} >= {(16, 32), (32, 32), (16, 64), (48, 96)}
        assert {x[4] for x in cs} == {1, 2, 3}
        assert {x[5] for x in cs} == {"per_sample", "shared", None}
        assert {x[6] for x in cs} == {True, False} and {x[7] for x in cs} == {True, False} and {x[8] for x in cs} == {True, False}
        assert any(x[4] >= 3 and (x[2] // 16) * (x[3] // 32) * x[4] > 2 * 256 for x in cs)
    assert all(x[2] % 16 == 0 and x[3] % 32 == 0 for x in bits.CASES)


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_output_bits_equal_the_record(record, case):
    got = bits.run_case(case)
    again = bits.run_case(case)
    print(case[0], got, again)
    assert got == again, "two runs of one library disagree"
    assert got == record[case[0]]
