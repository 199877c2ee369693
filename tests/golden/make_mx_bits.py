"""Bit record of the masked f16 + 2 x MX-fp6 kernels (csrc/modconv_mx_tile.h, csrc/modconv_mx4.hip): SHA-256 of the output bytes and the guard counter's
move (``flags[1]``) of seeded layers through ``ops.region_modconv3x3``.  Run once on the GPU at the commit whose bits are to be kept:

    python tests/golden/make_mx_bits.py tests/golden/mx_bits.json

``tests/test_gpu_mx_valu.py`` imports ``CASES`` / ``run_case`` from here and asserts the same hashes: a change to the K loop's operand preparation that is
meant to leave every value alone (fewer instructions, not other arithmetic) must reproduce them.

Inputs are made on the CPU (numpy ``RandomState`` — the same bytes everywhere) and copied to the device.  Region maps: 12 regions i.i.d. per pixel, the same
with a block of label 255 (no region), one region everywhere, and for the up layers cells of 8 output pixels (every tile of the four-parity kernel qualifies)
and a half-shifted map with a region-less corner (some tiles qualify).  ``edge`` plants products x * s on the values where the range logic can go wrong."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from e4s2024_amd import ops  # noqa: E402

DEV = "cuda:0"
NREG = 12

# Products planted by ``edge``: the largest finite f16, the last fp32 below the overflow threshold, values f16 rounds ACROSS a power of two (the fp32 exponent of
# |a| and the f16 exponent of a1 differ: the scale must come from the fp32 value) and their neighbours on the other side.
_BELOW = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))
EDGE_FINITE = [65504.0, _BELOW] + [s * 2.0 ** k * (1.0 + e) for k in (-14, -3, 0, 5, 10, 15) for e in (-2.0 ** -12, -2.0 ** -13, 2.0 ** -12) for s in (1.0, -1.0)]
EDGE_OVERFLOW = [65520.0, -65520.0]

#        name                 kind    bs cin cout  h   w   labels     edge
CASES = [("same_32to128_40x24", "same", 2, 32, 128, 24, 40, "iid", None),            # ragged tiles in both directions, two chunks
         ("same_32to128_40x24_none", "same", 2, 32, 128, 24, 40, "iid255", None),
         ("same_32to128_40x24_one", "same", 2, 32, 128, 24, 40, "single", None),
         ("same_48to128_40x24", "same", 2, 48, 128, 24, 40, "iid255", None),         # three chunks: the two-slot patch buffer wraps
         ("same_32to128_edge", "same", 2, 32, 128, 24, 40, "iid255", "finite"),
         ("same_32to128_edge_ovf", "same", 2, 32, 128, 24, 40, "iid", "overflow"),
         ("rgb_sp_16to128_32x16", "rgb", 2, 16, 128, 16, 32, "iid255", None),        # fused ToRGB + split-plane hand-over
         ("rgb_sp_16to128_edge", "rgb", 2, 16, 128, 16, 32, "iid", "finite"),
         ("up_32to128_32x16", "up", 2, 32, 128, 16, 32, "iid255", None),             # composed up layer
         ("up_32to128_one", "up", 2, 32, 128, 16, 32, "single", None),
         ("up_32to128_edge", "up", 2, 32, 128, 16, 32, "iid", "finite"),
         ("up_32to128_edge_ovf", "up", 2, 32, 128, 16, 32, "iid255", "overflow"),
         ("mx4_32to384_cells8", "mx4", 3, 32, 384, 8, 32, "cells8", None),           # four-parity kernel: every tile qualifies
         ("mx4_32to384_mixed", "mx4", 3, 32, 384, 8, 32, "mixed", None),             # ... some do
         ("mx4_32to384_iid", "mx4", 3, 32, 384, 8, 32, "iid", None),                 # ... none does
         ("mx4_32to384_one", "mx4", 3, 32, 384, 8, 32, "single", None),
         ("mx4_48to128_ragged", "mx4", 1, 48, 128, 20, 40, "cells8", None),          # partial tiles
         ("mx4_32to384_edge", "mx4", 3, 32, 384, 8, 32, "mixed", "finite"),
         ("mx4_32to384_edge_ovf", "mx4", 3, 32, 384, 8, 32, "cells8", "overflow")]


def _labels(kind, rs, bs, ho, wo):
    if kind == "single":
        return np.zeros((bs, ho, wo), np.uint8)
    if kind in ("iid", "iid255"):
        lab = rs.randint(0, NREG, (bs, ho, wo)).astype(np.uint8)
        if kind == "iid255":
            lab[:, 3: 3 + ho // 3, 5: 5 + wo // 3] = 255
        return lab
    cell = 8
    gy, gx = -(-ho // cell), -(-wo // cell)
    lab = np.repeat(np.repeat(rs.randint(0, NREG, (bs, gy, gx)), cell, 1), cell, 2)[:, :ho, :wo].astype(np.uint8)
    if kind == "mixed":                                         # right half: borders on odd output columns; a region-less corner
        lab[:, :, wo // 2:] = np.roll(lab, 1, axis=2)[:, :, wo // 2:]
        lab[:, : ho // 4, : wo // 4] = 255
    return lab


def _inputs(case):
    name, kind, bs, cin, cout, h, w, labk, edge = case
    rs = np.random.RandomState(sum(name.encode()) * 7 + cin)
    up = kind in ("up", "mx4")
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    x = rs.standard_normal((bs, cin, h, w)).astype(np.float32)
    s = (1.0 + 0.3 * rs.standard_normal((bs, NREG, cin))).astype(np.float32)
    if edge:
        # channel c carries modulation 2^(c % 5 - 2) in every region (exact products); the planted x = value / s then gives x * s == value exactly.
        # An 11 x 11 block of all-zero pixels: the lanes inside it see amax = 0 (clamped scale) in every row.
        s[:] = (2.0 ** ((np.arange(cin) % 5) - 2)).astype(np.float32)[None, None, :]
        x[:, :, 2:13, 14:25] = 0.0
        vals = EDGE_FINITE + (EDGE_OVERFLOW if edge == "overflow" else [])
        for i, v in enumerate(vals):
            for rep in range(3):
                b, c = (i + rep) % bs, (5 * i + 3 * rep) % cin
                y, xx = (7 * i + 11 * rep) % h, (3 * i + 13 * rep + 1) % w
                x[b, c, y, xx] = np.float32(v) / s[b, 0, c]
                assert np.float32(x[b, c, y, xx]) * s[b, 0, c] == np.float32(v)
    wgt = rs.standard_normal((1, cout, cin, 3, 3)).astype(np.float32)
    d = (rs.rand(bs, NREG, cout) + 0.5).astype(np.float32)
    nz = rs.standard_normal((bs, 1, ho, wo)).astype(np.float32)
    ab = (0.1 * rs.standard_normal(cout)).astype(np.float32)
    lab = _labels(labk, rs, bs, ho, wo)
    extra = {}
    if kind == "rgb":
        extra = {"w_rgb": rs.standard_normal((1, 3, cout, 1, 1)).astype(np.float32), "s_rgb": (1.0 + 0.3 * rs.standard_normal((bs, 1, cout))).astype(np.float32),
                 "b_rgb": (0.1 * rs.standard_normal((1, 3, 1, 1))).astype(np.float32), "s_next": (1.0 + 0.3 * rs.standard_normal((bs, 1, cout))).astype(np.float32)}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return t(x), t(wgt), t(s), t(d), t(nz), t(ab), t(lab), {k: t(v) for k, v in extra.items()}


def _sha(*tensors):
    hsh = hashlib.sha256()
    for o in tensors:
        hsh.update(o.detach().contiguous().cpu().numpy().tobytes())
    return hsh.hexdigest()


def run_case(case):
    """-> {"sha256": of the output bytes, "guard": how far flags[1] moved, "overflowed": the sticky bit}."""
    with torch.no_grad():
        return _run_case(case)


def _run_case(case):
    name, kind, bs, cin, cout, h, w, labk, edge = case
    x, wgt, s, d, nz, ab, lab, extra = _inputs(case)
    up = kind in ("up", "mx4")
    nw = torch.tensor([0.17], device=DEV)
    blur = torch.tensor([1., 3., 3., 1.], device=DEV)
    blur = blur[:, None] * blur[None, :]
    blur = blur / blur.sum() * 4
    wt, _ = ops.PreparedWeights().get(wgt, blur if up else None, up, True)
    wmx = ops.PreparedMx().get(wgt, blur if up else None, up, 1)
    kw = {}
    if kind == "mx4":
        kw["mx4"] = ops.PreparedMx().get(wgt, blur, True, 4)
    if kind == "rgb":
        r_wt, _ = ops.PreparedWeights().get(extra["w_rgb"], None, False, False)
        kw["rgb"] = (r_wt, extra["s_rgb"], extra["b_rgb"], None, None)
        kw["s_next"] = extra["s_next"]
    flags = ops.mx_flags(DEV)
    ops.mx_overflowed()
    before = int(flags[1].item())
    keep = ops.SPLITK_MAX_OUT_FLOATS
    try:
        ops.SPLITK_MAX_OUT_FLOATS = 0                # (no split-K on these small layers: one workgroup per tile runs the whole K loop)
        out = ops.region_modconv3x3(x, wt, s, d, lab, nz, nw, ab, True, cout, up, mx=(wmx, 1), **kw)
    finally:
        ops.SPLITK_MAX_OUT_FLOATS = keep
    torch.cuda.synchronize()
    outs = out if isinstance(out, tuple) else (out,)
    guard = int(flags[1].item()) - before
    return {"sha256": _sha(*outs), "guard": guard, "overflowed": bool(ops.mx_overflowed())}


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "mx_bits.json")
    rec = {}
    for case in CASES:
        rec[case[0]] = run_case(case)
        again = run_case(case)
        assert again == rec[case[0]], f"{case[0]}: two runs of one library disagree: {rec[case[0]]} / {again}"
        print(case[0], rec[case[0]], flush=True)
    with open(dst, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
