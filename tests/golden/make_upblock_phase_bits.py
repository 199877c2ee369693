"""Bit record of the region-uniform block kernel of the masked up layers (csrc/modconv_upblock_mx.hip) at MORE THAN ONE 32-channel chunk: the weight ring wraps,
chunks are converted between phases, a pair's group idles.  tests/golden/mx_stage_bits.json holds this kernel at one chunk only, so a change to its phase structure,
its counted waits or its staging split is pinned here — SHA-256 of the output bytes and the guard counter's move (``flags[1]``), as make_mx_stage_bits.py records
them.  Run once on the GPU at the commit whose bits are to be kept:

    python tests/golden/make_upblock_phase_bits.py tests/golden/upblock_phase_bits.json

``tests/test_gpu_upblock_phase.py`` imports ``CASES`` / ``run_case`` from here.  Two routes:

* ``ops``: ``ops.region_modconv3x3`` with the block route open from width 32 and both percent thresholds at 1 (block kernel + composed kernel on one output).
  That entry takes the route (and the f16 + fp6 kernels at all) from 128 output channels on, and its map kernel hands a row of four blocks over only as a whole:
  a pair of blocks is taken or left together there.
* ``direct``: ``e4s_masked_upconv_blocks_mx`` alone on a zero-filled output with a hand-made block map — the 64- and 96-channel layers (one tile, a partial
  tile), a pair with ONE mixed block (that group only keeps the barriers company) and a pair with both mixed (the workgroup returns at once).

Shapes: input 8 x 32 (one row of four blocks = two pairs) at 2 / 3 / 8 chunks (10 / 15 / 40 units), and 16 x 48 at batch 2 (two block rows, three pairs per row,
all four image borders, per-sample noise).  ``poison``: ``x`` is a view into a NaN-filled buffer (make_mx_stage_bits._place); the case runs with a stand-alone
``x`` too and the two results are equal."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from e4s2024_amd import ops  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_mx_stage_bits", os.path.join(HERE, "make_mx_stage_bits.py"))
stage = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(stage)

DEV = "cuda:0"
NREG = 12

#        name                              route    bs  cin cout  h   w   map          poison
CASES = [("ops_64to128_8x32_uni", "ops", 1, 64, 128, 8, 32, "uni", False),                    # 2 chunks, 10 units: the ring wraps, one conversion between chunks
         ("ops_96to128_8x32_uni", "ops", 1, 96, 128, 8, 32, "uni", False),                    # 3 chunks: an odd unit count
         ("ops_256to128_8x32_uni", "ops", 1, 256, 128, 8, 32, "uni", False),                  # the benchmark layer's depth, 40 units
         ("ops_64to160_8x32_uni", "ops", 1, 64, 160, 8, 32, "uni", False),                    # a partial tile of output channels
         ("ops_64to128_16x48_b2_none", "ops", 2, 64, 128, 16, 48, "none", True),              # two block rows, both edges, region-less pixels: one tile stays composed
         ("direct_64to64_8x32_uni", "direct", 1, 64, 64, 8, 32, "uni", False),
         ("direct_96to64_8x32_one_mixed", "direct", 1, 96, 64, 8, 32, "one_mixed", False),    # pair 0: its second block mixed, pair 1: its first
         ("direct_256to64_8x32_uni", "direct", 1, 256, 64, 8, 32, "uni", False),
         ("direct_64to96_8x32_both_mixed", "direct", 1, 64, 96, 8, 32, "both_mixed", False),  # pair 0 returns at once
         ("direct_64to64_16x48_b2_mixed", "direct", 2, 64, 64, 16, 48, "b2_mixed", True)]     # idle groups, early returns and full pairs on both edges


def _block_map(kind, bs, nby, nbx):
    """Region of every 16 x 16 output block (255: not region-uniform); the two blocks of a pair always differ."""
    m = ((3 * np.arange(nby)[None, :, None] + 5 * np.arange(nbx)[None, None, :] + 7 * np.arange(bs)[:, None, None] + 2) % NREG).astype(np.uint8)
    if kind == "one_mixed":
        m[:, 0, 1] = 255
        m[:, 0, 2] = 255
    elif kind == "both_mixed":
        m[:, 0, 0:2] = 255
    elif kind == "b2_mixed":
        m[0, 0, 1] = 255            # sample 0, row 0: the idle group is group 1
        m[0, 1, 4] = 255            # ... row 1, last pair: group 0
        m[1, 0, 2:4] = 255          # sample 1: a pair that returns
        m[1, 1, 0] = 255
    elif kind == "none":
        m[:, 1, 0:4] = 255          # ops route: the first tile (four blocks) of block row 1 carries region-less and mixed pixels
    return m


def _inputs(case):
    name, route, bs, cin, cout, h, w, mapk, _ = case
    rs = np.random.RandomState(sum(name.encode()) * 7 + cin)
    ho, wo = 2 * h, 2 * w
    a = {"x": rs.standard_normal((bs, cin, h, w)).astype(np.float32),
         "s": (1.0 + 0.3 * rs.standard_normal((bs, NREG, cin))).astype(np.float32),
         "wgt": rs.standard_normal((1, cout, cin, 3, 3)).astype(np.float32),
         "d": (rs.rand(bs, NREG, cout) + 0.5).astype(np.float32),
         "nz": rs.standard_normal((bs, 1, ho, wo)).astype(np.float32),          # per-sample noise
         "ab": (0.1 * rs.standard_normal(cout)).astype(np.float32)}
    bm = _block_map(mapk, bs, ho // 16, wo // 16)
    a["blocks"] = bm
    lab = np.repeat(np.repeat(bm, 16, 1), 16, 2).copy()                          # labels at the output resolution
    if mapk == "none":
        lab[:, 16:32, 0:64] = rs.randint(0, NREG, (bs, 16, 64))
        lab[:, 20:27, 3:41] = 255
    a["lab"] = lab
    return a


def run_case(case, poison=None):
    """-> {"sha256": of the output bytes, "guard": how far flags[1] moved, "overflowed": the sticky bit, "blocks": ctrl[2] (1 = the layer took the block route),
    "calls": how often the block kernel's entry point was called}.  ``poison``: None = as the case says, False = the same inputs with a stand-alone ``x``."""
    with torch.no_grad():
        return _run_case(case, case[8] if poison is None else poison)


def _run_case(case, poison):
    name, route, bs, cin, cout, h, w, mapk, _ = case
    a = _inputs(case)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)  # noqa: E731
    x, buf = stage._place(a["x"], poison)
    flags = ops.mx_flags(DEV)
    ops.mx_overflowed()
    before = int(flags[1].item())
    wgt = t(a["wgt"])
    nw = torch.tensor([0.17], device=DEV)
    blur = torch.tensor([1., 3., 3., 1.], device=DEV)
    blur = blur[:, None] * blur[None, :]
    blur = (blur / blur.sum() * 4).contiguous()
    wblk = ops.PreparedMx().get(wgt, None, False, 7)
    s, d, nz, ab = t(a["s"]), t(a["d"]), t(a["nz"]), t(a["ab"])
    names = []
    lib = ops.lib()
    orig = lib.call

    def call(fn, *args):
        names.append(fn)
        return orig(fn, *args)
    lib.call = call
    try:
        if route == "direct":
            out = torch.zeros((bs, cout, 2 * h, 2 * w), dtype=torch.float32, device=DEV)
            blocks = t(a["blocks"])
            ctrl = torch.tensor([0, 0, 1, 0], dtype=torch.int32, device=DEV)
            lib.call("e4s_masked_upconv_blocks_mx", ops._p(out), ops._p(x), ops._p(wblk), ops._p(flags), ops._p(s), ops._p(d), ops._p(blocks), ops._p(ctrl), ops._p(blur),
                     ops._p(nz), bs, ops._p(nw), ops._p(ab), 1, bs, cin, cout, h, w, NREG, ops._stream())
            took = int(ctrl[2].item())
        else:
            wt, _ = ops.PreparedWeights().get(wgt, blur, True, True)
            wmx = ops.PreparedMx().get(wgt, blur, True, 1)
            keep = (ops.SPLITK_MAX_OUT_FLOATS, ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT, ops.UP_BLOCKS_MIN_PERCENT_SMALL)
            try:
                ops.SPLITK_MAX_OUT_FLOATS = 0
                ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT, ops.UP_BLOCKS_MIN_PERCENT_SMALL = True, 32, 1, 1
                out = ops.region_modconv3x3(x, wt, s, d, t(a["lab"]), nz, nw, ab, True, cout, True, mx=(wmx, 1), up_blocks=(wblk, blur))
            finally:
                ops.SPLITK_MAX_OUT_FLOATS, ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT, ops.UP_BLOCKS_MIN_PERCENT_SMALL = keep
            took = int(ops._ctx().up_ctrl[2].item())
    finally:
        lib.call = orig
    torch.cuda.synchronize()
    if buf is not None:      # the kernels wrote nothing into the input's surroundings
        assert bool(torch.isnan(buf[:stage.PAD]).all()) and bool(torch.isnan(buf[-stage.PAD:]).all())
    assert bool(torch.isfinite(out).all()), name
    return {"sha256": stage.base._sha(out), "guard": int(flags[1].item()) - before, "overflowed": bool(ops.mx_overflowed()), "blocks": took,
            "calls": names.count("e4s_masked_upconv_blocks_mx")}


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "upblock_phase_bits.json")
    rec = {}
    for case in CASES:
        rec[case[0]] = run_case(case)
        again = run_case(case)
        assert again == rec[case[0]], f"{case[0]}: two runs of one library disagree: {rec[case[0]]} / {again}"
        assert rec[case[0]]["blocks"] == 1 and rec[case[0]]["calls"] == 1, f"{case[0]}: the layer did not take the block route: {rec[case[0]]}"
        if case[8]:
            alone = run_case(case, poison=False)
            assert alone == rec[case[0]], f"{case[0]}: the input's surroundings reach the output: {rec[case[0]]} / stand-alone {alone}"
        print(case[0], rec[case[0]], flush=True)
    with open(dst, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
