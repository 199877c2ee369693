"""Bit record of what the STAGING of the masked f16 + 2 x MX-fp6 kernels decides (csrc/modconv_mx_tile.h, csrc/modconv_mx4.hip, csrc/modconv_upblock_mx.hip): which
patch pixels are zero, which modulation row a pixel takes — SHA-256 of the output bytes and the guard counter's move (``flags[1]``), as make_mx_bits.py records them
for the K loop's arithmetic.  Run once on the GPU at the commit whose bits are to be kept:

    python tests/golden/make_mx_stage_bits.py tests/golden/mx_stage_bits.json

``tests/test_gpu_mx_stage.py`` imports ``CASES`` / ``run_case`` from here.  What the cases add to make_mx_bits.CASES:

* ``nreg16``: all 16 rows of the modulation table are in use and a block of pixels has no region — "no region" must not alias a real row;
* ``poison``: ``x`` is a view into the middle of a larger buffer filled with NaN and the batch is 2, so an out-of-image patch pixel of sample 0 lies next to sample
  1's data and one of sample 1 next to the NaNs: a staging that reads them instead of zeros changes the hash (or fills the output with NaN).  Every such case is
  run with a stand-alone ``x`` too: the two hashes are equal;
* ``blk``: an up layer 32 -> 128 at 128 x 128 through the region-uniform block kernel and the composed kernel together (label cells of 32 output pixels, one cell
  row shifted by 8 so that its blocks do not qualify, uniform blocks on all four image borders; with a region-less corner, with the poisoned buffer, with
  make_mx_bits' finite edge values).  ``blocks`` in the record is the control word ``ctrl[2]``: 1 = the layer did take the block route;
* ``enc``: the plain-convolution variant (``e4s_conv3x3_mx``, with and without instance-norm statistics) on a ragged map in the poisoned buffer."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from e4s2024_amd import ops, ops_encode  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_mx_bits", os.path.join(HERE, "make_mx_bits.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

DEV = "cuda:0"
PAD = 4100          # floats of NaN on either side of a poisoned x (16-byte aligned, not page aligned)

#        name                       kind   bs cin cout   h    w  labels      edge      nreg  poison
CASES = [("same_32to128_nreg16", "same", 2, 32, 128, 24, 40, "iid255", None, 16, False),
         ("same_32to128_poison", "same", 2, 32, 128, 24, 40, "iid255", None, 12, True),
         ("rgb_sp_16to128_poison", "rgb", 2, 16, 128, 16, 32, "iid255", None, 12, True),
         ("up_32to128_poison", "up", 2, 32, 128, 16, 32, "iid255", None, 12, True),
         ("mx4_48to128_ragged_poison", "mx4", 2, 48, 128, 20, 40, "cells8", None, 12, True),
         ("blk_32to128_cells32", "blk", 1, 32, 128, 128, 128, "cells32", None, 12, False),
         ("blk_32to128_cells32_none", "blk", 1, 32, 128, 128, 128, "cells32none", None, 12, False),
         ("blk_32to128_cells32_poison", "blk", 1, 32, 128, 128, 128, "cells32none", None, 12, True),
         ("blk_32to128_cells32_edge", "blk", 1, 32, 128, 128, 128, "cells32", "finite", 12, False),
         ("enc_32to128_poison", "enc", 2, 32, 128, 24, 40, None, None, 1, True),
         ("enc_norm_32to128_poison", "encnorm", 2, 32, 128, 24, 40, None, None, 1, True)]


def _labels(kind, rs, bs, ho, wo, nreg):
    if kind in ("iid", "iid255"):
        lab = rs.randint(0, nreg, (bs, ho, wo)).astype(np.uint8)
        if kind == "iid255":
            lab[:, 3: 3 + ho // 3, 5: 5 + wo // 3] = 255
        return lab
    if kind == "cells8":
        cell = 8
        gy, gx = -(-ho // cell), -(-wo // cell)
        return np.repeat(np.repeat(rs.randint(0, nreg, (bs, gy, gx)), cell, 1), cell, 2)[:, :ho, :wo].astype(np.uint8)
    # cells of 32 output pixels, horizontal neighbours always differ; cell row 3 shifted by 8 (its 16 x 16 blocks straddle two cells: they stay composed)
    cell = 32
    gy, gx = ho // cell, wo // cell
    cells = (rs.randint(0, nreg) + 3 * np.arange(gy)[None, :, None] + 5 * np.arange(gx)[None, None, :] + np.arange(bs)[:, None, None]) % nreg
    lab = np.repeat(np.repeat(cells, cell, 1), cell, 2).astype(np.uint8)
    lab[:, 3 * cell: 4 * cell] = np.roll(lab[:, 3 * cell: 4 * cell], 8, axis=2)
    if kind == "cells32none":
        lab[:, :cell, : 2 * cell] = 255
    return lab


def _inputs(case):
    name, kind, bs, cin, cout, h, w, labk, edge, nreg, _ = case
    rs = np.random.RandomState(sum(name.replace("_poison", "").encode()) * 7 + cin)      # (a poisoned case and its stand-alone twin: the same numbers)
    up = kind in ("up", "mx4", "blk")
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    x = rs.standard_normal((bs, cin, h, w)).astype(np.float32)
    a = {"x": x}
    if kind in ("enc", "encnorm"):
        a["wgt"] = (rs.standard_normal((cout, cin, 3, 3)) / np.sqrt(9.0 * cin)).astype(np.float32)
        a["slope"] = (0.25 + 0.1 * rs.standard_normal(cout)).astype(np.float32)
        if kind == "encnorm":
            a["mean"] = (0.2 * rs.standard_normal((bs, cin))).astype(np.float32)
            a["rstd"] = (rs.rand(bs, cin) + 0.5).astype(np.float32)
        return a
    s = (1.0 + 0.3 * rs.standard_normal((bs, nreg, cin))).astype(np.float32)
    if edge:      # make_mx_bits' planted products (its comment): x * s == value exactly, and an 11 x 11 block of all-zero pixels
        s[:] = (2.0 ** ((np.arange(cin) % 5) - 2)).astype(np.float32)[None, None, :]
        x[:, :, 2:13, 14:25] = 0.0
        for i, v in enumerate(base.EDGE_FINITE):
            for rep in range(3):
                b, c = (i + rep) % bs, (5 * i + 3 * rep) % cin
                y, xx = (7 * i + 11 * rep) % h, (3 * i + 13 * rep + 1) % w
                x[b, c, y, xx] = np.float32(v) / s[b, 0, c]
                assert np.float32(x[b, c, y, xx]) * s[b, 0, c] == np.float32(v)
    a["s"] = s
    a["wgt"] = rs.standard_normal((1, cout, cin, 3, 3)).astype(np.float32)
    a["d"] = (rs.rand(bs, nreg, cout) + 0.5).astype(np.float32)
    a["nz"] = rs.standard_normal((bs, 1, ho, wo)).astype(np.float32)
    a["ab"] = (0.1 * rs.standard_normal(cout)).astype(np.float32)
    a["lab"] = _labels(labk, rs, bs, ho, wo, nreg)
    if kind == "rgb":
        a.update({"w_rgb": rs.standard_normal((1, 3, cout, 1, 1)).astype(np.float32), "s_rgb": (1.0 + 0.3 * rs.standard_normal((bs, 1, cout))).astype(np.float32),
                  "b_rgb": (0.1 * rs.standard_normal((1, 3, 1, 1))).astype(np.float32), "s_next": (1.0 + 0.3 * rs.standard_normal((bs, 1, cout))).astype(np.float32)})
    return a


def _place(x, poison):
    """``x`` on the device: on its own, or as a contiguous view into the middle of a buffer of NaNs."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if not poison:
        return xd, None
    buf = torch.full((2 * PAD + xd.numel(),), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[PAD: PAD + xd.numel()].view(xd.shape)
    view.copy_(xd)
    return view, buf


def run_case(case, poison=None):
    """-> {"sha256": of the output bytes, "guard": how far flags[1] moved, "overflowed": the sticky bit[, "blocks": ctrl[2] of a ``blk`` case]}.
    ``poison``: None = as the case says, False = the same inputs with a stand-alone ``x``."""
    with torch.no_grad():
        return _run_case(case, case[10] if poison is None else poison)


def _run_case(case, poison):
    name, kind, bs, cin, cout, h, w, labk, edge, nreg, _ = case
    a = _inputs(case)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)  # noqa: E731
    x, buf = _place(a["x"], poison)
    flags = ops.mx_flags(DEV)
    ops.mx_overflowed()
    before = int(flags[1].item())
    res = {}
    if kind in ("enc", "encnorm"):
        wmx = ops.PreparedMx().get(t(a["wgt"]), None, False, 1)
        norm = (t(a["mean"]), t(a["rstd"])) if kind == "encnorm" else None
        outs = (ops_encode.conv3x3_mx(x, wmx, 1, cout, in_norm=norm, prelu=t(a["slope"])),)
    else:
        up = kind in ("up", "mx4", "blk")
        wgt = t(a["wgt"])
        nw = torch.tensor([0.17], device=DEV)
        blur = torch.tensor([1., 3., 3., 1.], device=DEV)
        blur = blur[:, None] * blur[None, :]
        blur = blur / blur.sum() * 4
        wt, _ = ops.PreparedWeights().get(wgt, blur if up else None, up, True)
        wmx = ops.PreparedMx().get(wgt, blur if up else None, up, 1)
        kw = {}
        if kind == "mx4":
            kw["mx4"] = ops.PreparedMx().get(wgt, blur, True, 4)
        if kind == "blk":
            kw["up_blocks"] = (ops.PreparedMx().get(wgt, None, False, 7), blur)
        if kind == "rgb":
            r_wt, _ = ops.PreparedWeights().get(t(a["w_rgb"]), None, False, False)
            kw["rgb"] = (r_wt, t(a["s_rgb"]), t(a["b_rgb"]), None, None)
            kw["s_next"] = t(a["s_next"])
        keep = (ops.SPLITK_MAX_OUT_FLOATS, ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT_SMALL)
        try:
            ops.SPLITK_MAX_OUT_FLOATS = 0                # (no split-K on these small layers: one workgroup per tile runs the whole K loop)
            # the block route as Generator(1024) takes it at 128 -> 256, with ONE threshold: UP_BLOCKS_MIN_PERCENT of the tile rows (a layer this small would
            # otherwise need UP_BLOCKS_MIN_PERCENT_SMALL of them, which the shifted cell row and the region-less corner are there to miss)
            ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT_SMALL = True, 128, 0
            out = ops.region_modconv3x3(x, wt, t(a["s"]), t(a["d"]), t(a["lab"]), t(a["nz"]), nw, t(a["ab"]), True, cout, up, mx=(wmx, 1), **kw)
        finally:
            ops.SPLITK_MAX_OUT_FLOATS, ops.UP_BLOCKS, ops.UP_BLOCKS_MIN_WIDTH, ops.UP_BLOCKS_MIN_PERCENT_SMALL = keep
        outs = out if isinstance(out, tuple) else (out,)
        if kind == "blk":
            res["blocks"] = int(ops._ctx().up_ctrl[2].item())
    torch.cuda.synchronize()
    if buf is not None:      # the kernels wrote nothing into the input's surroundings
        assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())
    res.update({"sha256": base._sha(*outs), "guard": int(flags[1].item()) - before, "overflowed": bool(ops.mx_overflowed())})
    return res


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "mx_stage_bits.json")
    rec = {}
    for case in CASES:
        rec[case[0]] = run_case(case)
        again = run_case(case)
        assert again == rec[case[0]], f"{case[0]}: two runs of one library disagree: {rec[case[0]]} / {again}"
        if case[10]:
            alone = run_case(case, poison=False)
            assert alone == rec[case[0]], f"{case[0]}: the input's surroundings reach the output: {rec[case[0]]} / stand-alone {alone}"
        print(case[0], rec[case[0]], flush=True)
    with open(dst, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
