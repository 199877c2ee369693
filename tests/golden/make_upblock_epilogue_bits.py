"""Bit record of the EPILOGUE of the region-uniform block kernel of the masked up layers (csrc/modconv_upblock_mx.hip): pre-blur tile, 4 x 4 FIR, demodulation,
noise, bias, leaky ReLU, fp32 NCHW stores.  The other records of this kernel (mx_stage_bits.json, upblock_phase_bits.json) run it at act = 1 with per-sample noise,
every optional operand present, whole channel tiles or a 32-channel rest, and a 16-byte aligned output; the branches beside that path are pinned here — SHA-256 of
the output bytes and the guard counter's move, as make_upblock_phase_bits.py records them.  Run once on the GPU at the commit whose bits are to be kept:

    python tests/golden/make_upblock_epilogue_bits.py tests/golden/upblock_epilogue_bits.json

``tests/test_gpu_upblock_epilogue.py`` imports ``CASES`` / ``run_case`` from here.  Every case calls ``e4s_masked_upconv_blocks_mx`` directly on a zero-filled
output with a hand-made block map, at cin = 32 (ONE chunk: the epilogue is most of the run).  Input 8 x 16 = one pair of blocks, the smallest launch, unless the
case says otherwise.  ``off``: the output is a view that starts ``off`` bytes past a 16-byte boundary inside a buffer of NaNs (the kernel then takes its
four-byte stores); the NaNs on both sides must survive, and the bytes must be those of the aligned run (case ``base``)."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from e4s2024_amd import ops  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_upblock_phase_bits", os.path.join(HERE, "make_upblock_phase_bits.py"))
phase = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(phase)

DEV, NREG, PAD = phase.DEV, phase.NREG, phase.stage.PAD
CIN = 32

#        name                  bs cout  h   w   what differs from `base`
CASES = [("base",               1, 64,  8, 16, {}),
         ("act0",               1, 64,  8, 16, {"act": 0}),                   # no leaky ReLU, no gain
         ("noise_null",         1, 64,  8, 16, {"noise": None}),
         ("noise_shared_b2",    2, 64,  8, 16, {"noise": "shared"}),          # noise_bs = 1 at batch 2
         ("act_bias_null",      1, 64,  8, 16, {"act_bias": None}),
         ("d_null",             1, 64,  8, 16, {"d": None}),
         ("cout72",             1, 72,  8, 16, {}),                           # the second channel tile: 8 channels = half of one 16-channel pass, none of the other three
         ("cout16",             1, 16,  8, 16, {}),
         ("b2_16x32_one_mixed", 2, 64, 16, 32, {"map": "one_mixed"}),         # two block rows, both image borders, an idle group (group 1 in sample 0, group 0 in sample 1)
         ("out_off4",           1, 64,  8, 16, {"off": 4}),
         ("out_off8",           1, 64,  8, 16, {"off": 8}),
         ("out_off12",          1, 64,  8, 16, {"off": 12})]
ALIGNED_OF = {"out_off4": "base", "out_off8": "base", "out_off12": "base"}    # same inputs (the seed ignores the name for these), aligned output


def _inputs(case):
    name, bs, cout, h, w, opt = case
    seed_name = ALIGNED_OF.get(name, name)
    a = phase._inputs((seed_name, "direct", bs, CIN, cout, h, w, "uni", False))
    if opt.get("map") == "one_mixed":
        a["blocks"][0, 0, 1] = 255          # sample 0, block row 0, pair 0: its second block is mixed
        a["blocks"][1, 1, 2] = 255          # sample 1, block row 1, pair 1: its first
    return a


def run_case(case):
    """-> {"sha256": of the output bytes, "guard": how far flags[1] moved, "overflowed": the sticky bit, "calls": how often the block kernel's entry point was called}."""
    with torch.no_grad():
        return _run_case(case)[0]


def run_case_bytes(case):
    """-> (the record of run_case, the output as a host array)."""
    with torch.no_grad():
        rec, out = _run_case(case)
        return rec, out.cpu().numpy()


def _run_case(case):
    name, bs, cout, h, w, opt = case
    a = _inputs(case)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)  # noqa: E731
    flags = ops.mx_flags(DEV)
    ops.mx_overflowed()
    before = int(flags[1].item())
    wgt = t(a["wgt"])
    nw = torch.tensor([0.17], device=DEV)
    blur = torch.tensor([1., 3., 3., 1.], device=DEV)
    blur = blur[:, None] * blur[None, :]
    blur = (blur / blur.sum() * 4).contiguous()
    wblk = ops.PreparedMx().get(wgt, None, False, 7)
    x, s, blocks = t(a["x"]), t(a["s"]), t(a["blocks"])
    d = t(a["d"]) if opt.get("d", 1) is not None else None
    ab = t(a["ab"]) if opt.get("act_bias", 1) is not None else None
    nzk = opt.get("noise", "per_sample")
    nz = None if nzk is None else t(a["nz"][:1]) if nzk == "shared" else t(a["nz"])
    noise_bs = 0 if nz is None else nz.shape[0]
    n = bs * cout * 4 * h * w
    off = opt.get("off", 0)
    assert off % 4 == 0 and 0 <= off < 16
    if off:
        buf = torch.full((2 * PAD + n + 4,), float("nan"), dtype=torch.float32, device=DEV)
        lo = PAD + off // 4
        assert buf.data_ptr() % 16 == 0 and PAD % 4 == 0
        out = buf[lo: lo + n].view(bs, cout, 2 * h, 2 * w)
        out.zero_()
    else:
        buf = None
        out = torch.zeros((bs, cout, 2 * h, 2 * w), dtype=torch.float32, device=DEV)
    assert out.data_ptr() % 16 == off
    ctrl = torch.tensor([0, 0, 1, 0], dtype=torch.int32, device=DEV)
    names = []
    lib = ops.lib()
    orig = lib.call

    def call(fn, *args):
        names.append(fn)
        return orig(fn, *args)
    lib.call = call
    try:
        lib.call("e4s_masked_upconv_blocks_mx", ops._p(out), ops._p(x), ops._p(wblk), ops._p(flags), ops._p(s), ops._p(d), ops._p(blocks), ops._p(ctrl), ops._p(blur),
                 ops._p(nz), noise_bs, ops._p(nw), ops._p(ab), opt.get("act", 1), bs, CIN, cout, h, w, NREG, ops._stream())
    finally:
        lib.call = orig
    torch.cuda.synchronize()
    if buf is not None:      # the kernel wrote nothing beside its output
        assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + n:]).all()), f"{name}: the NaNs around the output did not survive"
    assert bool(torch.isfinite(out).all()), name
    if opt.get("map") == "one_mixed":       # a mixed block is not this kernel's: its pixels keep the zeros
        assert float(out[0, :, 0:16, 16:32].abs().max()) == 0.0 and float(out[1, :, 16:32, 32:48].abs().max()) == 0.0, name
        assert float(out[0, :, 0:16, 0:16].abs().max()) > 0.0 and float(out[1, :, 16:32, 48:64].abs().max()) > 0.0, name
    rec = {"sha256": phase.stage.base._sha(out), "guard": int(flags[1].item()) - before, "overflowed": bool(ops.mx_overflowed()),
           "calls": names.count("e4s_masked_upconv_blocks_mx")}
    return rec, out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "upblock_epilogue_bits.json")
    rec = {}
    for case in CASES:
        rec[case[0]] = run_case(case)
        again = run_case(case)
        assert again == rec[case[0]], f"{case[0]}: two runs of one library disagree: {rec[case[0]]} / {again}"
        assert rec[case[0]]["calls"] == 1, f"{case[0]}: {rec[case[0]]}"
        print(case[0], rec[case[0]], flush=True)
    for name, al in ALIGNED_OF.items():
        assert rec[name] == rec[al], f"{name}: not the bytes of the aligned run: {rec[name]} / {rec[al]}"
    with open(dst, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
