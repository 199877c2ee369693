"""Bit record of the half-composed up layer (csrc/modconv_uphc.hip, ``e4s_modconv_up_hc``): SHA-256 of the hi and the lo output plane and of the 16 bytes behind
them, for seeded inputs.  Run once on the GPU at the commit whose bits are to be kept:

    python tests/golden/make_uphc_bits.py tests/golden/uphc_bits.json

``tests/test_gpu_uphc_bits.py`` imports ``CASES`` / ``run_case`` from here.  Every case calls the entry point directly on an output buffer filled with 0x5a5a
(a pixel the kernel does not write, or a tail it does not zero, shows in the hash).  The inputs come from numpy's generator on the host, so the record does not
depend on the device's random numbers.  The shapes are the smallest that cross the tile edges of the 16 x 16 (14 kept columns) and of the 8 x 32 (30 kept columns)
geometry: widths one short of, equal to and one past one and two tiles, heights around one and two tile rows, 2 / 4 / 8 chunks, 1 - 3 channel tiles, batch 1 - 3,
noise per sample / shared / none, activation on / off, no activation bias, the asymmetric rank-1 blur of test_gpu_chain.py, a rank-1 blur from 1-3-3-1, one
case with more tiles than twice the CUs of the chip, so that a workgroup of the persistent kernel walks several items, and two whose last round of the walk is a
partial one with several channel tiles per tile."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from e4s2024_amd import ops  # noqa: E402

DEV = "cuda:0"

#        name            cin cout   h    w  bs  noise         act    asym   act_bias
CASES = [("w14_h7",       32,  32,   7,  14, 1, "per_sample", True,  False, True),
         ("w15_h8",       64,  64,   8,  15, 2, "shared",     False, True,  True),
         ("w29_h9",      128,  96,   9,  29, 3, None,         True,  False, True),
         ("w30_h17",      32,  64,  17,  30, 2, "per_sample", True,  True,  True),
         ("w31_h8",       64,  32,   8,  31, 1, None,         False, False, True),
         ("w32_h9",       32,  96,   9,  32, 1, "per_sample", True,  False, False),
         ("w37_h17",     128,  32,  17,  37, 2, "per_sample", True,  True,  True),
         ("w61_h7",       64,  96,   7,  61, 3, "shared",     True,  False, True),
         ("w60_h16",      32,  32,  16,  60, 1, "per_sample", True,  False, True),
         ("w28_h16",      64,  64,  16,  28, 1, "shared",     True,  True,  True),
         ("many_tiles",   32,  32, 160, 300, 3, "shared",     True,  False, True),
         # more tiles than CUs with 2 / 3 channel tiles each: the tiles left over after the full rounds of the persistent walk (270 = 256 + 14 and 360 = 256 + 104
         # tiles of 8 x 30 on 256 CUs) are handed out by item, one per workgroup and two per workgroup (the second pair straddles two tiles)
         ("split_round1", 32,  64,  72, 300, 3, "per_sample", True,  False, True),
         ("split_round2", 32,  96, 240, 120, 3, "shared",     True,  True,  True)]


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case):
    """-> {"hi": SHA-256 of the hi plane's bytes, "lo": of the lo plane's, "tail": of the 16 bytes behind the two planes}."""
    name, cin, cout, h, w, bs, noise, act, asym, bias = case
    rng = np.random.default_rng(_seed(name))
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)  # noqa: E731
    with torch.no_grad():
        x, wgt = f(bs, cin, h, w), f(1, cout, cin, 3, 3)
        s = (f(bs, 1, cin) * 0.3 + 1.0).contiguous()
        d = (f(bs, cout).abs() * 0.5 + 0.25).contiguous()
        sn = (f(bs, cout) * 0.3 + 1.0).contiguous()
        ab = f(cout) if bias else None
        nz = None if noise is None else f(bs if noise == "per_sample" else 1, 1, 2 * h, 2 * w)
        nw = torch.tensor([0.17], device=DEV)
        if asym:
            blur = (torch.tensor([1., 2., 5., 1.], device=DEV)[:, None] * torch.tensor([2., 3., 1., 1.], device=DEV)[None, :] / 63 * 4).contiguous()
        else:
            k1 = torch.tensor([1., 3., 3., 1.], device=DEV)
            blur = (k1[:, None] * k1[None, :] / k1.sum() ** 2 * 4).contiguous()
        assert ops.blur_is_rank1(blur)
        hc = ops.PreparedHc().get(wgt, blur)
        assert hc is not None, "the half-composed route is switched off"
        xsp = ops.to_split_planes(x, s)
        n = 2 * bs * cout * 4 * h * w
        buf = torch.full((n + 8,), 0x5a5a, dtype=torch.int16, device=DEV)
        assert buf.data_ptr() % 16 == 0
        ops.lib().call("e4s_modconv_up_hc", ops._p(buf), ops._p(xsp), ops._p(hc[0]), ops._p(hc[1]), ops._p(d), ops._p(blur), ops._p(nz), 0 if nz is None else nz.shape[0],
                       ops._p(nw) if nz is not None else None, ops._p(ab), 1 if act else 0, bs, cin, cout, h, w, ops._p(sn), ops._stream())
        torch.cuda.synchronize()
        return {"hi": _sha(buf[:n // 2]), "lo": _sha(buf[n // 2:n]), "tail": _sha(buf[n:])}


ZERO_TAIL = hashlib.sha256(bytes(16)).hexdigest()


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "uphc_bits.json")
    rec = {}
    for case in CASES:
        rec[case[0]] = run_case(case)
        again = run_case(case)
        assert again == rec[case[0]], f"{case[0]}: two runs of one library disagree: {rec[case[0]]} / {again}"
        assert rec[case[0]]["tail"] == ZERO_TAIL, f"{case[0]}: the 16 bytes behind the planes are not zero"
        print(case[0], rec[case[0]], flush=True)
    with open(dst, "w") as f_:
        json.dump(rec, f_, indent=1, sort_keys=True)
        f_.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
