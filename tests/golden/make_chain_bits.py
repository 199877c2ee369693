"""Bit record of the chain's same-resolution convolutions (csrc/modconv_chain.hip, ``e4s_chain_conv3x3``): SHA-256 of the hi and the lo output plane, of the 16
bytes behind them (64 -> 64 variant: the one with the split-plane hand-over) and of the fused ToRGB image, for seeded inputs.  Run once on the GPU at the commit whose
bits are to be kept:

    python tests/golden/make_chain_bits.py tests/golden/chain_bits.json

``tests/test_gpu_chain_bits.py`` imports ``CASES`` / ``run_case`` from here.  Every case calls the entry point directly on output buffers filled with 0x5a5a (a
pixel the kernel does not write, or a tail it does not zero, shows in the hash).  The inputs come from numpy's generator on the host, so the record does not depend
on the device's random numbers.  The shapes are the smallest that reach each path of the 16 x 32 tile (h % 16 == 0 and w % 32 == 0 is the entry point's contract):
one tile that touches all four borders, two tiles either way, 3 x 3 tiles with an interior one, batch 1 - 3, noise per sample / shared / none, the skip image
present and absent, activation on and off, no activation bias, and per variant one case with more tiles than twice the CUs of the chip (batch 3 of 160 x 640 = 600
tiles), so that a workgroup of the persistent kernel walks three tiles and reloads its per-sample tables on the way."""
import ctypes
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

#        name          c    h    w  bs  noise         skip   act    act_bias      (c = 32: 32 -> 32 + ToRGB, the last layer; c = 64: 64 -> 64 + ToRGB + split planes)
CASES = [("c32_16x32", 32,  16,  32, 1, "per_sample", True,  True,  True),
         ("c64_16x32", 64,  16,  32, 1, "shared",     True,  True,  True),
         ("c32_32x32", 32,  32,  32, 2, "shared",     False, True,  True),
         ("c64_32x32", 64,  32,  32, 3, "per_sample", True,  False, True),
         ("c32_16x64", 32,  16,  64, 3, None,         True,  False, True),
         ("c64_16x64", 64,  16,  64, 2, None,         False, True,  True),
         ("c32_48x96", 32,  48,  96, 2, "per_sample", True,  True,  False),
         ("c64_48x96", 64,  48,  96, 3, "shared",     True,  True,  False),
         ("c32_many",  32, 160, 640, 3, "shared",     True,  True,  True),
         ("c64_many",  64, 160, 640, 3, "per_sample", True,  True,  True)]


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case):
    """-> {"rgb": SHA-256 of the image's bytes} and, for the 64 -> 64 variant, {"hi", "lo", "tail"}: of the two planes and of the 16 bytes behind them."""
    name, c, h, w, bs, noise, skip, act, bias = case
    rng = np.random.default_rng(_seed(name))
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV)  # noqa: E731
    with torch.no_grad():
        x, wgt = f(bs, c, h, w), f(1, c, c, 3, 3)
        s = (f(bs, 1, c) * 0.3 + 1.0).contiguous()
        d = (f(bs, c).abs() * 0.5 + 0.25).contiguous()
        sn = (f(bs, c) * 0.3 + 1.0).contiguous()
        ab = f(c) if bias else None
        nz = None if noise is None else f(bs if noise == "per_sample" else 1, h * w)
        nw = torch.tensor([0.17], device=DEV)
        r_wt, r_s, r_bias = (f(c, 3) * 0.2).contiguous(), (f(bs, c) * 0.3 + 1.0).contiguous(), f(3)
        sk = f(bs, 3, h // 2, w // 2) if skip else None
        k1 = torch.tensor([1., 3., 3., 1.], device=DEV)
        upk = (k1[:, None] * k1[None, :] / k1.sum() ** 2 * 4).contiguous()
        wt, _ = ops.PreparedWeights().get(wgt, None, False, True)
        xsp = ops.to_split_planes(x, s)
        want_out = c == 64
        n = 2 * bs * c * h * w
        buf = torch.full((n + 8,), 0x5a5a, dtype=torch.int16, device=DEV) if want_out else None
        rgb = torch.full((bs * 3 * h * w * 2,), 0x5a5a, dtype=torch.int16, device=DEV)      # fp32 [bs, 3, h, w], as raw bytes
        L = ops.ChainLayer()
        L.x_sp, L.whi, L.wlo, L.d = xsp.data_ptr(), wt[0].data_ptr(), wt[1].data_ptr(), d.data_ptr()
        if nz is not None:
            L.noise, L.noise_bs, L.noise_weight = nz.data_ptr(), nz.shape[0], nw.data_ptr()
        if ab is not None:
            L.act_bias = ab.data_ptr()
        L.act = 1 if act else 0
        if want_out:
            assert buf.data_ptr() % 16 == 0
            L.out_sp, L.s_next = buf.data_ptr(), sn.data_ptr()
        L.rgb_out, L.rgb_wt, L.rgb_s, L.rgb_bias = rgb.data_ptr(), r_wt.data_ptr(), r_s.data_ptr(), r_bias.data_ptr()
        if sk is not None:
            L.rgb_skip, L.rgb_up_kernel = sk.data_ptr(), upk.data_ptr()
        L.bs, L.cin, L.cout, L.h, L.w = bs, c, c, h, w
        ops.lib().call("e4s_chain_conv3x3", ctypes.byref(L), ops._stream())
        torch.cuda.synchronize()
        rec = {"rgb": _sha(rgb)}
        if want_out:
            rec.update({"hi": _sha(buf[:n // 2]), "lo": _sha(buf[n // 2:n]), "tail": _sha(buf[n:])})
        return rec


ZERO_TAIL = hashlib.sha256(bytes(16)).hexdigest()


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "chain_bits.json")
    rec = {}
    for case in CASES:
        rec[case[0]] = run_case(case)
        again = run_case(case)
        assert again == rec[case[0]], f"{case[0]}: two runs of one library disagree: {rec[case[0]]} / {again}"
        assert rec[case[0]].get("tail", ZERO_TAIL) == ZERO_TAIL, f"{case[0]}: the 16 bytes behind the planes are not zero"
        print(case[0], rec[case[0]], flush=True)
    with open(dst, "w") as f_:
        json.dump(rec, f_, indent=1, sort_keys=True)
        f_.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
