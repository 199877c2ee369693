"""The parts of the chain's same-resolution kernels (csrc/modconv_chain.hip), each layer alone on the chip at batch 4: the full kernel, without its epilogue
(E4S_CHAIN_EXP=1), without its MFMAs (2), without its activation DMA (4), with none of the three (7).  Needs the phase-prof build, whose launcher reads
E4S_CHAIN_EXP at every call:

    python -m e4s2024_amd.build --phase-prof
    E4S_HIP_LIB=e4s2024_amd/lib/libe4s_hip_prof.so python tools/time_chain_parts.py

Prints the mean of 30 launches, three rounds per setting (ms)."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from e4s2024_amd import ops

dev = "cuda:0"


def t(fn, n=30):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def case(c, res, want_out, bs=4):
    torch.manual_seed(0)
    x = torch.randn(bs, c, res, res, device=dev)
    w = torch.randn(1, c, c, 3, 3, device=dev)
    s = torch.randn(bs, 1, c, device=dev) * 0.3 + 1
    d = torch.rand(bs, c, device=dev) + 0.25
    with torch.no_grad():
        wt, _ = ops.PreparedWeights().get(w, None, False, True)
        r_wt, _ = ops.PreparedWeights().get(torch.randn(1, 3, c, 1, 1, device=dev), None, False, False)
    noise = torch.randn(1, 1, res, res, device=dev)
    nw, ab = torch.tensor([0.1], device=dev), torch.randn(c, device=dev)
    k1 = torch.tensor([1., 3., 3., 1.], device=dev)
    upk = k1[:, None] * k1[None, :] / k1.sum() ** 2 * 4
    rgb = (r_wt, torch.randn(bs, 1, c, device=dev), torch.randn(1, 3, 1, 1, device=dev), torch.randn(bs, 3, res // 2, res // 2, device=dev), upk)
    s_next = torch.randn(bs, 1, c, device=dev)
    xsp = ops.to_split_planes(x, s)
    run = lambda: ops.chain_conv3x3(xsp, wt, d, noise, nw, ab, True, c, s_next=s_next if want_out else None, rgb=rgb)
    for exp, what in ((0, "full"), (1, "no epilogue"), (2, "no MFMAs"), (4, "no activation DMA"), (7, "none of the three"), (0, "full again")):
        os.environ["E4S_CHAIN_EXP"] = str(exp)
        print(f"conv {c}->{c} @{res} bs {bs}  E4S_CHAIN_EXP={exp} ({what}): " + "  ".join(f"{t(run):.4f}" for _ in range(3)) + " ms", flush=True)
    os.environ["E4S_CHAIN_EXP"] = "0"


if __name__ == "__main__":
    print("library:", os.environ.get("E4S_HIP_LIB", "product (E4S_CHAIN_EXP has no effect on it)"), flush=True)
    case(32, 1024, False)
    case(64, 512, True)
