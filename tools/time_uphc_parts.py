"""The parts of the persistent half-composed up kernel (csrc/modconv_uphc.hip), each layer alone on the chip at batch 4: the full kernel, without its epilogue
(E4S_HC_EXP=1), without its MFMAs (2), with neither (3), with everything but the output stores (4).  Needs the phase-prof build, whose launcher reads E4S_HC_EXP at
every call:

    python -m e4s2024_amd.build --phase-prof
    E4S_HIP_LIB=e4s2024_amd/lib/libe4s_hip_prof.so python tools/time_uphc_parts.py

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


def case(cin, cout, res, bs=4):
    torch.manual_seed(1)
    x = torch.randn(bs, cin, res, res, device=dev)
    w = torch.randn(1, cout, cin, 3, 3, device=dev)
    s = torch.randn(bs, 1, cin, device=dev) * 0.3 + 1
    d = torch.rand(bs, cout, device=dev) + 0.25
    k1 = torch.tensor([1., 3., 3., 1.], device=dev)
    blur = k1[:, None] * k1[None, :] / k1.sum() ** 2 * 4
    noise = torch.randn(1, 1, 2 * res, 2 * res, device=dev)
    nw, ab = torch.tensor([0.1], device=dev), torch.randn(cout, device=dev)
    s_next = torch.randn(bs, 1, cout, device=dev)
    hc = ops.PreparedHc().get(w, blur)
    xsp = ops.to_split_planes(x, s)
    run = lambda: ops.modconv_up_single(xsp, None, s, d, blur, noise, nw, ab, True, cout, s_next=s_next, hc=hc)
    for exp, what in ((0, "full"), (1, "no epilogue"), (2, "no MFMAs"), (3, "neither"), (4, "all but the stores"), (0, "full again")):
        os.environ["E4S_HC_EXP"] = str(exp)
        print(f"up {cin}->{cout} @{res}->{2 * res} bs {bs}  E4S_HC_EXP={exp} ({what}): " + "  ".join(f"{t(run):.4f}" for _ in range(3)) + " ms", flush=True)
    os.environ["E4S_HC_EXP"] = "0"


if __name__ == "__main__":
    print("library:", os.environ.get("E4S_HIP_LIB", "product (E4S_HC_EXP has no effect on it)"), flush=True)
    case(64, 32, 512)
    case(128, 64, 256)
