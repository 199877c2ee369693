"""Row f9 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

``ops.blender_unet`` against ``ops.ResUNet`` run by stock PyTorch on the same device with the same seeded weights (the composition the reference route
runs), 256 x 256 packages at batch 1 and 8, eager and captured in a graph.

    python tools/time_resunet.py [--rounds 5] [--json out.json]
    python tools/time_resunet.py --profile-pass            # a few native calls at batch 1 and nothing else: the run to put under
                                                           # rocprofv3 --kernel-trace --stats for the per-kernel shares

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The convolution work is
counted from the layer shapes (``conv_flop``) and printed with the rate it gives."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import resunet_model as RM
from e4s2024_amd import ops

dev = "cuda:0"
H = W = 256
WIDTH = 64


def conv_flop(bs, width=WIDTH, h=H, w=W):
    """Multiply-adds x 2 of the network's 22 convolutions (7 blocks x (conv1, conv2, sqz) and the head) at ``bs`` images, from the layer shapes."""
    total = 0
    chans = [(12, width, 1, 0), (width, 2 * width, 2, 1), (2 * width, 4 * width, 2, 2), (4 * width, 8 * width, 2, 3),
             (12 * width, 4 * width, 1, 2), (6 * width, 2 * width, 1, 1), (3 * width, width, 1, 0)]
    for cin, cout, _, level in chans:
        px = (h >> level) * (w >> level)
        total += px * cout * (9 * cin + 9 * cout + cin)
    total += h * w * 3 * width
    return 2 * total * bs


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, rounds, reps):
    """{name: [ms per call, one per round]}: every function warmed, then round by round one after the other."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps))
    return out


def graphed(fn):
    """``fn`` captured after a warm-up on a side stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    net = ops.ResUNet(WIDTH).eval()
    net.load_state_dict(RM.state_dict(WIDTH))
    net = net.to(dev)
    if a.profile_pass:
        x = torch.from_numpy(RM.packages(5, 1, H, W)).to(dev)
        for _ in range(12):
            ops.blender_unet(x, net)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_resunet", "profile_pass": True, "calls": 12, "ok": True}))
        return
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"blender_unet against ops.ResUNet on stock PyTorch, width {WIDTH}, {H} x {W}, {doc['device']}")
    for bs in (1, 8):
        x = torch.from_numpy(RM.packages(5, bs, H, W)).to(dev)
        agree = float((ops.blender_unet(x, net) - net(x)).abs().max())
        gflop = conv_flop(bs) / 1e9
        reps = 20 if bs == 1 else 5
        fns = {"hip": lambda: ops.blender_unet(x, net), "torch": lambda: net(x)}
        for mode in ("eager", "graph"):
            if mode == "graph":
                fns = {k: graphed(fn) for k, fn in fns.items()}
            res = alternate(fns, a.rounds, reps)
            s = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}
            for k, v in s.items():
                print(f"  bs {bs} {mode:5s} {k:5s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}   "
                      f"{gflop / v['median_ms']:.1f} TFLOP/s of {gflop:.1f} GFLOP counted", flush=True)
            faster = max(res["hip"]) < min(res["torch"])
            print(f"  bs {bs} {mode}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch round: {faster}",
                  flush=True)
            doc["cases"][f"bs{bs} {mode}"] = {**s, "hip_faster_beyond_spread": faster, "gflop_counted": gflop, "outputs_agree_to": agree}
        print(f"  bs {bs}: outputs agree to {agree:.1e}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_resunet", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
