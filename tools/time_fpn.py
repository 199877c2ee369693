"""Row f10 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.blender_fpn`` against ``ops.BlenderFPN`` run by stock PyTorch on the same device with the same seeded weights (the composition the reference
  route runs), 256 x 256 images at batch 1 and 8, eager and captured in a graph;
* ``ops.blender_forward`` against the same forward with that stock composition producing the features (``blender_recolor`` after it in both), eager.

    python tools/time_fpn.py [--rounds 5] [--json out.json]
    python tools/time_fpn.py --profile-pass                # a few native FPN calls at batch 1 and nothing else: the run to put under
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
import torch

import colorref_model as CM
import fpn_model as FM
import resunet_model as RM
from e4s2024_amd import ops
from time_resunet import alternate, graphed

dev = "cuda:0"
H = W = 256


def conv_flop(bs, h=H, w=W):
    """Multiply-adds x 2 of one FPN call at ``bs`` images, from the layer shapes: (encoder, SPADE blocks' own convolutions, gamma / beta, shared MLPs)."""
    h2, w2 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    h4, w4 = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    enc = 9 * (h * w * 3 * 64 + h2 * w2 * 64 * 128 + h2 * w2 * 128 * 256 + h4 * w4 * 256 * 512 + h4 * w4 * 512 * 512)
    px = h4 * w4
    blocks = px * (9 * (512 * 512 * 2) * 2 + 9 * (512 * 256 + 256 * 256) + 512 * 256)
    norms = (512, 512, 512, 512, 512, 256, 512)
    gb = px * 9 * 128 * 2 * sum(norms)
    shared = px * 27 * 128 * len(norms)
    return tuple(2 * bs * v for v in (enc, blocks, gb, shared))


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    whole = ops.BlenderNet().eval()
    whole.referencer.FPN.load_state_dict(FM.state_dict())
    whole.unet.load_state_dict(RM.state_dict(64))
    whole.referencer.trainable_tao.fill_(7.0)
    whole = whole.to(dev)
    net = whole.referencer.FPN
    if a.profile_pass:
        x = torch.from_numpy(FM.images(5, 1, H, W)).to(dev)
        for _ in range(12):
            ops.blender_fpn(x, net)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_fpn", "profile_pass": True, "calls": 12, "ok": True}))
        return
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"blender_fpn against ops.BlenderFPN on stock PyTorch, {H} x {W}, {doc['device']}")
    for bs in (1, 8):
        x = torch.from_numpy(FM.images(5, bs, H, W)).to(dev)
        agree = float((ops.blender_fpn(x, net) - net(x)).abs().max())
        parts = conv_flop(bs)
        gflop = sum(parts) / 1e9
        reps = 10 if bs == 1 else 3
        fns = {"hip": lambda: ops.blender_fpn(x, net), "torch": lambda: net(x)}
        for mode in ("eager", "graph"):
            if mode == "graph":
                fns = {k: graphed(fn) for k, fn in fns.items()}
            res = alternate(fns, a.rounds, reps)
            s = spread(res)
            for k, v in s.items():
                print(f"  fpn bs {bs} {mode:5s} {k:5s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}   "
                      f"{gflop / v['median_ms']:.1f} TFLOP/s of {gflop:.1f} GFLOP counted", flush=True)
            faster = max(res["hip"]) < min(res["torch"])
            print(f"  fpn bs {bs} {mode}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch round: "
                  f"{faster}", flush=True)
            doc["cases"][f"fpn bs{bs} {mode}"] = {**s, "hip_faster_beyond_spread": faster, "gflop_counted": gflop, "gflop_parts": [p / 1e9 for p in parts],
                                                  "outputs_agree_to": agree}
        print(f"  fpn bs {bs}: outputs agree to {agree:.1e}; GFLOP encoder / blocks / gamma-beta / shared = " + " / ".join(f"{p / 1e9:.1f}" for p in parts),
              flush=True)
        img_a, img_t = (torch.from_numpy(CM.image(500 + i, bs, H, W)).to(dev) for i in range(2))
        lab_a, lab_t = (torch.from_numpy(CM.blocky_labels(510 + i, bs, H, W, 32)).to(dev) for i in range(2))

        def stock_forward():
            return ops.blender_recolor(img_a, img_t, lab_a, lab_t, net(img_a), net(img_t), whole.referencer.trainable_tao.detach().reshape(1), whole.unet)

        fns = {"hip": lambda: ops.blender_forward(img_a, img_t, lab_a, lab_t, whole, False), "torch": stock_forward}
        agree = float((fns["hip"]()[0] - fns["torch"]()[0]).abs().max())
        res = alternate(fns, a.rounds, max(reps // 2, 2))
        s = spread(res)
        for k, v in s.items():
            print(f"  forward bs {bs} eager {k:5s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}", flush=True)
        faster = max(res["hip"]) < min(res["torch"])
        print(f"  forward bs {bs}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch round: {faster}; "
              f"predictions agree to {agree:.1e}", flush=True)
        doc["cases"][f"forward bs{bs} eager"] = {**s, "hip_faster_beyond_spread": faster, "outputs_agree_to": agree}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_fpn", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
