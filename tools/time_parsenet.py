"""Row f13 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.parsenet_mask`` (uint8 faces to 0 / 255 masks) against ``ops.ParseNet.forward`` + ``argmax`` + the colour table run by stock PyTorch on the same device
  with the same seeded weights, and ``ops.parsenet_forward(with_image=True)`` against ``ops.ParseNet.forward`` alone: the network ``FaceParse`` builds
  (512, 512, 32, 64, 19, ch_range [32, 256]) at batch 1 and 4, eager and captured in a graph.

    python tools/time_parsenet.py [--rounds 5] [--json out.json]
    python tools/time_parsenet.py --profile-pass           # a few native calls at batch 1 and nothing else: the run to put under
                                                           # rocprofv3 --kernel-trace for the per-kernel shares (tools/rocpd_summary.py)

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The native route counts as not
slower only if its slowest round is below the stock route's fastest.  The multiply-adds are counted from the layer shapes and printed with the rate they
give (the stock route always runs both heads; ``parsenet_mask`` runs the 19-output one)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import parsenet_model as PM
from e4s2024_amd import ops, seeded
from time_resunet import alternate, graphed

dev = "cuda:0"
SIZE = 512
WARMUP = 30                                  # calls of either route before a batch size is timed


def flop(net, size=SIZE, image_head=True):
    """Multiply-adds x 2 of one sample, counted from the layer shapes."""
    c0, blocks, head, ncls = net.structure
    macs = 27 * c0 * size * size
    h = size
    for _, scale, cin, cout in blocks:
        ho = (h - 1) // 2 + 1 if scale == "down" else 2 * h if scale == "up" else h
        mid = 2 * h if scale == "up" else h                                                    # conv1's output: before the stride, behind the upsampling
        macs += 9 * cin * cout * mid * mid + 9 * cout * cout * ho * ho
        if scale != "none" or cin != cout:
            macs += 9 * cin * cout * ho * ho
        h = ho
    return 2 * (macs + 9 * head * (ncls + (3 if image_head else 0)) * h * h)


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    net = ops.ParseNet().eval()
    with torch.device("meta"):
        template = ops.ParseNet().state_dict()
    net.load_state_dict(seeded.seeded_parsenet_state_dict(template, PM.WEIGHT_SEED), strict=True)
    net = net.to(dev)
    cmap = torch.tensor(ops.MASK_COLORMAP, dtype=torch.uint8, device=dev)
    faces = lambda bs: torch.from_numpy(PM.images_u8(5, bs, SIZE, SIZE)).to(dev)              # noqa: E731
    if a.profile_pass:
        img = faces(1)
        for _ in range(6):
            ops.parsenet_mask(img, net)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_parsenet", "profile_pass": True, "calls": 6, "ok": True}))
        return
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"parsenet_mask / parsenet_forward against ops.ParseNet.forward on stock PyTorch, size {SIZE}, {doc['device']}; per sample "
          f"{flop(net) / 1e9:.1f} GFLOP counted with both heads, {flop(net, image_head=False) / 1e9:.1f} with the mask head alone")
    for bs in (1, 4):
        img = faces(bs)
        x = torch.from_numpy(PM.img2tensor(img.cpu().numpy())).to(dev)
        want = net(x)
        got = ops.parsenet_forward(x, net, with_image=True)
        agree = max(float((got[0] - want[0]).abs().max()), float((got[1] - want[1]).abs().max()))
        masks_differ = float((ops.parsenet_mask(img, net) != cmap[want[0].argmax(1)]).float().mean())
        for _ in range(WARMUP):                                                                # the clocks settle: the first block is timed like the later ones
            ops.parsenet_mask(img, net)
            net(x)
        pairs = {"mask": ({"hip": lambda: ops.parsenet_mask(img, net), "torch": lambda: cmap[net(x)[0].argmax(1)]}, flop(net, image_head=False)),
                 "forward": ({"hip": lambda: ops.parsenet_forward(x, net, with_image=True), "torch": lambda: net(x)}, flop(net))}
        for what, (fns, fl) in pairs.items():
            gflop = bs * fl / 1e9
            for mode in ("eager", "graph"):
                if mode == "graph":
                    fns = {k: graphed(fn) for k, fn in fns.items()}
                res = alternate(fns, a.rounds, 3)
                s = spread(res)
                for k, v in s.items():
                    print(f"  {what:7s} bs {bs} {mode:5s} {k:5s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}   "
                          f"{gflop / v['median_ms']:.1f} TFLOP/s of {gflop:.1f} GFLOP the native route computes", flush=True)
                faster = max(res["hip"]) < min(res["torch"])
                print(f"  {what:7s} bs {bs} {mode}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch "
                      f"round: {faster}", flush=True)
                doc["cases"][f"{what} bs{bs} {mode}"] = {**s, "hip_not_slower_beyond_spread": faster, "gflop_counted": gflop}
        print(f"  bs {bs}: outputs agree to {agree:.1e} (max |logit| {float(want[0].abs().max()):.2f}), {masks_differ:.5f} of the mask pixels differ", flush=True)
        doc["cases"][f"agreement bs{bs}"] = {"outputs_agree_to": agree, "mask_pixels_differ": masks_differ}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_parsenet", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
