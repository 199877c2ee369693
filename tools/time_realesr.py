"""Row f11 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.realesr_forward`` against ``ops.RRDBNet`` run by stock PyTorch on the same device with the same seeded weights (what the reference route runs
  through basicsr), 23 blocks, 256 x 256 images at batch 1 and 4, eager, and at batch 1 captured in a graph;
* ``pipeline.color_transfer_blender`` (two face parses, the recolouring network, Pillow's resize, the Real-ESRGAN step) at 1024 x 1024, batch 1, with the
  time of its last step, ``pipeline.realesr_infer_image``, beside it.

    python tools/time_realesr.py [--rounds 5] [--json out.json]
    python tools/time_realesr.py --profile-pass            # a few native network calls at batch 1 and nothing else: the run to put under
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

import rrdb_model as RM
from e4s2024_amd import ops, pipeline, seeded
from time_resunet import alternate, graphed

dev = "cuda:0"
H = W = 256
BLOCKS = 23


def conv_flop(bs, num_block=BLOCKS, h=H, w=W):
    """Multiply-adds x 2 of one network call at ``bs`` images, from the layer shapes: (dense blocks, the rest at h x w, the three convolutions behind the
    upsampling and conv_last)."""
    rdb = sum(9 * (64 + 32 * k) * 32 for k in range(4)) + 9 * 192 * 64
    body = num_block * 3 * rdb * h * w
    low = 9 * (3 * 64 + 64 * 64) * h * w
    up = 9 * 64 * 64 * (4 * h * w + 2 * 16 * h * w) + 9 * 64 * 3 * 16 * h * w
    return tuple(2 * bs * v for v in (body, low, up))


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    sd = RM.base_state_dict(BLOCKS)
    sd = RM.calibrated(sd, RM.network(sd, RM.images01(1, 1, 12, 12)))                         # conv_last rescaled on a small input: an image, not a flat field
    net = ops.RRDBNet(BLOCKS).eval()
    net.load_state_dict(sd)
    net = net.to(dev)
    if a.profile_pass:
        x = torch.from_numpy(RM.images01(5, 1, H, W)).to(dev)
        for _ in range(6):
            ops.realesr_forward(x, net)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_realesr", "profile_pass": True, "calls": 6, "ok": True}))
        return
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"realesr_forward against ops.RRDBNet on stock PyTorch, {BLOCKS} blocks, {H} x {W}, {doc['device']}")
    for bs in (1, 4):
        x = torch.from_numpy(RM.images01(5, bs, H, W)).to(dev)
        agree = float((ops.realesr_forward(x, net) - net(x)).abs().max())
        parts = conv_flop(bs)
        gflop = sum(parts) / 1e9
        fns = {"hip": lambda: ops.realesr_forward(x, net), "torch": lambda: net(x)}
        for mode in ("eager", "graph") if bs == 1 else ("eager",):
            if mode == "graph":
                fns = {k: graphed(fn) for k, fn in fns.items()}
            res = alternate(fns, a.rounds, 3 if bs == 1 else 1)
            s = spread(res)
            for k, v in s.items():
                print(f"  network bs {bs} {mode:5s} {k:5s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}   "
                      f"{gflop / v['median_ms']:.1f} TFLOP/s of {gflop:.1f} GFLOP counted", flush=True)
            faster = max(res["hip"]) < min(res["torch"])
            print(f"  network bs {bs} {mode}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch round: "
                  f"{faster}", flush=True)
            doc["cases"][f"network bs{bs} {mode}"] = {**s, "hip_faster_beyond_spread": faster, "gflop_counted": gflop, "gflop_parts": [p / 1e9 for p in parts],
                                                      "outputs_agree_to": agree}
        print(f"  network bs {bs}: outputs agree to {agree:.1e}; GFLOP dense blocks / rest at 256 / behind the upsampling = "
              + " / ".join(f"{p / 1e9:.1f}" for p in parts), flush=True)

    # the whole 'blender' colour transfer at the pipeline's size
    import e4s2024_amd
    e4s2024_amd.install()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    parser = FaceParser(None, device=dev)
    seeded.apply_seeded(parser.seg, 7, "bisenet")
    parser.seg.eval()
    blender = ops.BlenderNet().eval()
    blender.referencer.FPN.load_state_dict(seeded.seeded_fpn_state_dict(22))
    blender.unet.load_state_dict(seeded.seeded_resunet_state_dict(21, 64))
    blender.referencer.trainable_tao.fill_(7.0)
    blender = blender.to(dev)
    a_u8, t_u8 = (ops.tensor2im_u8(seeded.seeded_image(31 + i, 1, 1024).to(dev)) for i in range(2))
    fns = {"color_transfer_blender": lambda: pipeline.color_transfer_blender(a_u8, t_u8, parser, blender, net, flip_target=False),
           "realesr_infer_image": lambda: pipeline.realesr_infer_image(net, a_u8)}
    s = spread(alternate(fns, a.rounds, 3))
    for k, v in s.items():
        print(f"  {k} bs 1, 1024 x 1024: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}", flush=True)
    doc["cases"]["color_transfer_blender bs1"] = s
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_realesr", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
