"""Row f16 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.gpen_sr_image`` against the mirror module ``ops.GpenSRNet`` run by stock PyTorch on the same device with the same seeded weights and the ends of
  ``RealESRNet.process`` as tensor operations (what the reference route runs, without its two host round trips), scale 4, 23 blocks, ``num_feat`` 32 (what
  ``RealESRNet`` builds) and 64, batch 1, square images of the given sizes;
* ``ops.cv_resize_linear`` of a frame to four times its size;
* ``pipeline.gpen_face_enhancement`` per frame: a 256 x 256 frame, the x4 RealESRNet pass (``num_feat`` 32), the 512 generator, the default ParseNet and the
  ResNet-50 detector on the 1024 x 1024 result, one face (tools/time_gpen_frame.py's synthetic detections), with ``gpen_enhance_frames`` on a 1024 x 1024
  frame beside it: the difference is the RealESRNet pass and the resize.

    python tools/time_gpen_sr.py [--sizes 256 512 1024] [--rounds 5] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The convolution work is counted
from the layer shapes (``conv_flop``) and printed with the rate it gives."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import gpen_sr_model as M
from e4s2024_amd import ops, pipeline
from time_gpen_frame import faces_of, networks
from time_resunet import alternate

dev = "cuda:0"
BLOCKS, SCALE = 23, 4


def conv_flop(nf, h, w, num_block=BLOCKS):
    """Multiply-adds x 2 of one scale-4 network call on an h x w image, from the layer shapes."""
    rdb = sum(9 * (nf + 32 * k) * 32 for k in range(4)) + 9 * (nf + 128) * nf
    low = num_block * 3 * rdb + 9 * (3 * nf + nf * nf)
    up = 9 * nf * nf * (4 + 2 * 16) + 9 * nf * 3 * 16
    return 2 * (low + up) * h * w


def sr_net(nf):
    sd = M.base_state_dict(SCALE, nf, BLOCKS)
    sd = M.calibrated(sd, M.process(sd, M.images_u8(1, 1, 12, 12))[0])                         # conv_last rescaled on a small input: an image, not a flat field
    net = ops.GpenSRNet(BLOCKS, nf, SCALE).eval()
    net.load_state_dict(sd)
    return net.to(dev)


def stock_image(img_u8, net):
    """``RealESRNet.process`` at scale 4 as stock tensor operations around the mirror module, BGR uint8 ``[1, H, W, 3]`` in and out, all on the device."""
    x = (img_u8.float() / 255.).flip(-1).permute(0, 3, 1, 2)
    y = net(x).clamp_(0, 1).flip(1).permute(0, 2, 3, 1)
    return (y * 255.0).round().to(torch.uint8)


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"gpen_sr_image against ops.GpenSRNet on stock PyTorch, scale {SCALE}, {BLOCKS} blocks, batch 1, {doc['device']}")
    nets = {nf: sr_net(nf) for nf in (32, 64)}
    for size in a.sizes:
        img = torch.from_numpy(M.images_u8(size, 1, size, size)).to(dev)
        for nf, net in nets.items():
            off = (ops.gpen_sr_image(img, net).int() - stock_image(img, net).int()).abs()
            gflop = conv_flop(nf, size, size) / 1e9
            res = alternate({"hip": lambda: ops.gpen_sr_image(img, net), "torch": lambda: stock_image(img, net)}, a.rounds, 3 if size <= 256 else 1)
            s = spread(res)
            for k, v in s.items():
                print(f"  {size:4d}^2 num_feat {nf} {k:5s}: median {v['median_ms']:9.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}   "
                      f"{gflop / v['median_ms']:.1f} TFLOP/s of {gflop:.1f} GFLOP counted", flush=True)
            faster = max(res["hip"]) < min(res["torch"])
            print(f"  {size:4d}^2 num_feat {nf}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch "
                  f"round: {faster}; images differ on {float((off > 0).float().mean()):.2e} of the values, by {int(off.max())} at the most", flush=True)
            doc["cases"][f"sr_image {size} nf{nf}"] = {**s, "hip_faster_beyond_spread": faster, "gflop_counted": gflop,
                                                      "values_off": float((off > 0).float().mean()), "largest_difference": int(off.max())}
        s = spread(alternate({"resize": lambda: ops.cv_resize_linear(img, (4 * size, 4 * size))}, a.rounds, 10))
        v = s["resize"]
        print(f"  {size:4d}^2 cv_resize_linear to {4 * size}^2: median {v['median_ms']:.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}", flush=True)
        doc["cases"][f"cv_resize_linear {size}"] = s

    # the whole of FaceEnhancement.process per frame, "GPEN x4": a 256 x 256 frame to 1024 x 1024
    det, gen, par = networks()
    rng = np.random.default_rng(0)
    dets, landms = faces_of(1, rng)
    real_detect = pipeline.gpen_detect_faces

    def detect(net, fr, bgr=True):
        real_detect(net, fr, bgr=bgr)                                                         # its time is spent; its arbitrary detections are replaced
        return [(dets, landms)] * fr.shape[0]

    small = torch.from_numpy(M.images_u8(3, 1, 256, 256)).to(dev)
    big = ops.cv_resize_linear(small, (1024, 1024))
    pipeline.gpen_detect_faces = detect
    try:
        s = spread(alternate({"gpen_face_enhancement": lambda: pipeline.gpen_face_enhancement(det, gen, par, nets[32], small),
                              "gpen_enhance_frames": lambda: pipeline.gpen_enhance_frames(det, gen, par, big),
                              "gpen_super_resolve": lambda: pipeline.gpen_super_resolve(nets[32], small)}, a.rounds, 3))
    finally:
        pipeline.gpen_detect_faces = real_detect
    for k, v in s.items():
        print(f"  {k} per frame (256^2 -> 1024^2, one face): median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}", flush=True)
    doc["cases"]["face_enhancement 256 x4"] = s
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_gpen_sr", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
