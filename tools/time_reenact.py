"""Row f17 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round: the upstream vox-256
configuration at 256 x 256, seeded weights, against the mirror modules run by stock PyTorch on the same device with the same weights:

* ``ops.he_estimator_forward`` plus ``ops.keypoint_transformation`` on a batch of driving frames: the per-frame cost of this stage;
* ``ops.kp_detector_forward`` on the source: once per clip;
* ``ops.reenact_keypoints`` on a clip of ``--frames`` driving frames, eager and replayed from a captured graph.

    python tools/time_reenact.py [--frames 8] [--rounds 5] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The convolution work of the five
``UpBlock3d`` is counted from the layer shapes and printed with the rate it gives."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import vid2vid_kp_model as M
from e4s2024_amd import ops, seeded
from time_resunet import alternate, graphed

dev = "cuda:0"


def seeded_net(cls, fn):
    net = cls().eval()
    with torch.device("meta"):
        template = cls().state_dict()
    net.load_state_dict(fn(template, M.WEIGHT_SEED), strict=True)
    return net.to(dev)


def up_blocks_flop(structure, H, W):
    """Multiply-adds x 2 of the UpBlock3d convolutions of one image, from the layer shapes."""
    _, down, depth, up, _, _, _, _ = structure
    D, h, w = ops.kp_volume_size(structure, H, W)
    h, w = h >> len(up), w >> len(up)
    total, cin = 0, down[-1]
    for c in up:
        h, w = 2 * h, 2 * w
        total += 2 * 27 * cin * c * D * h * w
        cin = c
    return total


def stock_transform(kp, he):
    """``keypoint_transformation`` of drive_demo.py:135-180 as stock tensor operations on the device (the tests' model supplies the rotation)."""
    idx = torch.arange(M.NUM_BINS, dtype=torch.float32, device=he["yaw"].device)
    deg = [(torch.softmax(he[k], 1) * idx).sum(1) * 3 - 99 for k in ("yaw", "pitch", "roll")]
    rot = M.rotation(*deg)
    bs = rot.shape[0]
    return torch.einsum("bmp,bkp->bkm", rot, kp["value"].expand(bs, -1, -1)) + he["t"].unsqueeze(1) + he["exp"].view(bs, -1, 3)


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def show(doc, name, res, note=""):
    s = spread(res)
    for k, v in s.items():
        print(f"  {name} {k:6s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}{note}", flush=True)
    if "hip" in res and "torch" in res:
        faster = max(res["hip"]) < min(res["torch"])
        print(f"  {name}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch round: {faster}", flush=True)
        s["hip_faster_beyond_spread"] = faster
    doc["cases"][name] = s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "frames": a.frames, "cases": {}}
    print(f"face-vid2vid keypoints and head pose at the upstream configuration, 256 x 256, {doc['device']}")
    kp_net = seeded_net(ops.KPDetector, seeded.seeded_kp_detector_state_dict)
    he_net = seeded_net(ops.HEEstimator, seeded.seeded_he_estimator_state_dict)
    frames = torch.from_numpy(M.to_float(M.images_u8(1, a.frames + 1, 256, 256))).to(dev)
    source, driving = frames[:1].contiguous(), frames[1:].contiguous()

    kp = ops.kp_detector_forward(source, kp_net)
    want = kp_net(source)
    print(f"  kp_detector_forward against the mirror on stock PyTorch: {float((kp['value'] - want['value']).abs().max()):.2e} on the keypoints", flush=True)
    gflop = up_blocks_flop(kp_net.structure, 256, 256) / 1e9
    res = alternate({"hip": lambda: ops.kp_detector_forward(source, kp_net), "torch": lambda: kp_net(source)}, a.rounds, 3)
    show(doc, "KPDetector batch 1", res, f"   ({gflop:.1f} GFLOP counted in the five UpBlock3d)")

    for bs in sorted({1, a.frames}):
        x = driving[:bs].contiguous()
        got, ref = ops.he_estimator_forward(x, he_net), he_net(x)
        off = max(float((got[k] - ref[k]).abs().max()) for k in got)
        print(f"  he_estimator_forward batch {bs} against the mirror on stock PyTorch: {off:.2e} on the heads", flush=True)
        res = alternate({"hip": lambda: ops.keypoint_transformation(kp, ops.he_estimator_forward(x, he_net), False),
                         "torch": lambda: stock_transform(kp, he_net(x))}, a.rounds, 3)
        show(doc, f"HEEstimator + transformation batch {bs}", res)

    replay = graphed(lambda: ops.reenact_keypoints(source, driving, kp_net, he_net))
    show(doc, f"reenact_keypoints {a.frames} frames", alternate({"eager": lambda: ops.reenact_keypoints(source, driving, kp_net, he_net), "graph": replay}, a.rounds, 3))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_reenact", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
