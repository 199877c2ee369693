"""Row f15 measurement, one process on the GPU, device events, every shape warmed: ``pipeline.gpen_enhance_frames`` at the production sizes — a 1024 x 1024
frame, the 512 generator, the default ParseNet, the ResNet-50 detector, the reference's constants (101 taps, sigma 11) — with one face and four faces per
frame, at batch 1 and 4:

* the whole call;
* each new kernel on its own (transforms, warp-crop, smooth, feather, paste);
* the three networks on their own (detector, generator, ParseNet mask), and the new kernels' share of the sum.

    python tools/time_gpen_frame.py [--rounds 5] [--iters 5] [--json out.json]
    python tools/time_gpen_frame.py --profile-pass      # a few calls of the new ops at batch 1, four faces, and nothing else: the run to put under
                                                        # rocprofv3 --kernel-trace for the per-kernel times

The seeded detector's detections are arbitrary in number, so the detector runs (and is timed) on the frame and its result is replaced by the wanted number of
synthetic faces: landmarks that are the reference points under a similarity, so that the faces lie inside the frame and overlap.  There is no cv2 here to time
against: no ratio is reported.  Each figure is the median over the rounds with the min .. max of the rounds beside it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from e4s2024_amd import ops, pipeline, seeded

dev = "cuda:0"
SIZE, S = 1024, 512
WARMUP = 3


def faces_of(n, rng):
    """(dets [n, 5], landms [n, 10]) of n overlapping faces inside the frame, about 300 pixels each (not 'small'), scores above the threshold."""
    ref = ops.gpen_reference_points(S)
    dets, landms = [], []
    for i in range(n):
        cx, cy, s, a = 380 + 90 * i, 420 + 60 * (i % 2), 0.55 + 0.05 * i, np.deg2rad(-15 + 10 * i)
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        landms.append((s * (ref - S / 2) @ R.T + [cx, cy] + 0.3 * rng.standard_normal((5, 2))).T.reshape(10))
        half = s * S * 0.4
        dets.append([cx - half, cy - half, cx + half, cy + half, 0.99 - 0.01 * i])
    return torch.tensor(np.array(dets), dtype=torch.float32, device=dev), torch.tensor(np.array(landms), dtype=torch.float32, device=dev)


def timed(fn, iters):
    """Milliseconds per call over ``iters`` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def networks():
    det = ops.RetinaFace().eval()
    det.load_state_dict(seeded.seeded_retinaface_state_dict(0), strict=True)
    gen = ops.GPEN(S).eval()
    gen.load_state_dict(seeded.seeded_gpen_state_dict(0, S), strict=True)
    par = ops.ParseNet().eval()
    with torch.device("meta"):
        template = ops.ParseNet().state_dict()
    par.load_state_dict(seeded.seeded_parsenet_state_dict(template, 0), strict=True)
    return det.to(dev), gen.to(dev), par.to(dev)


def parts(frames, dets, landms, n_per_frame):
    """The new ops as closures over prepared inputs, in the chain's order, for a batch whose every frame has the same faces."""
    bs, D = frames.shape[0], ops.GPEN_PASTE_DEFAULTS
    dets, landms = dets.repeat(bs, 1), landms.repeat(bs, 1)
    fof = torch.arange(bs, dtype=torch.int32, device=dev).repeat_interleave(n_per_frame)
    fb = torch.arange(bs + 1, dtype=torch.int32, device=dev) * n_per_frame
    ref = ops.gpen_reference_points(S)
    T, flags = ops.gpen_face_transforms(dets, landms, ref)
    crops = ops.gpen_warp_crop(frames, fof, T, S)
    rng = torch.Generator(device="cpu").manual_seed(1)
    pm = (torch.rand((dets.shape[0], S // 32, S // 32), generator=rng) < 0.9).to(torch.uint8).mul(255).repeat_interleave(32, 1).repeat_interleave(32, 2).to(dev)
    masks = ops.gpen_mask_feather(pm, D["ksize"], D["sigma"], D["thres"])
    return {
        "transforms": lambda: ops.gpen_face_transforms(dets, landms, ref),
        "warp_crop": lambda: ops.gpen_warp_crop(frames, fof, T, S),
        "smooth": lambda: ops.gpen_smooth_small(crops, flags | ops.GPEN_FACE_SMALL),
        "feather": lambda: ops.gpen_mask_feather(pm, D["ksize"], D["sigma"], D["thres"]),
        "paste": lambda: ops.gpen_paste(frames, crops, masks, T, flags, fb),
    }, crops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--profile-pass", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    frame = torch.from_numpy(rng.integers(0, 256, (1, SIZE, SIZE, 3), dtype=np.uint8)).to(dev)
    if args.profile_pass:
        dets, landms = faces_of(4, rng)
        p, _ = parts(frame, dets, landms, 4)
        for _ in range(3):
            for fn in p.values():
                fn()
        torch.cuda.synchronize()
        return
    det, gen, par = networks()
    real_detect = pipeline.gpen_detect_faces
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "cases": {}}
    for bs in (1, 4):
        frames = frame.repeat(bs, 1, 1, 1).contiguous()
        for n in (1, 4):
            dets, landms = faces_of(n, rng)

            def detect(net, fr, bgr=True):
                real_detect(net, fr, bgr=bgr)                 # its time is spent; its arbitrary detections are replaced
                return [(dets, landms)] * fr.shape[0]

            pipeline.gpen_detect_faces = detect
            try:
                p, crops = parts(frames, dets, landms, n)
                fns = {"whole": lambda: pipeline.gpen_enhance_frames(det, gen, par, frames),
                       "detector": lambda: real_detect(det, frames, bgr=False),
                       "generator": lambda: pipeline.gpen_enhance(gen, crops),
                       "parsenet": lambda: pipeline.gpen_face_mask(par, crops), **p}
                for fn in fns.values():
                    for _ in range(WARMUP):
                        fn()
                res = {k: [] for k in fns}
                for _ in range(args.rounds):
                    for k, fn in fns.items():
                        res[k].append(timed(fn, args.iters))
            finally:
                pipeline.gpen_detect_faces = real_detect
            case = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}
            new = sum(case[k]["median_ms"] for k in p)
            nets = sum(case[k]["median_ms"] for k in ("detector", "generator", "parsenet"))
            case["new_kernels_ms"], case["networks_ms"], case["new_share"] = new, nets, new / (new + nets)
            doc["cases"][f"bs{bs}_faces{n}"] = case
            print(f"batch {bs}, {n} face(s) per frame:")
            for k in fns:
                c = case[k]
                print(f"  {k:<11} {c['median_ms']:9.3f} ms   ({c['min_ms']:.3f} .. {c['max_ms']:.3f})")
            print(f"  new kernels {new:.3f} ms beside the three networks' {nets:.3f} ms: {100 * new / (new + nets):.1f} % of the sum; the paste at "
                  f"{case['paste']['median_ms'] / case['parsenet']['median_ms']:.3f} of a ParseNet call", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
