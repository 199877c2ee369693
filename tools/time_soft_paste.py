"""Row f6 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

1. ``ops.soft_erosion`` on [8, 3, 512, 512] and [8, 1, 1024, 1024] against the plain PyTorch composition on the same device (``F.conv2d`` plus the
   boolean-indexed normalisation per plane — its host synchronisations are part of what it costs), configurations (15, 0.6, 1) and (17, 0.9, 7);
2. ``pipeline.paste_back_soft`` per frame at batch 8 against the same chain with that PyTorch composition in place of the kernel;
3. ``pipeline.swap_images`` per image at batch 8 beside ``pipeline.swap_frames``;
and the kernel launches per call (torch.profiler, in a pass of its own).

    python tools/time_soft_paste.py [--rounds 7] [--skip-swap] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import align, ops, pipeline, seeded
from e4s2024_amd.ops_post import _soft_erosion_weights

dev = "cuda:0"
BS = 8


def torch_soft_erosion(x, kernel_size=15, threshold=0.6, iterations=1):
    """SoftErosion.forward with stock PyTorch ops, the maximum per plane (what a user of the image mode runs today)."""
    ch = x.shape[1]
    w = _soft_erosion_weights(kernel_size, x.device).t()[None, None].expand(ch, 1, -1, -1).contiguous()
    pad = kernel_size // 2
    for _ in range(iterations - 1):
        x = torch.min(x, F.conv2d(x, weight=w, groups=ch, padding=pad))
    x = F.conv2d(x, weight=w, groups=ch, padding=pad)
    mask = x >= threshold
    x[mask] = 1.0
    for b in range(x.shape[0]):
        for c in range(ch):
            p, nm = x[b, c], ~mask[b, c]
            p[nm] /= p[nm].max()
    return x, mask


def torch_paste_back_soft(swapped_u8, target_u8, labels, hole, radius=2):
    fg, hard_border, hard_full = ops.foreground_masks(labels, hole, radius)
    s, _ = torch_soft_erosion(torch.cat([hard_full, hard_full - hard_border, fg], dim=1))
    content, border = s[:, 2:3].contiguous(), (s[:, 0:1] - s[:, 1:2]).clamp_(0, 1)
    h, w = swapped_u8.shape[1:3]
    cm = ops.bilinear_resize(content, (h, w), align_corners=False)
    bm = ops.bilinear_resize(border, (h, w), align_corners=False)
    pasted = ops.blend_with_mask(target_u8, swapped_u8, cm, 1.0)
    t = target_u8.permute(0, 3, 1, 2).contiguous()
    return ops.blending(t, pasted.permute(0, 3, 1, 2).float(), bm).permute(0, 2, 3, 1).contiguous()


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
        for _ in range(2):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps))
    return out


def launches(fn):
    """Kernel launches of one call (None where the profiler does not see the device)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as e:  # noqa: BLE001
        print(f"  (launch count not measured: {type(e).__name__}: {e})")
        return None


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def report(title, res, per=1, unit="ms"):
    s = {k: summary(v) for k, v in res.items()}
    for k, v in s.items():
        print(f"  {title} {k:14s}: median {v['median_ms'] / per:9.3f} {unit}   rounds {v['min_ms'] / per:.3f} .. {v['max_ms'] / per:.3f}", flush=True)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-swap", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "soft_erosion": {}, "paste_back_soft": {}, "swap": {}}
    labs = np.concatenate([seeded.facelike_labels(5, BS // 2), seeded.blocky_labels(3, BS // 2)])
    fg512 = torch.from_numpy(np.isin(labs, (0, 11, 4, 7, 8), invert=True).astype(np.float32))[:, None].to(dev)

    print(f"1. soft_erosion, {doc['device']}")
    shapes = {"8x3x512x512": torch.cat([fg512, fg512.flip(-1), fg512.flip(-2)], dim=1).contiguous(),
              "8x1x1024x1024": F.interpolate(fg512, size=(1024, 1024), mode="bilinear", align_corners=True).contiguous()}
    for sname, x in shapes.items():
        for cfg in ((15, 0.6, 1), (17, 0.9, 7)):
            hs, hh = ops.soft_erosion(x, *cfg)
            ts, th = torch_soft_erosion(x.clone(), *cfg)
            agree = {"soft_max_abs": float((hs - ts).abs().max()), "hard_flips": int((hh != th).sum())}
            res = alternate({"hip": lambda: ops.soft_erosion(x, *cfg), "torch": lambda: torch_soft_erosion(x, *cfg)}, a.rounds, 10)
            tag = f"{sname} k{cfg[0]} t{cfg[1]} i{cfg[2]}"
            s = report(tag, res)
            n_hip, n_torch = launches(lambda: ops.soft_erosion(x, *cfg)), launches(lambda: torch_soft_erosion(x, *cfg))
            faster = max(res["hip"]) < min(res["torch"])
            print(f"  {tag}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.1f}x, slowest hip round below fastest torch round: {faster}; "
                  f"launches hip {n_hip} torch {n_torch}; outputs agree to {agree['soft_max_abs']:.1e}, {agree['hard_flips']} hard flips", flush=True)
            doc["soft_erosion"][tag] = {**s, "launches": {"hip": n_hip, "torch": n_torch}, "hip_faster_beyond_spread": faster, **agree}

    print("2. paste_back_soft, batch 8")
    g = torch.Generator(device=dev).manual_seed(0)
    sw = torch.randint(0, 256, (BS, 1024, 1024, 3), device=dev, generator=g, dtype=torch.uint8)
    tg = torch.randint(0, 256, (BS, 1024, 1024, 3), device=dev, generator=g, dtype=torch.uint8)
    lab = torch.from_numpy(labs).to(dev)
    hole = torch.zeros_like(lab)
    hole[:, 320:400, 200:330] = 1
    same = bool(torch.equal(pipeline.paste_back_soft(sw, tg, lab, hole), torch_paste_back_soft(sw, tg, lab, hole)))
    res = alternate({"hip": lambda: pipeline.paste_back_soft(sw, tg, lab, hole), "torch_softer": lambda: torch_paste_back_soft(sw, tg, lab, hole)}, a.rounds, 5)
    s = report("per frame", res, per=BS)
    n_hip, n_torch = launches(lambda: pipeline.paste_back_soft(sw, tg, lab, hole)), launches(lambda: torch_paste_back_soft(sw, tg, lab, hole))
    print(f"  launches per call: hip {n_hip}, torch softer {n_torch}; outputs identical: {same}", flush=True)
    doc["paste_back_soft"] = {**s, "launches": {"hip": n_hip, "torch_softer": n_torch}, "outputs_identical": same, "batch": BS}

    if not a.skip_swap:
        print("3. swap_images beside swap_frames, batch 8, 1920x1080 frames")
        import e4s2024_amd
        e4s2024_amd.install()
        from models.networks import Net3
        from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
        opts = argparse.Namespace(fsencoder_type="psp", remaining_layer_idx=13, num_seg_cls=12, out_size=1024, train_G=False, start_from_latent_avg=True,
                                  learn_in_w=False)
        net = Net3(opts).eval()
        seeded.apply_seeded(net, 4, "net3")
        net.latent_avg = seeded.seeded_latent_avg(2, 18).to(dev)
        net = net.to(dev)
        parser = FaceParser(None, device=dev)
        seeded.apply_seeded(parser.seg, 7, "bisenet")
        parser.seg.eval()
        rng = np.random.default_rng(0)
        h, w = 1080, 1920
        quads = []
        for _ in range(BS):
            c, ang = np.array([w / 2 + rng.uniform(-w / 8, w / 8), h / 2 + rng.uniform(-h / 8, h / 8)]), rng.uniform(-0.3, 0.3)
            x = np.array([np.cos(ang), np.sin(ang)]) * 300.0
            y = np.flipud(x) * [-1, 1]
            quads.append(np.stack([c - x - y, c - x + y, c + x + y, c + x - y]))
        plan = align.crop_plan(np.stack(quads), (h, w), 1024).to(dev)
        frames = torch.randint(0, 256, (BS, h, w, 3), device=dev, generator=g, dtype=torch.uint8)
        driven = seeded.seeded_image(5, BS, 1024).to(dev)
        ops.STRICT_MASK = False
        res = alternate({"swap_images": lambda: pipeline.swap_images(net, parser, driven, frames, plan),
                         "swap_frames": lambda: pipeline.swap_frames(net, parser, driven, frames, plan)}, a.rounds, 3)
        s = report("per image", res, per=BS)
        n_img, n_vid = launches(lambda: pipeline.swap_images(net, parser, driven, frames, plan)), launches(lambda: pipeline.swap_frames(net, parser, driven, frames, plan))
        print(f"  launches per call: swap_images {n_img}, swap_frames {n_vid}", flush=True)
        doc["swap"] = {**s, "launches": {"swap_images": n_img, "swap_frames": n_vid}, "batch": BS}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_soft_paste", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
