"""Row f7 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

1. ``ops.grey_dilate`` on [8, 1, 1024, 1024] at radius 10 (achieved bytes/s: 4 B in + 4 B out per pixel);
2. the statistics + solve + apply trio at batch 8 (``ops.skin_color_transfer``), and the moments and apply kernels alone with their achieved bytes/s
   against the 4.8 TB/s a 1 GiB device copy reaches on this part;
3. ``pipeline.color_transfer`` per image at batch 8;
4. ``pipeline.swap_images(ct_mode='lct')`` per image beside ``swap_images()`` and ``swap_images(recolor_fn=host)``, ``host`` = the numpy restatement
   (``tests/colortransfer_model.py``) with its device -> host -> device copies: the route a user has without this row.

    python tools/time_color_transfer.py [--rounds 7] [--skip-swap] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from e4s2024_amd import align, ops, pipeline, seeded
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

dev = "cuda:0"
BS = 8
HBM_COPY_BYTES_PER_S = 4.8e12


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


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def report(title, res, per=1, nbytes=None):
    s = {k: summary(v) for k, v in res.items()}
    for k, v in s.items():
        line = f"  {title} {k:18s}: median {v['median_ms'] / per:9.4f} ms   rounds {v['min_ms'] / per:.4f} .. {v['max_ms'] / per:.4f}"
        if nbytes and k in nbytes:
            rate = nbytes[k] / (v["median_ms"] * 1e-3)
            v["bytes_per_s"] = rate
            line += f"   {rate / 1e12:.2f} TB/s = {rate / HBM_COPY_BYTES_PER_S:.2f} of a device copy's 4.8 TB/s"
        print(line, flush=True)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-swap", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    import colortransfer_model as CM
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch": BS}
    labs_d = torch.from_numpy(np.concatenate([seeded.facelike_labels(5, BS // 2), seeded.facelike_labels(9, BS // 2)])).to(dev)
    labs_t = torch.from_numpy(np.concatenate([seeded.facelike_labels(6, BS // 2), seeded.facelike_labels(12, BS // 2)])).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    sw = torch.randint(0, 256, (BS, 1024, 1024, 3), device=dev, generator=g, dtype=torch.uint8)
    tg = torch.randint(0, 256, (BS, 1024, 1024, 3), device=dev, generator=g, dtype=torch.uint8)
    lut = torch.zeros(256, device=dev)
    lut[list(pipeline.CT_FACE_CLASSES)] = 1.0
    md = ops.bilinear_resize(lut[labs_d.long()][:, None], (1024, 1024), align_corners=False)
    mt = ops.bilinear_resize(lut[labs_t.long()][:, None], (1024, 1024), align_corners=False)
    px = BS * 1024 * 1024

    print(f"1. grey_dilate [8, 1, 1024, 1024] radius 10, {doc['device']}")
    res = alternate({"grey_dilate": lambda: ops.grey_dilate(md, 10), "grey_erode": lambda: ops.grey_erode(md, 10)}, a.rounds, 20)
    doc["grey_morph"] = report("r=10", res, nbytes={"grey_dilate": 8 * px, "grey_erode": 8 * px})

    print("2. statistics + solve + apply, batch 8")
    nbytes = ctypes.c_int64(0)
    lib().call("e4s_ct_moments_scratch_bytes", BS, 1024, 1024, ctypes.byref(nbytes))
    part = torch.empty((2, nbytes.value // 8), dtype=torch.float64, device=dev)
    coef = ops.color_transfer_coefficients(sw, tg, md, mt, "lct")
    composed = torch.empty((BS, 3, 1024, 1024), device=dev)
    res = alternate({
        "trio_lct": lambda: ops.skin_color_transfer(sw, tg, md, mt, "lct", with_q=False),
        "trio_mkl": lambda: ops.skin_color_transfer(sw, tg, md, mt, "mkl", with_q=False),
        "moments_one_image_set": lambda: lib().call("e4s_ct_moments", _p(part[0]), _p(sw), _p(md), BS, 1024, 1024, _stream()),
        "solve": lambda: lib().call("e4s_ct_solve", _p(coef), _p(part[0]), _p(part[1]), BS, 1024, 1024, 0, _stream()),
        "apply": lambda: lib().call("e4s_ct_apply", _p(composed), None, _p(sw), _p(md), _p(coef), BS, 1024, 1024, _stream()),
    }, a.rounds, 20)
    doc["transfer"] = report("batch 8", res, nbytes={"moments_one_image_set": 7 * px, "apply": (7 + 12) * px})

    print("3. pipeline.color_transfer, batch 8")
    res = alternate({"lct": lambda: pipeline.color_transfer(sw, tg, labs_d, labs_t, "lct"), "mkl": lambda: pipeline.color_transfer(sw, tg, labs_d, labs_t, "mkl")},
                    a.rounds, 5)
    doc["color_transfer"] = report("per image", res, per=BS)

    if not a.skip_swap:
        print("4. swap_images with and without the colour transfer, batch 8, 1920x1080 frames")
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
        # the host route needs the two maps; the seeded parser's maps are arbitrary, so the host model is fed the face-like maps of part 3 (same work per pixel)
        ld_h, lt_h = labs_d.cpu().numpy(), labs_t.cpu().numpy()

        def host(swapped, crops):
            return torch.from_numpy(CM.color_transfer(swapped.cpu().numpy(), crops.cpu().numpy(), ld_h, lt_h, "lct")).to(dev)

        res = alternate({"ct_mode_lct": lambda: pipeline.swap_images(net, parser, driven, frames, plan, ct_mode="lct"),
                         "no_recolor": lambda: pipeline.swap_images(net, parser, driven, frames, plan)}, a.rounds, 3)
        res["recolor_fn_host"] = [timed(lambda: pipeline.swap_images(net, parser, driven, frames, plan, recolor_fn=host), 1) for _ in range(2)]
        doc["swap_images"] = report("per image", res, per=BS)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_color_transfer", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
