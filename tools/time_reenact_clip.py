"""Row f24 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.sk_resize`` at ``[8, 1024, 1024, 3] -> 256 x 256`` beside a device copy of the bytes it must move and beside the stock-PyTorch composition on the same
  card (a reflect pad, two depthwise ``F.conv2d`` with the 13 Gaussian taps, ``F.interpolate(bilinear)``: float32, the cost of the step, not its bits);
* ``ops.frames_u8`` at ``[8, 3, 256, 256]`` beside ``(pred * 255).to(uint8)`` with the transpose;
* the stages of ``pipeline.reenact_drivens`` and ``pipeline.reenact_recolor_clip`` at the reference's configuration (source and targets 1024 x 1024, size 256,
  every network at its upstream shape with seeded weights), each stage timed alone on the inputs the chain hands it, and the whole calls.

    python tools/time_reenact_clip.py [--frames 2] [--rounds 3] [--kernels-only] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The GPEN stage depends on what the
detector finds, and a seeded detector finds what its random class heads say (750 boxes a frame): its class heads are zeroed here, so it runs at its full cost
and finds no face, ``gpen_face_enhancement`` is the detector, the RealESRNet pass and the frame's resize, and what ONE detected face adds (the warp, the
generator at 512 x 512, the mask and the paste) is timed beside it on one crop, as tools/time_gpen_frame.py times it in full."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import torch.nn.functional as F

import e4s2024_amd
from e4s2024_amd import ops, pipeline, seeded
from time_reenact import seeded_net, show
from time_resunet import alternate

dev = "cuda:0"
SEED, W = 24, 0.8


def torch_sk_resize(u8, size, taps):
    """The 4 : 1 case on stock PyTorch in float32: uint8 [bs, H, W, 3] -> float32 [bs, 3, size, size]."""
    x = u8.permute(0, 3, 1, 2).float() / 255
    r = taps.numel() // 2
    x = F.conv2d(F.pad(x, (0, 0, r, r), mode="reflect"), taps.view(1, 1, -1, 1).expand(3, 1, -1, 1), groups=3)
    x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="reflect"), taps.view(1, 1, 1, -1).expand(3, 1, 1, -1), groups=3)
    return F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)


def networks():
    gen = ops.OcclusionAwareSPADEGenerator().eval()
    template = {k: torch.empty(s, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32, device="meta")
                for k, s in ops.generator_state_dict_shapes().items()}
    gen.load_state_dict(seeded.seeded_generator_state_dict(template, SEED), strict=True)
    kp, he = seeded_net(ops.KPDetector, seeded.seeded_kp_detector_state_dict), seeded_net(ops.HEEstimator, seeded.seeded_he_estimator_state_dict)
    det = ops.RetinaFace().eval()
    sd = seeded.seeded_retinaface_state_dict(0)
    for k in sd:                                                                               # seeded class heads call 750 boxes a frame faces: zeroed, every
        if k.startswith("ClassHead."):                                                         # score is 0.5 and the detector, at its full cost, finds none
            sd[k] = torch.zeros_like(sd[k])
    det.load_state_dict(sd, strict=True)
    gpen = ops.GPEN(512).eval()
    gpen.load_state_dict(seeded.seeded_gpen_state_dict(0, 512), strict=True)
    par = ops.ParseNet().eval()
    with torch.device("meta"):
        t = ops.ParseNet().state_dict()
    par.load_state_dict(seeded.seeded_parsenet_state_dict(t, 0), strict=True)
    sr = ops.GpenSRNet(23, 32, 4).eval()                                                       # realesrnet_x4: 32 features, 23 blocks
    sr.load_state_dict(seeded.seeded_gpen_sr_state_dict(SEED, 23, 32, 4), strict=True)
    return [m.to(dev) for m in (gen, kp, he, det, gpen, par, sr)]


def recolor_networks():
    e4s2024_amd.install()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    parser = FaceParser(None, device=dev)
    seeded.apply_seeded(parser.seg, 7, "bisenet")
    parser.seg.eval()
    blender = ops.BlenderNet().eval()
    blender.referencer.FPN.load_state_dict(seeded.seeded_fpn_state_dict(22))
    blender.unet.load_state_dict(seeded.seeded_resunet_state_dict(21, 64))
    cf = ops.CodeFormer().eval()
    cf.load_state_dict(seeded.seeded_codeformer_state_dict(SEED), strict=True)
    esr = ops.GpenSRNet(23, 64, 4).eval()
    esr.load_state_dict(seeded.seeded_gpen_sr_state_dict(SEED, 23, 64, 4), strict=True)
    return parser, blender.to(dev), cf.to(dev), esr.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="the two kernels alone")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "frames": a.frames, "cases": {}}
    print(f"whole-clip reenactment chain, source and targets 1024 x 1024, size 256, {doc['device']}")

    # the resize kernel alone
    big = torch.randint(0, 256, (8, 1024, 1024, 3), dtype=torch.uint8, device=dev)
    taps = torch.exp(-0.5 / 1.5 ** 2 * torch.arange(-6, 7, dtype=torch.float32, device=dev) ** 2)      # sigma (4 - 1) / 2, radius int(4 sigma + 0.5)
    taps = taps / taps.sum()
    nbytes = 8 * (1024 * 1024 * 3 + 256 * 256 * 3 * 4)
    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    got, stock = ops.sk_resize(big, (256, 256)), torch_sk_resize(big, 256, taps)
    print(f"  sk_resize against the stock float32 composition: {float((got - stock).abs().max()):.2e} at the most (the stock form is not the rule at the borders)")
    name = "sk_resize [8, 1024, 1024, 3] -> 256 x 256"
    show(doc, name, alternate({"hip": lambda: ops.sk_resize(big, (256, 256)), "copy": lambda: dst.copy_(src), "torch": lambda: torch_sk_resize(big, 256, taps)},
                              a.rounds, 10))
    for k in ("hip", "copy"):
        ms = doc["cases"][name][k]["median_ms"]
        print(f"  {k}: {nbytes / 1e6:.1f} MB in {ms:.3f} ms = {nbytes / ms / 1e9:.2f} TB/s ({nbytes / 8 / 1e6:.2f} MB a frame)", flush=True)
    pred = torch.rand((8, 3, 256, 256), device=dev)
    assert torch.equal(ops.frames_u8(pred), (pred * 255).to(torch.uint8).permute(0, 2, 3, 1))
    show(doc, "frames_u8 [8, 3, 256, 256]", alternate({"hip": lambda: ops.frames_u8(pred), "torch": lambda: (pred * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()},
                                                       a.rounds, 20))
    del big, src, dst

    if not a.kernels_only:
        n = a.frames
        gen, kp, he, det, gpen, par, sr = networks()
        parser, blender, cf, esr = recolor_networks()
        source_u8 = ops.tensor2im_u8(seeded.seeded_image(31, 1, 1024).to(dev))
        targets_u8 = torch.cat([ops.tensor2im_u8(seeded.seeded_image(40 + i, 1, 1024).to(dev)) for i in range(n)])
        both = torch.cat((source_u8, targets_u8))
        x = ops.sk_resize(both, (256, 256))
        source, driving = x[:1].contiguous(), x[1:].contiguous()
        pred = pipeline.reenact_clip(gen, kp, he, source, driving)
        frames = ops.frames_u8(pred, flip=True)
        per_frame = pipeline.gpen_detect_faces(det, ops.cv_resize_linear(frames, (1024, 1024)), bgr=False)
        print(f"  faces per frame found by the seeded detector: {[int(d.shape[0]) for d, _ in per_frame]}", flush=True)
        Dr = pipeline.gpen_face_enhancement(det, gpen, par, sr, frames)
        D = Dr.flip(3)
        face = ops.cv_resize_linear(frames, (512, 512))[:1].expand(n, -1, -1, -1).contiguous()  # n crops, so that the per-frame division holds: one face a frame
        stages = {
            "sk_resize (source + targets)": lambda: ops.sk_resize(both, (256, 256)),
            "reenact_clip": lambda: pipeline.reenact_clip(gen, kp, he, source, driving),
            "frames_u8": lambda: ops.frames_u8(pred, flip=True),
            "gpen_face_enhancement": lambda: pipeline.gpen_face_enhancement(det, gpen, par, sr, frames),
            "  of it gpen_super_resolve (RRDB x4, 32 features)": lambda: pipeline.gpen_super_resolve(sr, frames),
            "  beside it, per detected face: gpen_enhance + gpen_face_mask at 512 x 512": lambda: pipeline.gpen_face_mask(par, pipeline.gpen_enhance(gpen, face)),
            "channel reversal of D (a pass of its own)": lambda: Dr.flip(3),
            "recolor_frames": lambda: pipeline.recolor_frames(parser, blender, cf, esr, D, targets_u8, True, W),
            "  of it esrgan_enhance (RRDB x4, 64 features, 2 x 2 tiles)": lambda: ops.esrgan_enhance(D[:, ::2, ::2].permute(0, 3, 1, 2).contiguous(), esr, outscale=2,
                                                                                                   chw=True),
        }
        print(f"  per-stage split, {n} frames (ms per FRAME; the source's share of the first two stages is in them):")
        for nm, fn in stages.items():
            res = {"hip": [t / n for t in alternate({"hip": fn}, a.rounds, 1)["hip"]]}
            show(doc, f"stage {nm.strip()}", res)
        nets = (gen, kp, he, det, gpen, par, sr)
        whole = {"reenact_drivens": lambda: pipeline.reenact_drivens(*nets, source_u8, targets_u8),
                 "reenact_recolor_clip": lambda: pipeline.reenact_recolor_clip(*nets, parser, blender, cf, esr, source_u8, targets_u8, flip_target=True, w=W)}
        for nm, fn in whole.items():
            res = {"hip": [t / n for t in alternate({"hip": fn}, a.rounds, 1)["hip"]]}
            show(doc, f"whole {nm}", res)
        c = doc["cases"]
        total = c["whole reenact_recolor_clip"]["hip"]["median_ms"]
        for nm in ("stage of it gpen_super_resolve (RRDB x4, 32 features)", "stage of it esrgan_enhance (RRDB x4, 64 features, 2 x 2 tiles)", "stage reenact_clip"):
            print(f"  {nm}: {100 * c[nm]['hip']['median_ms'] / total:.1f} % of reenact_recolor_clip", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_reenact_clip", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
