"""Row f23 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round: ``pipeline.codeformer_enhance``
(CodeFormer at the caller's configuration, then the tiled Real-ESRGAN x2 step with a 23-block x4plus-shaped network, seeded weights) against the same steps on
stock PyTorch float32 on the same card — the mirror modules, the mirror ``GpenSRNet`` per tile, torch ops for the ends:

* the whole of ``codeformer_enhance`` and the Real-ESRGAN step alone (``ops.esrgan_enhance`` on a restored face made beforehand) at ``[1, 3, 512, 512]`` and
  ``[--batch, 3, 512, 512]`` (8 by default);
* ``tile=400`` (the reference's 2 x 2 tiles of 440 x 440: 592^2 pixels' worth of convolution) against ``tile=0`` (512^2) at batch 1;
* ``ops.cv_resize_lanczos4`` alone at ``[8, 2048, 2048, 3] -> 1024 x 1024``: time, and bytes per second over the 15.7 MB a face must move, beside a device copy
  of as many bytes;
* the device time of every entry point of one native Real-ESRGAN step, each timed alone.

    python tools/time_esrgan_tile.py [--batch 8] [--rounds 3] [--blocks 23] [--lanczos-only] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The stock Lanczos stand-in is the
2 : 1 case alone (one coefficient set): two strided depthwise convolutions in float32 over a replicate pad, rounded once — stock PyTorch has no fixed-point
equivalent, so it stands for the step's cost, not its bits."""
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

from e4s2024_amd import ops, pipeline, seeded
from time_generator_front import trace
from time_reenact import show
from time_resunet import alternate

dev = "cuda:0"
SEED, W = 21, 0.8
HALF_TAPS = (-26, 122, -340, 1267, 1267, -340, 122, -26)


def torch_lanczos_half(u8):
    """The 2 : 1 shrink on stock PyTorch: uint8 [bs, H, W, 3] -> uint8 [bs, H / 2, W / 2, 3] (float32; the cost of the step, not its bits)."""
    x = u8.permute(0, 3, 1, 2).float()
    k = torch.tensor(HALF_TAPS, dtype=torch.float32, device=u8.device) / 2048
    x = F.conv2d(F.pad(x, (3, 3, 0, 0), mode="replicate"), k.view(1, 1, 1, 8).expand(3, 1, 1, 8), stride=(1, 2), groups=3)
    x = F.conv2d(F.pad(x, (0, 0, 3, 3), mode="replicate"), k.view(1, 1, 8, 1).expand(3, 1, 8, 1), stride=(2, 1), groups=3)
    return x.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def torch_enhance(esr, restored, tile, tile_pad=40):
    """``RealESRGANer.enhance(outscale=2)`` on stock PyTorch: uint8 [bs, 3, H, W] -> uint8 [bs, 2H, 2W, 3]."""
    x = restored.float() / 255
    bs, _, H, Wd = x.shape
    out = x.new_zeros((bs, 3, 4 * H, 4 * Wd))
    for (y0, y1, x0, x1), (oy0, oy1, ox0, ox1), (Y0, X0) in ops.esrgan_tiles(H, Wd, tile, tile_pad):
        out[:, :, Y0:Y0 + oy1 - oy0, X0:X0 + ox1 - ox0] = esr(x[:, :, y0:y1, x0:x1])[:, :, oy0:oy1, ox0:ox1]
    big = (out.clamp_(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return torch_lanczos_half(big)


def torch_codeformer_enhance(cf, esr, faces):
    x = ((faces.float() / 255.0) - 0.5) / 0.5
    out = cf(x, w=W, adain=True)[0]
    restored = (((out.clamp(-1, 1) + 1) / 2) * 255).round().to(torch.uint8)
    return torch_enhance(esr, restored, 400)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--json", default=None)
    ap.add_argument("--lanczos-only", action="store_true", help="the resize kernel alone")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "blocks": a.blocks, "cases": {}}
    print(f"CodeFormer restoration with the tiled Real-ESRGAN x2 step ({a.blocks} blocks, num_feat 64), 512 x 512, w = {W}, {doc['device']}")
    cf = ops.CodeFormer().eval()
    cf.load_state_dict(seeded.seeded_codeformer_state_dict(SEED), strict=True)
    cf = cf.to(dev)
    esr = ops.GpenSRNet(a.blocks, 64, 4).eval()
    esr.load_state_dict(seeded.seeded_gpen_sr_state_dict(SEED, a.blocks, 64, 4), strict=True)
    esr = esr.to(dev)
    base = torch.from_numpy(seeded.seeded_array(SEED, "f23.faces", (1, 3, 512, 512), 127.5, 60.0, "normal").clip(0, 255).astype("uint8")).to(dev)

    # the Lanczos kernel alone
    big = torch.randint(0, 256, (8, 2048, 2048, 3), dtype=torch.uint8, device=dev)
    nbytes = 8 * (2048 * 2048 * 3 + 1024 * 1024 * 3)
    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    res = alternate({"hip": lambda: ops.cv_resize_lanczos4(big, (1024, 1024)), "copy": lambda: dst.copy_(src), "torch": lambda: torch_lanczos_half(big)}, a.rounds, 5)
    show(doc, "lanczos4 [8, 2048, 2048, 3] -> 1024 x 1024", res)
    med = doc["cases"]["lanczos4 [8, 2048, 2048, 3] -> 1024 x 1024"]
    for k in ("hip", "copy"):
        print(f"  {k}: {nbytes / 1e6:.1f} MB in {med[k]['median_ms']:.3f} ms = {nbytes / med[k]['median_ms'] / 1e9:.2f} TB/s ({nbytes / 8 / 1e6:.1f} MB a face)", flush=True)
    doc["lanczos_bytes"] = nbytes
    del big, src, dst

    for bs in ([] if a.lanczos_only else sorted({1, a.batch})):
        faces = torch.cat([base.roll(17 * i, 3) for i in range(bs)]).contiguous()
        restored = pipeline.codeformer_restore(cf, faces, w=W)
        got, want = ops.esrgan_enhance(restored, esr, outscale=2, chw=True), torch_enhance(esr, restored, 400)
        diff = (got.int() - want.int()).abs()
        print(f"  batch {bs}: the native step against stock float32: {100 * float((diff <= 1).float().mean()):.2f} % of the bytes within one grey level, "
              f"{int(diff.max())} at the most; image std {float(got.float().std()):.1f}", flush=True)
        reps = 2 if bs == 1 else 1
        res = alternate({"hip": lambda: ops.esrgan_enhance(restored, esr, outscale=2, chw=True), "torch": lambda: torch_enhance(esr, restored, 400)}, a.rounds, reps)
        show(doc, f"esrgan_enhance tile 400 batch {bs}", res)
        res = alternate({"hip": lambda: pipeline.codeformer_enhance(cf, esr, faces, w=W), "torch": lambda: torch_codeformer_enhance(cf, esr, faces)}, a.rounds, reps)
        show(doc, f"codeformer_enhance batch {bs}", res)
        if bs == 1:
            res = alternate({"hip": lambda: ops.esrgan_enhance(restored, esr, outscale=2, chw=True, tile=0), "torch": lambda: torch_enhance(esr, restored, 0)}, a.rounds, reps)
            show(doc, "esrgan_enhance tile 0 batch 1", res)
            t400, t0 = doc["cases"]["esrgan_enhance tile 400 batch 1"]["hip"]["median_ms"], doc["cases"]["esrgan_enhance tile 0 batch 1"]["hip"]["median_ms"]
            print(f"  tile 400 / tile 0 = {t400 / t0:.3f} (592^2 / 512^2 = {592 * 592 / 512 / 512:.3f} in convolved pixels)", flush=True)
            stages = trace(lambda: ops.esrgan_enhance(restored, esr, outscale=2, chw=True))
            total = sum(sum(ms) for ms in stages.values())
            for name, ms in sorted(stages.items(), key=lambda kv: -sum(kv[1])):
                print(f"  trace batch 1 {name:28s} {len(ms):5d} calls  {sum(ms):9.3f} ms = {100 * sum(ms) / total:5.1f} %", flush=True)
            doc["trace_ms"] = {k: [len(v), sum(v)] for k, v in stages.items()}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_esrgan_tile", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
