"""Row f5 measurement: ``ops.crop_align`` and ``ops.paste_into_frames`` per frame at 1920x1080 and 3840x2160, batch 8, next to Pillow's
host route for the same frames (``crop_image``'s crop + QUAD transform, and the PERSPECTIVE transform + alpha_composite of the paste)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from e4s2024_amd import align, ops

dev = "cuda:0"
BS, S, N = 8, 1024, 20


def gpu_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(N):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / N


def quads(h, w, half, rng):
    out = []
    for _ in range(BS):
        cx, cy, ang = w / 2 + rng.uniform(-w / 8, w / 8), h / 2 + rng.uniform(-h / 8, h / 8), rng.uniform(-0.3, 0.3)
        x = np.array([np.cos(ang), np.sin(ang)]) * half
        y = np.flipud(x) * [-1, 1]
        c = np.array([cx, cy])
        out.append(np.stack([c - x - y, c - x + y, c + x + y, c + x - y]))
    return np.stack(out)


def main():
    try:
        from PIL import Image
    except ImportError:
        Image = None
    rng = np.random.default_rng(0)
    for (h, w), half in (((1080, 1920), 300.0), ((2160, 3840), 600.0)):
        plan = align.crop_plan(quads(h, w, half, rng), (h, w), S).to(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        frames = torch.randint(0, 256, (BS, h, w, 3), device=dev, generator=g, dtype=torch.uint8)
        faces = torch.randint(0, 256, (BS, S, S, 3), device=dev, generator=g, dtype=torch.uint8)
        work = frames.clone()
        crop_ms = gpu_ms(lambda: ops.crop_align(frames, plan))
        paste_ms = gpu_ms(lambda: ops.paste_into_frames(faces, work, plan, out=work))
        copy_ms = gpu_ms(lambda: ops.paste_into_frames(faces, frames, plan, out=work))
        box = plan.paste_boxes.numpy()
        area = float(((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).mean())
        line = (f"{w}x{h} batch {BS}: crop_align {crop_ms / BS * 1e3:.1f} us/frame ({S * S * 3 * 2 / (crop_ms / BS * 1e-3) / 1e9:.0f} GB/s of "
                f"crop bytes x2), paste in place {paste_ms / BS * 1e3:.1f} us/frame (box {area / 1e6:.2f} Mpx), paste out of place "
                f"{copy_ms / BS * 1e3:.1f} us/frame")
        if Image is not None:
            fr, fa = frames[:2].cpu().numpy(), faces[:2].cpu().numpy()
            t0 = time.perf_counter()
            for i in range(2):
                img = Image.fromarray(fr[i])
                x0, y0, x1, y1 = plan.boxes[i].tolist()
                img.crop((x0, y0, x1, y1)).transform((S, S), Image.QUAD, (plan.quads[i] - [x0, y0] + 0.5).flatten(), Image.BILINEAR)
            t1 = time.perf_counter()
            for i in range(2):
                base = Image.fromarray(fr[i]).convert("RGBA")
                base.alpha_composite(Image.fromarray(fa[i]).convert("RGBA").transform(base.size, Image.PERSPECTIVE, tuple(plan.inv_coeffs[i].cpu().numpy()), Image.BILINEAR))
                base.convert("RGB")
            t2 = time.perf_counter()
            line += f"; Pillow on the host: crop {(t1 - t0) / 2 * 1e3:.1f} ms/frame, paste {(t2 - t1) / 2 * 1e3:.1f} ms/frame"
        print(line, flush=True)


if __name__ == "__main__":
    main()
