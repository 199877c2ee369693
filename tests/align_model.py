"""Numpy model of the Pillow operations behind the crop-align and paste-into-frame path (``align.py``, ``csrc/align.hip``), so that the GPU
tests do not need Pillow on the GPU machine.  ``tests/test_align_cpu.py`` pins the model against Pillow itself, byte for byte.

Pillow's rules (src/libImaging/Geometry.c, bilinear filter on 8-bit RGB): output pixel (x, y) is sampled at (x + 0.5, y + 0.5) mapped through
the transform in double arithmetic; a sample outside [0, w) x [0, h) of the source is not taken; otherwise, with xi -= 0.5, yi -= 0.5, the
two columns floor(xi), floor(xi) + 1 are clamped, the row floor(yi) is clamped, the row below is used only inside the source (else the first
row's value), v = lerp(lerp(p00, p01, dx), lerp(p10, p11, dx), dy) and the byte is the truncated v."""
import numpy as np


def sample_bilinear(src: np.ndarray, xi: np.ndarray, yi: np.ndarray):
    """``src`` uint8 [h, w, 3]; ``xi``, ``yi`` float64 of one shape -> (uint8 [..., 3] samples, bool [...] taken)."""
    h, w = src.shape[:2]
    ok = (xi >= 0.0) & (xi < w) & (yi >= 0.0) & (yi < h)
    px = np.zeros(xi.shape + (3,), dtype=np.uint8)
    if h == 0 or w == 0 or not ok.any():
        return px, ok
    xs, ys = xi[ok] - 0.5, yi[ok] - 0.5
    xf, yf = np.floor(xs), np.floor(ys)
    dx, dy = (xs - xf)[:, None], (ys - yf)[:, None]
    x, y = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
    yc = np.clip(y, 0, h - 1)
    second = (y + 1 >= 0) & (y + 1 < h)
    y1 = np.where(second, y + 1, yc)
    s = src.astype(np.int64)
    a0, b0, a1, b1 = s[yc, x0], s[yc, x1], s[y1, x0], s[y1, x1]
    v1 = a0 + (b0 - a0) * dx
    v2 = np.where(second[:, None], a1 + (b1 - a1) * dx, v1)
    v = v1 + (v2 - v1) * dy
    px[ok] = v.astype(np.int64).astype(np.uint8)
    return px, ok


def warp_quad(src: np.ndarray, coeffs, size: int, rows_per_chunk: int = 256) -> np.ndarray:
    """``Image.fromarray(src).transform((size, size), QUAD, data, BILINEAR)`` given Pillow's 8 derived coefficients; fill 0."""
    a0, a1, a2, a3, a4, a5, a6, a7 = (float(v) for v in coeffs)
    out = np.zeros((size, size, 3), dtype=np.uint8)
    xin = np.arange(size, dtype=np.float64)[None, :] + 0.5
    for r in range(0, size, rows_per_chunk):
        yin = np.arange(r, min(r + rows_per_chunk, size), dtype=np.float64)[:, None] + 0.5
        xi = a0 + a1 * xin + a2 * yin + a3 * xin * yin
        yi = a4 + a5 * xin + a6 * yin + a7 * xin * yin
        out[r:r + yin.shape[0]] = sample_bilinear(src, xi, yi)[0]
    return out


def paste_perspective(face: np.ndarray, frame: np.ndarray, coeffs, rows_per_chunk: int = 256) -> np.ndarray:
    """``frame`` with ``Image.fromarray(face).convert('RGBA').transform(frame.size, PERSPECTIVE, coeffs, BILINEAR)`` alpha-composited over it:
    every pixel that samples the opaque face takes the sample, every other keeps the frame's value."""
    a0, a1, a2, a3, a4, a5, a6, a7 = (float(v) for v in coeffs)
    h, w = frame.shape[:2]
    out = frame.copy()
    xin = np.arange(w, dtype=np.float64)[None, :] + 0.5
    for r in range(0, h, rows_per_chunk):
        yin = np.arange(r, min(r + rows_per_chunk, h), dtype=np.float64)[:, None] + 0.5
        den = a6 * xin + a7 * yin + 1
        xi = (a0 * xin + a1 * yin + a2) / den
        yi = (a3 * xin + a4 * yin + a5) / den
        px, ok = sample_bilinear(face, xi, yi)
        blk = out[r:r + yin.shape[0]]
        blk[ok] = px[ok]
    return out


def resample_pass(img: np.ndarray, xmin, cnt, kk, out_size: int, axis: int) -> np.ndarray:
    """One pass of Pillow's 8-bit resampler over uint8 [h, w, c] (axis 1 = width, 0 = height) from the host tables
    (``ops_post._pil_resample_tables``): clip8((2^21 + sum_j k[o][j] * in[xmin[o] + j]) >> 22)."""
    xmin, cnt, kk = (np.asarray(t, dtype=np.int32) for t in (xmin, cnt, kk))
    src = np.moveaxis(img, axis, 0).astype(np.int32)                       # [in, other, c]; int32 sums like the library's
    acc = np.full((out_size,) + src.shape[1:], 1 << 21, dtype=np.int32)
    n_in = src.shape[0]
    for j in range(kk.shape[1]):
        live = j < cnt
        idx = np.clip(xmin + j, 0, n_in - 1)
        acc += np.where(live, kk[:, j], 0)[:, None, None] * src[idx]
    acc = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.moveaxis(acc, 0, axis))


def pil_resize(img: np.ndarray, size, resample: str = "bicubic") -> np.ndarray:
    """``Image.resize(size, filter)`` of uint8 [h, w, c]: width pass, then height pass (Pillow's order)."""
    from e4s2024_amd import ops          # (ops first: it imports ops_post)
    wd, ht = int(size[0]), int(size[1])
    out = img
    for axis, target in ((1, wd), (0, ht)):
        n_in = out.shape[axis]
        if target == n_in:
            continue
        xmin, cnt, kk, _ = ops._pil_resample_tables(n_in, target, "cpu", resample)
        out = resample_pass(out, xmin.numpy(), cnt.numpy(), kk.numpy(), target, axis)
    return out


def crop_align(frame: np.ndarray, plan, i: int) -> np.ndarray:
    """Frame ``i``'s crop under ``plan`` (``align.CropPlan``): the Lanczos shrink, the source window, the QUAD warp."""
    src = frame
    if int(plan.shrink[i]) > 1:
        src = pil_resize(frame, tuple(int(v) for v in plan.resized_wh[i]), "lanczos")
    x0, y0, x1, y1 = (int(v) for v in plan.boxes[i])
    return warp_quad(src[y0:y1, x0:x1], plan.quad_coeffs[i].cpu().numpy(), plan.output_size)


def paste(face: np.ndarray, frame: np.ndarray, plan, i: int) -> np.ndarray:
    return paste_perspective(face, frame, plan.inv_coeffs[i].cpu().numpy())


# ------------------------------------------------------------------------------------------------ Pillow itself (host tests only)
def pil_crop_image(frame: np.ndarray, quad: np.ndarray, size: int) -> np.ndarray:
    """What the reference's ``crop_image(frame, size, quad)`` does with Pillow (no padding), restated; the shrink uses LANCZOS (the filter
    Pillow < 10 called ANTIALIAS)."""
    from PIL import Image
    img = Image.fromarray(frame)
    quad = np.array(quad, dtype=np.float64)
    qsize = np.hypot(*((quad[3] - quad[1]) / 2)) * 2
    shrink = int(np.floor(qsize / size * 0.5))
    if shrink > 1:
        img = img.resize((int(np.rint(float(img.size[0]) / shrink)), int(np.rint(float(img.size[1]) / shrink))), Image.LANCZOS)
        quad /= shrink
        qsize /= shrink
    border = max(int(np.rint(qsize * 0.1)), 3)
    box = (int(np.floor(quad[:, 0].min())), int(np.floor(quad[:, 1].min())), int(np.ceil(quad[:, 0].max())), int(np.ceil(quad[:, 1].max())))
    box = (max(box[0] - border, 0), max(box[1] - border, 0), min(box[2] + border, img.size[0]), min(box[3] + border, img.size[1]))
    if box[2] - box[0] < img.size[0] or box[3] - box[1] < img.size[1]:
        img = img.crop(box)
        quad -= box[0:2]
    return np.asarray(img.transform((size, size), Image.QUAD, (quad + 0.5).flatten(), Image.BILINEAR))


def pil_paste(face: np.ndarray, frame: np.ndarray, inv_coeffs) -> np.ndarray:
    """The reference's "op2. paste back": the face as RGBA (alpha 255) warped by PERSPECTIVE into the frame's size, alpha-composited over it."""
    from PIL import Image
    base = Image.fromarray(frame).convert("RGBA")
    layer = Image.fromarray(face).convert("RGBA")
    warped = layer.transform(base.size, Image.PERSPECTIVE, tuple(float(v) for v in inv_coeffs), Image.BILINEAR)
    base.alpha_composite(warped)
    return np.asarray(base.convert("RGB"))


# ------------------------------------------------------------------------------------------------ test inputs
def square_quad(cx, cy, half, angle=0.0):
    """A face square (the kind ``align.quads_from_transforms`` makes) centred at (cx, cy) with half-side ``half``, rotated by ``angle``."""
    x = np.array([np.cos(angle), np.sin(angle)]) * half
    y = np.flipud(x) * [-1, 1]
    c = np.array([cx, cy], dtype=np.float64)
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y])


def make_frame(rng, h, w):
    """uint8 [h, w, 3]: per-pixel noise over smooth gradients (every interpolation weight and every truncation matters)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7) % 256], axis=-1)
    noise = rng.integers(0, 256, size=(h, w, 3))
    return np.where(rng.random((h, w, 1)) < 0.5, base, noise).astype(np.uint8)
