"""Row f23: ``RealESRGANer.enhance`` (swap_face_fine/realesrgan_utils.py:69-250) as ``CodeFormerInfer.infer_image`` calls it, restated directly in float64 or
float32 — the tile geometry of ``tile_process``, ``pre_process`` / ``tile_process`` / ``post_process`` around the network of tests/gpen_sr_model.py at scale 4,
the two rounding ends — and ``cv2.resize(..., INTER_LANCZOS4)`` on uint8 in numpy integer arithmetic, with the seeded cases of the tests and single-change mutants
of itself.

    pre      float(v) / 255 (numpy's float32 division) -> [1, 3, H, W], channel order kept -> F.pad(img, (0, pre_pad, 0, pre_pad), 'reflect')
    tiles    ceil(Hp / tile) x ceil(Wp / tile); a tile's input is its tile_size cell grown by tile_pad and clipped to the image; of its x4 output the window
             [(start - start_pad) 4, + cell 4) is kept and put at start 4.  tile <= 0: one network call on the whole image
    post     the crop of 4 pre_pad rows and columns; clamp(0, 1); (x * 255.0).round() on float32 (half to even); uint8
    resize   only if outscale is not None and != 4: to (int(W outscale), int(H outscale)).  Per axis scale = 1.0 / (double(dst) / src),
             f = float((d + 0.5) scale - 0.5), s = floor(f), f -= s in float32 — NOT reset at the borders; eight taps at clamp(s - 3 + k, 0, src - 1);
             coefficients by interpolateLanczos4: f < FLT_EPSILON: (0, 0, 0, 1, 0, 0, 0, 0); otherwise y0 = -(f + 3) pi / 4, s0 = sin y0, c0 = cos y0 in double,
             c[i] = float((cs[i][0] s0 + cs[i][1] c0) / (y_i y_i)), y_i = -(f + 3 - i) pi / 4, a float32 running sum, inv = 1.f / sum, c[i] *= inv; then
             short(rint(c[i] * 2048.f)), no fix-up of the sum to 2048.  h = sum S[x_k] a_k (int32), v = sum h_k b_k (int32), saturate_u8((v + 2^21) >> 22).
             (f + 3 and f + 3 - i are float32 sums, as C forms them from a float and an int; libm's sin / cos through ``math``.)

The tiled network and the rounding end are checked against the reference's own code on the CPU (tests/golden/g33_esrgan_tile.npz).  cv2 is installed nowhere this
project is built or tested, so the resize has never been run against OpenCV: this restatement of OpenCV's portable (non-SIMD) fixed-point path is the pin, as
tests/gpen_sr_model.py pins ``INTER_LINEAR`` and tests/gpen_paste_model.py ``warpAffine``.  OpenCV >= 4.5 replaced the ``f < FLT_EPSILON`` branch of
interpolateLanczos4 by a per-tap guard (a tap whose y_i is below FLT_EPSILON gets 1e30 before the normalisation); after the rounding to 11 bits both give
(0, 0, 0, 2048, 0, 0, 0, 0).

Weights: ``seeded.seeded_gpen_sr_state_dict`` at scale 4 / feat 64, conv_last rescaled per case so that the float64 x4 output on the case has mean 0.5 and standard
deviation 0.25 (``gpen_sr_model.calibrated``).  ``bound`` and the uint8 rule are gpen_sr_model's, never computed from the code under test."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import gpen_sr_model as SM
from gpen_sr_model import MUTANT_MARGIN, bound, check_u8, max_err  # noqa: F401

SCALE = 4
NUM_FEAT = 64
# The seed of the images and of the weights: the first at which the MODEL alone (float32 against float64) passes check_u8 on every golden case and leaves it
# conditioned — >= 99 % strict pixels, < 10 % clamped, a spread over 30 grey levels.  Seed 1, the first tried, does: 99.80 - 99.87 % strict, 1.2 - 2.3 %
# clamped, std 63 (seeds 2 - 8 would do as well: tests/golden/make_golden_esrgan_tile.py --seeds prints the table).
CASE_SEED = 1
# the golden's cases: tag -> (H, W, tile, tile_pad, pre_pad)
GOLDEN_CASES = {
    "11x14.t5.p2": (11, 14, 5, 2, 0),        # 3 x 3 tiles, interior tiles padded on both sides, the last row of tiles one pixel high
    "9x9.t4.p1.pre3": (9, 9, 4, 1, 3),       # pre-pad and its crop
    "6x7.t400.p40": (6, 7, 400, 40, 0),      # one tile, the pad clipped away
    "6x7.t0": (6, 7, 0, 10, 0),              # the untiled branch (tile_pad is not read)
}
GOLDEN_BLOCKS = 1
GOLDEN_OUTSCALES = (2, None, 1.5)
DEEP_CASE = ("deep.b23.8x8.t5.p2", 23, 8, 8, 5, 2, 0)                     # the full depth, on the device tests only
TILE_MUTANTS = ("pad_ignored", "crop_unscaled", "prepad_replicate", "half_up")
LANCZOS_MUTANTS = ("lanczos_no_center", "lanczos_float", "lanczos_sum_fixed", "lanczos_fraction_clamped", "lanczos_antialias")
MUTANTS = TILE_MUTANTS + LANCZOS_MUTANTS
# (H, W, Ho, Wo) of the resize alone: the device test's table and the cases the Lanczos mutants are measured on
RESIZE_CASES = ((16, 16, 8, 8), (9, 13, 5, 7), (7, 5, 15, 12), (8, 8, 8, 8), (1, 1, 3, 3), (20, 3, 10, 9), (64, 48, 32, 24))

_CASE = {}


# ------------------------------------------------------------------------------------------------ tile_process's geometry
def tiles(H, W, tile, tile_pad, mutant=None):
    """Per tile ((y0, y1, x0, x1), (oy0, oy1, ox0, ox1), (Y0, X0)): the padded input window, the kept window of the tile's x4 output, its place in the x4 image;
    rows of tiles first.  ``tile <= 0``: the whole image."""
    if tile <= 0:
        return [((0, H, 0, W), (0, SCALE * H, 0, SCALE * W), (0, 0))]
    pad = 0 if mutant == "pad_ignored" else tile_pad
    k = 1 if mutant == "crop_unscaled" else SCALE
    out = []
    for y in range(math.ceil(H / tile)):
        for x in range(math.ceil(W / tile)):
            sx, sy = x * tile, y * tile
            ex, ey = min(sx + tile, W), min(sy + tile, H)
            sxp, exp_, syp, eyp = max(sx - pad, 0), min(ex + pad, W), max(sy - pad, 0), min(ey + pad, H)
            ox, oy = (sx - sxp) * k, (sy - syp) * k
            out.append(((syp, eyp, sxp, exp_), (oy, oy + (ey - sy) * SCALE, ox, ox + (ex - sx) * SCALE), (sy * SCALE, sx * SCALE)))
    return out


# ------------------------------------------------------------------------------------------------ pre_process, tile_process, post_process
def pre_process(img_u8, pre_pad, dtype=torch.float64, mutant=None):
    """uint8 ``[H, W, 3]`` to the pre-padded ``[1, 3, H + pre_pad, W + pre_pad]``.  The division is numpy's: in float32 a correctly rounded float32 quotient."""
    img = np.asarray(img_u8)
    v = img.astype(np.float32) / 255 if dtype == torch.float32 else img.astype(np.float64) / 255.
    x = torch.from_numpy(np.ascontiguousarray(v.transpose(2, 0, 1)))[None]
    return F.pad(x, (0, pre_pad, 0, pre_pad), "replicate" if mutant == "prepad_replicate" else "reflect") if pre_pad else x


def tile_process(sd, x, tile, tile_pad, dtype=torch.float64, mutant=None):
    """The x4 image ``[1, 3, 4 Hp, 4 Wp]`` of the pre-padded ``x``, tile by tile (``tile <= 0``: ``process``)."""
    _, _, H, W = x.shape
    out = torch.zeros((1, 3, SCALE * H, SCALE * W), dtype=dtype)
    for (y0, y1, x0, x1), (oy0, oy1, ox0, ox1), (Y0, X0) in tiles(H, W, tile, tile_pad, mutant):
        r = SM.network(sd, x[:, :, y0:y1, x0:x1], dtype)
        out[:, :, Y0:Y0 + oy1 - oy0, X0:X0 + ox1 - ox0] = r[:, :, oy0:oy1, ox0:ox1]
    return out


def to_u8(r, mutant=None):
    """(u, uint8 image ``[H, W, 3]``) of the cropped x4 output ``r [1, 3, H, W]``: ``u`` = clamp(r, 0, 1) * 255 in r's precision."""
    u = (torch.as_tensor(r)[0].clamp(0, 1).permute(1, 2, 0) * 255.0).numpy()
    return u, (np.floor(u + 0.5) if mutant == "half_up" else np.rint(u)).astype(np.uint8)


def x4(sd, img_u8, tile, tile_pad, pre_pad, dtype=torch.float64, mutant=None):
    """``pre_process -> tile_process -> post_process`` on a uint8 ``[H, W, 3]`` image: (r ``[1, 3, 4H, 4W]`` as an array, u, the uint8 x4 image)."""
    H, W = np.asarray(img_u8).shape[:2]
    r = tile_process(sd, pre_process(img_u8, pre_pad, dtype, mutant), tile, tile_pad, dtype, mutant)[:, :, :SCALE * H, :SCALE * W].numpy()
    return (r,) + to_u8(r, mutant)


def out_size(H, W, outscale):
    """``(Wo, Ho)`` of ``enhance``'s cv2.resize, or None where it does not run."""
    return None if outscale is None or outscale == float(SCALE) else (int(W * outscale), int(H * outscale))


def enhance(sd, img_u8, outscale, tile, tile_pad, pre_pad, dtype=torch.float64, mutant=None):
    """``RealESRGANer.enhance(img, outscale)`` on an RGB uint8 ``[H, W, 3]`` image under the RGB convention: the uint8 result."""
    img = np.asarray(img_u8)
    big = x4(sd, img, tile, tile_pad, pre_pad, dtype, mutant)[2]
    dsize = out_size(img.shape[0], img.shape[1], outscale)
    return big if dsize is None else resize_lanczos4(big, dsize, mutant)


# ------------------------------------------------------------------------------------------------ cv2.resize, INTER_LANCZOS4, uint8
S45 = 0.70710678118654752440084436210485
CS = ((1, 0), (-S45, -S45), (0, 1), (S45, -S45), (-1, 0), (S45, S45), (0, -1), (-S45, S45))
F32 = np.float32


def lanczos4_coeffs_f32(f):
    """``interpolateLanczos4``: eight float32 coefficients at the float32 fraction ``f``."""
    f = F32(f)
    if f < np.finfo(np.float32).eps:
        return [F32(0)] * 3 + [F32(1)] + [F32(0)] * 4
    x3 = F32(f + F32(3))
    y0 = -float(x3) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c, total = [], F32(0)
    for i in range(8):
        y = -float(F32(x3 - F32(i))) * math.pi * 0.25
        c.append(F32((CS[i][0] * s0 + CS[i][1] * c0) / (y * y)))
        total = F32(total + c[i])
    inv = F32(F32(1) / total)
    return [F32(v * inv) for v in c]


def lanczos4_taps(f, mutant=None):
    """The eight 11-bit integer coefficients at the fraction ``f``."""
    taps = [int(np.rint(F32(v * F32(2048)))) for v in lanczos4_coeffs_f32(f)]
    if mutant == "lanczos_sum_fixed":
        taps[int(np.argmax(taps))] += 2048 - sum(taps)
    return taps


def lanczos4_axis(src, dst, mutant=None):
    """(index int64 [dst, 8] (clamped), taps int64 [dst, 8], f float32 [dst]) of one axis."""
    scale = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    f = (d * scale).astype(np.float32) if mutant == "lanczos_no_center" else ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    if mutant == "lanczos_fraction_clamped":                                                  # INTER_LINEAR's border rule, which INTER_LANCZOS4 does not have
        lo, hi = s < 0, s >= src - 1
        s = np.where(lo, 0, np.where(hi, src - 1, s))
        f = np.where(lo | hi, F32(0), f).astype(np.float32)
    idx = np.clip(s[:, None] - 3 + np.arange(8)[None], 0, src - 1)
    cache = {}
    taps = np.array([cache.get(v) or cache.setdefault(v, lanczos4_taps(v, mutant)) for v in f.tolist()], dtype=np.int64).reshape(dst, 8)
    return idx, taps, f


def lanczos4_kernel(x):
    """The Lanczos-4 window sinc(x) sinc(x / 4) on |x| < 4, float64."""
    x = np.asarray(x, np.float64)
    return np.where(np.abs(x) < 4, np.sinc(x) * np.sinc(x / 4), 0.0)


def resample_lanczos4_f64(img_u8, dsize, antialias=False):
    """A float64 Lanczos-4 resample with clamped borders at cv2's coordinates, rounded and clipped to uint8: what the integer resize is a fixed-point form of.
    ``antialias``: the support scaled by the shrink ratio, which PIL does and cv2 does not."""
    img = np.asarray(img_u8).astype(np.float64)
    Wo, Ho = int(dsize[0]), int(dsize[1])
    for axis, dst in ((1, Wo), (0, Ho)):
        src = img.shape[axis]
        scale = src / dst
        fs = max(scale, 1.0) if antialias else 1.0
        n = int(math.ceil(4 * fs))
        c = (np.arange(dst) + 0.5) * scale - 0.5
        base = np.floor(c).astype(np.int64)
        k = np.arange(-n + 1, n + 1)
        pos = base[:, None] + k[None]
        wgt = lanczos4_kernel((pos - c[:, None]) / fs)
        wgt /= wgt.sum(1, keepdims=True)
        taken = np.take(img, np.clip(pos, 0, src - 1).reshape(-1), axis=axis)
        shape = list(img.shape)
        shape[axis:axis + 1] = [dst, len(k)]
        wshape = [1] * len(shape)
        wshape[axis], wshape[axis + 1] = dst, len(k)
        img = (taken.reshape(shape) * wgt.reshape(wshape)).sum(axis + 1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def resize_lanczos4(img_u8, dsize, mutant=None):
    """``cv2.resize(img, (Wo, Ho), interpolation=cv2.INTER_LANCZOS4)`` of a uint8 ``[H, W, 3]`` (or batched ``[bs, H, W, 3]``) image, in integer arithmetic."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8
    if img.ndim == 4:
        return np.stack([resize_lanczos4(i, dsize, mutant) for i in img])
    if mutant == "lanczos_antialias":
        return resample_lanczos4_f64(img, dsize, antialias=True)
    H, W = img.shape[:2]
    Wo, Ho = int(dsize[0]), int(dsize[1])
    yi, yt, fy = lanczos4_axis(H, Ho, mutant)
    xi, xt, fx = lanczos4_axis(W, Wo, mutant)
    if mutant == "lanczos_float":
        cy = np.array([lanczos4_coeffs_f32(v) for v in fy], np.float64)
        cx = np.array([lanczos4_coeffs_f32(v) for v in fx], np.float64)
        rows = (img.astype(np.float64)[:, xi] * cx[None, :, :, None]).sum(2)
        return np.clip(np.rint((rows[yi] * cy[:, :, None, None]).sum(1)), 0, 255).astype(np.uint8)
    rows = (img.astype(np.int64)[:, xi] * xt[None, :, :, None]).sum(2)                        # [H, Wo, 3]
    assert np.abs(rows).max() < 2 ** 31
    v = (rows[yi] * yt[:, :, None, None]).sum(1)                                              # [Ho, Wo, 3]
    assert np.abs(v).max() + (1 << 21) < 2 ** 31
    return np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ cases
def image_u8(tag, H, W, seed=CASE_SEED, bs=1):
    return SM.images_u8(seed * 1000 + sum(map(ord, tag)), bs, H, W)


def solved(sd, img, tile, tile_pad, pre_pad):
    """dict(sd, img, r, u, x4, e32): ``sd`` calibrated on the RGB uint8 image ``img [H, W, 3]``, the float64 model on it and the float32 model's error."""
    r0 = x4(sd, img, tile, tile_pad, pre_pad)[0]
    sd = SM.calibrated(sd, r0)
    r, u, big = x4(sd, img, tile, tile_pad, pre_pad)
    r32, u32, big32 = x4(sd, img, tile, tile_pad, pre_pad, torch.float32)
    return dict(sd=sd, img=img, r=r, u=u, x4=big, r32=r32, x4_f32=big32, e32=max_err(r32, r), cfg=(tile, tile_pad, pre_pad))


def golden_case(tag, seed=CASE_SEED):
    """dict(sd, img [H, W, 3] RGB, r, u, x4, r32, x4_f32, e32, cfg) of a golden case, made once."""
    key = (tag, seed)
    if key not in _CASE:
        H, W, tile, tile_pad, pre_pad = GOLDEN_CASES[tag]
        _CASE[key] = solved(SM.base_state_dict(SCALE, NUM_FEAT, GOLDEN_BLOCKS, seed), image_u8(tag, H, W, seed)[0], tile, tile_pad, pre_pad)
    return _CASE[key]


def deep_case():
    """dict(...) of the 23-block case, as ``golden_case``; a batch of one."""
    tag, nb, H, W, tile, tile_pad, pre_pad = DEEP_CASE
    if tag not in _CASE:
        _CASE[tag] = solved(SM.base_state_dict(SCALE, NUM_FEAT, nb, CASE_SEED), image_u8(tag, H, W)[0], tile, tile_pad, pre_pad)
    return _CASE[tag]


def conditioned(c):
    """(strict share, clamped share, std) of the MODEL in float32 against itself in float64 under the uint8 rule."""
    return check_u8(c["x4_f32"], c["u"], c["e32"])


def resize_image(H, W, bs=2):
    return SM.images_u8(2300 + 31 * H + W, bs, H, W)
