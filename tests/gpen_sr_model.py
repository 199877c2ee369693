"""Row f16: the RealESRNet pass of GPEN's ``FaceEnhancement.process`` restated directly, in float64 or float32 — ``RRDBNet(3, 3, scale, num_feat, num_block, 32)``
of swap_face_fine/gpen/sr_model/rrdbnet_arch.py with the ``pixel_unshuffle`` of arch_util.py in front of it, ``RealESRNet.process`` of real_esrnet.py around it —
and ``cv2.resize`` at its default ``INTER_LINEAR`` in numpy integer arithmetic, with the seeded cases of the tests and single-change mutants of itself.

    network  f = conv_first(unshuffle_r(x)); f = f + conv_body(body(f)); f = lrelu(conv_up1(nearest_x2(f))); f = lrelu(conv_up2(nearest_x2(f)))
             out = conv_last(lrelu(conv_hr(f)))           r = 1, 2, 4 at scale 4, 2, 1; unshuffle channel c r r + dy r + dx; RDB / RRDB as tests/rrdb_model.py
    process  uint8 BGR -> / 255 -> RGB -> reflect pad (bottom, right) to a multiple of r -> network -> crop of ph rows, pw columns (of the OUTPUT: the
             reference takes off ph, not scale * ph) -> clamp(0, 1) -> BGR -> (x * 255.0).round() (half to even) -> uint8
    resize   per axis scale = src / dst (double), f = float((d + 0.5) scale - 0.5), s = floor(f), f -= s; s < 0: s = 0, f = 0; s >= src - 1: s = src - 1, f = 0;
             a0 = short(rint((1 - f) 2048)), a1 = short(rint(f 2048)) with 1 - f in float32; rows in int32 h = S[s] a0 + S[s + 1] a1; then
             (((b0 (h0 >> 4)) >> 16) + ((b1 (h1 >> 4)) >> 16) + 2) >> 2

The network and ``process`` are checked against the reference's own code on the CPU (tests/golden/g27_gpen_sr.npz).  cv2 is installed nowhere this project is
built or tested, so the resize has never been run against OpenCV: this restatement of OpenCV's portable (non-SIMD) fixed-point path is the pin, as
tests/gpen_paste_model.py pins ``warpAffine``.  One known difference from OpenCV's source is kept as the issue states the rule: OpenCV clamps the ROW index of an
out-of-range ``s`` and keeps its fraction, which on the first and last output rows of an upscale can differ from ``f = 0`` by one grey level.

Weights: ``seeded.seeded_gpen_sr_state_dict`` (row f11's distribution), then conv_last's weight and bias rescaled per case so that the float64 output on the case
has mean 0.5 and standard deviation 0.25 (tests/rrdb_model.py explains why).  ``bound = max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against
itself in float64; it is never computed from the code under test.

The uint8 rule for a rounding end.  With ``u = clamp(r, 0, 1) * 255`` in float64 and ``margin = 8 e32 * 255``, a pixel is *strict* when ``u`` lies farther than
``margin`` from every ``k + 0.5``.  Strict pixels must equal ``rint(u)``; the others may differ by one."""
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

FLOOR = 2e-7
MARGIN = 8.0
MUTANT_MARGIN = 10.0                         # every mutant moves the model by at least this many bounds on some case (the integer resize: one grey level)
WEIGHT_SEED = 27
SLOPE = 0.2
OUT_MEAN, OUT_STD = 0.5, 0.25
UNSHUFFLE = {4: 1, 2: 2, 1: 4}

# the golden's networks: (scale, num_feat, num_block), and its images (H, W): odd, even and mixed parity
GOLDEN_NETS = ((2, 32, 1), (4, 32, 2), (1, 64, 1), (2, 64, 1))
GOLDEN_SIZES = ((7, 9), (12, 20), (5, 6))
# the full depth, on the device tests only: (scale, num_feat, num_block, h, w, batch)
DEEP_CASE = ("s2.f32.b23.8x8", 2, 32, 23, 8, 8, 2)
NET_MUTANTS = ("unshuffle_order", "pad_replicate", "residual_missing")
END_MUTANTS = ("crop_scaled", "half_up", "truncate", "no_flip_out")
RESIZE_MUTANTS = ("resize_no_center", "resize_float")
MUTANTS = NET_MUTANTS + END_MUTANTS + RESIZE_MUTANTS


def tag_of(scale, num_feat, num_block, H, W):
    return f"s{scale}.f{num_feat}.b{num_block}.{H}x{W}"


IMAGE_CASES = {tag_of(s, f, b, H, W): (s, f, b, H, W) for s, f, b in GOLDEN_NETS for H, W in GOLDEN_SIZES}


def bound(e32, want):
    return max(MARGIN * float(e32), FLOOR * float(np.abs(np.asarray(want)).max()))


def max_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


# ------------------------------------------------------------------------------------------------ seeded inputs and weights
def images_u8(seed, bs, H, W, noise=40):
    """uint8 [bs, H, W, 3]: smooth waves over the whole range plus uniform noise of +-``noise`` grey levels."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rs = np.random.RandomState(seed)
    img = np.zeros((bs, H, W, 3))
    for b in range(bs):
        for c in range(3):
            fy, fx, ph = rs.uniform(0.5, 3.0), rs.uniform(0.5, 3.0), rs.uniform(0, 6.28)
            img[b, :, :, c] = 127.5 + 130 * np.sin(fy * yy / max(H, 2) * 6.28 + fx * xx / max(W, 2) * 6.28 + ph)
    img += rs.uniform(-noise, noise, img.shape)
    return img.clip(0, 255).astype(np.uint8)


_SD = {}
_CASE = {}


def base_state_dict(scale, num_feat, num_block, seed=WEIGHT_SEED):
    key = (scale, num_feat, num_block, seed)
    if key not in _SD:
        _SD[key] = seeded.seeded_gpen_sr_state_dict(seed, num_block, num_feat, scale)
    return _SD[key]


def calibrated(sd, out64):
    """``sd`` with conv_last's weight and bias rescaled so that ``out64``, the float64 output under ``sd``, gets mean 0.5 and standard deviation 0.25."""
    m, s = float(out64.mean()), float(out64.std())
    a = OUT_STD / s
    sd = dict(sd)
    sd["conv_last.weight"] = (sd["conv_last.weight"].double() * a).float()
    sd["conv_last.bias"] = ((sd["conv_last.bias"].double() - m) * a + OUT_MEAN).float()
    return sd


# ------------------------------------------------------------------------------------------------ the network
def conv(sd, p, x):
    return F.conv2d(x, sd[p + ".weight"].to(x), sd[p + ".bias"].to(x), padding=1)


def lrelu(x):
    return F.leaky_relu(x, SLOPE)


def rdb(sd, p, x):
    xs = [x]
    for k in range(1, 5):
        xs.append(lrelu(conv(sd, f"{p}.conv{k}", torch.cat(xs, 1))))
    return conv(sd, f"{p}.conv5", torch.cat(xs, 1)) * 0.2 + x


def rrdb(sd, p, x, mutant=None):
    y = rdb(sd, p + ".rdb3", rdb(sd, p + ".rdb2", rdb(sd, p + ".rdb1", x)))
    return y + x if mutant == "residual_missing" else y * 0.2 + x                # (the mutant: the 0.2 of the residual is missing)


def num_blocks(sd):
    n = 0
    while f"body.{n}.rdb1.conv1.weight" in sd:
        n += 1
    return n


def scale_of(sd):
    return {3: 4, 12: 2, 48: 1}[int(sd["conv_first.weight"].shape[1])]


def unshuffle(x, r, mutant=None):
    """arch_util.pixel_unshuffle: [b, c, h, w] -> [b, c r r, h / r, w / r], channel c r r + dy r + dx (the mutant: dx r + dy)."""
    b, c, hh, hw = x.shape
    assert hh % r == 0 and hw % r == 0
    v = x.reshape(b, c, hh // r, r, hw // r, r)                                   # (b, c, y, dy, x, dx)
    v = v.permute(0, 1, 5, 3, 2, 4) if mutant == "unshuffle_order" else v.permute(0, 1, 3, 5, 2, 4)
    return v.reshape(b, c * r * r, hh // r, hw // r)


def up2(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def network(sd, x, dtype=torch.float64, mutant=None):
    """``RRDBNet.forward``: ``x`` an array or tensor ``[bs, 3, h, w]`` with h, w divisible by r; returns a tensor of ``dtype`` ``[bs, 3, 4h / r, 4w / r]``."""
    x = torch.as_tensor(x).to(dtype)
    r = UNSHUFFLE[scale_of(sd)]
    with torch.no_grad():
        feat = conv(sd, "conv_first", unshuffle(x, r, mutant) if r > 1 else x)
        body = feat
        for i in range(num_blocks(sd)):
            body = rrdb(sd, f"body.{i}", body, mutant)
        feat = feat + conv(sd, "conv_body", body)
        feat = lrelu(conv(sd, "conv_up1", up2(feat)))
        feat = lrelu(conv(sd, "conv_up2", up2(feat)))
        return conv(sd, "conv_last", lrelu(conv(sd, "conv_hr", feat)))


# ------------------------------------------------------------------------------------------------ RealESRNet.process
def pads(H, W, scale):
    r = UNSHUFFLE[scale]
    return -H % r, -W % r


def output_size(H, W, scale):
    ph, pw = pads(H, W, scale)
    return scale * (H + ph) - ph, scale * (W + pw) - pw


def sr_input(img_u8, scale, bgr=True, dtype=torch.float64, mutant=None):
    """The head of ``process`` for a batch: uint8 ``[bs, H, W, 3]`` to the padded ``[bs, 3, H + ph, W + pw]`` (before the unshuffle).  The division is numpy's:
    in float32, a correctly rounded float32 quotient."""
    img = np.asarray(img_u8)
    v = img.astype(np.float32) / 255. if dtype == torch.float32 else img.astype(np.float64) / 255.
    if bgr:
        v = v[..., ::-1]
    x = torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))
    ph, pw = pads(img.shape[1], img.shape[2], scale)
    return F.pad(x, (0, pw, 0, ph), "replicate" if mutant == "pad_replicate" else "reflect") if ph or pw else x


def sr_input_unshuffled_f32(img_u8, r, bgr=True):
    """What ``e4s_gsr_input`` writes, bit for bit: float32 ``[bs, 3 r r, (H + ph) / r, (W + pw) / r]``."""
    return unshuffle(sr_input(img_u8, UNSHUFFLE_INV[r], bgr, torch.float32), r).numpy()


UNSHUFFLE_INV = {r: s for s, r in UNSHUFFLE.items()}


def to_u8(r, crop, scale=1, bgr=True, mutant=None):
    """(u, uint8 image) of the network output ``r [bs, 3, H, W]`` (array or tensor): ``u`` = clamp(r, 0, 1) * 255 in r's precision, cropped by ``crop = (ph, pw)``
    and flipped, ``[bs, Ho, Wo, 3]``; the image is its rounding half to even."""
    r = torch.as_tensor(r)
    ph, pw = crop
    if mutant == "crop_scaled":
        ph, pw = scale * ph, scale * pw
    r = r[:, :, :r.shape[2] - ph, :r.shape[3] - pw].clamp(0, 1)
    if bgr and mutant != "no_flip_out":
        r = r.flip(1)
    u = (r.permute(0, 2, 3, 1) * 255.0).numpy()
    if mutant == "half_up":
        v = np.floor(u + 0.5)
    elif mutant == "truncate":
        v = np.floor(u)
    else:
        v = np.rint(u)
    return u, v.astype(np.uint8)


def process(sd, img_u8, bgr=True, dtype=torch.float64, mutant=None):
    """``RealESRNet.process`` for a batch ``[bs, H, W, 3]``: (network output ``[bs, 3, s (H + ph), s (W + pw)]`` as a tensor, u, uint8 ``[bs, Ho, Wo, 3]``)."""
    scale = scale_of(sd)
    img = np.asarray(img_u8)
    r = network(sd, sr_input(img, scale, bgr, dtype, mutant), dtype, mutant)
    u, out = to_u8(r, pads(img.shape[1], img.shape[2], scale), scale, bgr, mutant)
    return r, u, out


def strict_pixels(u, e32):
    margin = MARGIN * float(e32) * 255
    u = np.asarray(u, np.float64)
    return np.abs(u - np.floor(u) - 0.5) > margin


def check_u8(got, u, e32):
    """The uint8 rule on ``got`` against the float64 ``u``; returns (strict share, clamped share, standard deviation of the expected image)."""
    u = np.asarray(u, np.float64)
    want, strict = np.rint(u).astype(np.uint8), strict_pixels(u, e32)
    assert got.shape == want.shape, f"shape {got.shape}, expected {want.shape}"
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert (diff[strict] == 0).all(), f"{int((diff[strict] != 0).sum())} strict pixels differ"
    assert diff.max() <= 1, f"a pixel differs by {int(diff.max())}"
    return float(strict.mean()), float(((u <= 0) | (u >= 255)).mean()), float(want.astype(np.float64).std())


def tie_values():
    """float32 values r in [0, 1] whose float32 product with 255 is exactly k + 0.5, for even and odd k: where half-to-even and half-up part."""
    out = []
    for k in range(0, 255):
        r = np.float32((k + 0.5) / 255.0)
        for cand in (r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(1))):
            if np.float32(cand * np.float32(255.0)) == np.float32(k + 0.5):
                out.append(cand)
                break
    return np.array(out, np.float32)


# ------------------------------------------------------------------------------------------------ the kernels alone
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 values held in float64 arrays ``a``, ``b`` and a float32 array ``c``: the product is exact in float64
    (48 bits); the float64 sum is made round-to-odd with its error term (TwoSum), after which the rounding to float32 is the correct one (53 >= 24 + 2)."""
    p = a * b
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    inexact = err != 0
    if inexact.any():
        trunc = np.where(inexact & ((err > 0) != (s > 0)), np.nextafter(s, 0.0), s)           # the exact sum cut towards zero
        odd = (np.ascontiguousarray(trunc).view(np.int64) | 1).view(np.float64)
        s = np.where(inexact, odd, s)
    return s.astype(np.float32)


def tail_f32(x, weight, bias):
    """conv_last in float32 in the kernel's documented order, bit for bit: bias, then one FUSED multiply-add per (input channel, row, column), every pixel on
    its own chain.  Elementwise numpy, so the same bits on every machine."""
    x, w = np.asarray(x, np.float32), np.asarray(weight, np.float32)
    bs, C, H, W = x.shape
    xp = np.zeros((bs, C, H + 2, W + 2), np.float64)
    xp[:, :, 1:-1, 1:-1] = x
    w = w.astype(np.float64)
    acc = np.broadcast_to(np.asarray(bias, np.float32)[None, :, None, None], (bs, 3, H, W)).copy()
    for c in range(C):
        for ky in range(3):
            for kx in range(3):
                acc = fma32(w[None, :, c, ky, kx, None, None], xp[:, None, c, ky:ky + H, kx:kx + W], acc)
    return acc


def tail(x, weight, bias):
    """``e4s_gsr_tail``'s convolution in float64: dict(r ``[bs, 3, H, W]``, e32) with ``e32`` the float32 chain ``tail_f32`` against it: the margin of the uint8
    rule."""
    x, w, b = (torch.as_tensor(t) for t in (x, weight, bias))
    r = F.conv2d(x.double(), w.double(), b.double(), padding=1).numpy()
    f32 = tail_f32(x.numpy(), w.numpy(), b.numpy())
    return dict(r=r, f32=f32, e32=max_err(f32, r))


TAIL_SEED = 7                                # the first seed at which the MODEL leaves every tail case below conditioned (5 and 6 leave 98.5 % strict)
TAIL_CASES = tuple((C, H, W) for C in (32, 64) for H, W in ((9, 11), (20, 20)))
TAIL_CROPS = ((0, 0), (1, 3), (3, 2), (0, 4))


def tail_case(C, H, W, bs=2):
    """dict(x, w, b, r, f32, e32) of a case of the tail kernel alone, made once: unit-normal planes, weights that give the output a spread of 0.25 about 0.5."""
    key = ("tail", C, H, W, bs)
    if key not in _CASE:
        x = seeded.seeded_array(TAIL_SEED, "gsr.tail.x", (bs, C, H, W), 0.0, 1.0, "normal")
        w = seeded.seeded_array(TAIL_SEED, "gsr.tail.w", (3, C, 3, 3), 0.0, 0.25 / np.sqrt(C * 9.0), "normal")
        b = np.array([0.5, 0.45, 0.55], dtype=np.float32)
        _CASE[key] = dict(x=x, w=w, b=b, **tail(x, w, b))
    return _CASE[key]


# ------------------------------------------------------------------------------------------------ cv2.resize, INTER_LINEAR, uint8
def _resize_axis(src, dst, mutant=None):
    """(s int64 [dst], a0, a1 int64 [dst]; f float32 [dst]) of one axis."""
    scale = np.float64(src) / np.float64(dst)
    d = np.arange(dst, dtype=np.float64)
    f = (d * scale).astype(np.float32) if mutant == "resize_no_center" else ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, a0, a1, f


def resize_linear(img_u8, dsize, mutant=None):
    """``cv2.resize(img, (Wo, Ho))`` of a uint8 ``[H, W, 3]`` (or batched ``[bs, H, W, 3]``) image at INTER_LINEAR, in integer arithmetic."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8
    if img.ndim == 4:
        return np.stack([resize_linear(i, dsize, mutant) for i in img])
    H, W = img.shape[:2]
    Wo, Ho = int(dsize[0]), int(dsize[1])
    if H == 2 * Ho and W == 2 * Wo:
        raise ValueError("resize_linear: the exact 2 : 1 downscale is cv2's INTER_AREA")
    sy, b0, b1, fy = _resize_axis(H, Ho, mutant)
    sx, a0, a1, fx = _resize_axis(W, Wo, mutant)
    sy1, sx1 = np.minimum(sy + 1, H - 1), np.minimum(sx + 1, W - 1)
    S = img.astype(np.int64)
    if mutant == "resize_float":
        Sf = img.astype(np.float64)
        fx64, fy64 = fx.astype(np.float64)[None, :, None], fy.astype(np.float64)[:, None, None]
        rows = Sf[:, sx] * (1 - fx64) + Sf[:, sx1] * fx64
        return np.clip(np.rint(rows[sy] * (1 - fy64) + rows[sy1] * fy64), 0, 255).astype(np.uint8)
    rows = S[:, sx] * a0[None, :, None] + S[:, sx1] * a1[None, :, None]            # [H, Wo, 3], int32 range
    h0, h1 = rows[sy], rows[sy1]
    out = (((b0[:, None, None] * (h0 >> 4)) >> 16) + ((b1[:, None, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ cases


def solved(sd, img, bgr=True):
    """dict(sd, img, r, u, out, e32, scale): ``sd`` calibrated on the batch ``img [bs, H, W, 3]``, the float64 model on it and the float32 model's error."""
    scale = scale_of(sd)
    ph, pw = pads(img.shape[1], img.shape[2], scale)
    r0 = process(sd, img, bgr)[0]
    sd = calibrated(sd, r0[:, :, :r0.shape[2] - ph, :r0.shape[3] - pw])
    r, u, out = process(sd, img, bgr)
    r32 = process(sd, img, bgr, dtype=torch.float32)[0]
    return dict(sd=sd, img=img, r=r.numpy(), u=u, out=out, e32=max_err(r32.numpy(), r.numpy()), scale=scale)


def image_case(tag):
    """dict(sd, img [1, H, W, 3] BGR, r (float64 network output), u, out, e32, scale) of an image case, made once."""
    if tag not in _CASE:
        scale, nf, nb, H, W = IMAGE_CASES[tag]
        _CASE[tag] = solved(base_state_dict(scale, nf, nb), images_u8(sum(map(ord, tag)), 1, H, W))
    return _CASE[tag]


# FaceEnhancement.process with use_sr: tag -> (H, W of the frame, aligned); the network is FE_NET, calibrated on the case's input.  The faces, masks and
# detections are case A's of tests/golden/make_golden_gpen_paste.py (an 80 x 96 frame, S 32): the super-resolved frame has that size, or 79 x 95
FE_NET = (2, 32, 1)
FE_CASES = {"fe.full": (40, 48, False), "fe.odd": (39, 47, False), "fe.aligned": (32, 32, True)}
FE_PASTE = dict(S=32, ksize=9, sigma=1.5, thres=3, small_face=100)
FE_SHARED = ("dets", "landms", "ef", "pm")   # stored once in the golden, as fe.<key>


def fe_record(golden, tag):
    """A stored not-aligned FaceEnhancement case as tests/gpen_paste_model.py takes its cases (``frame`` is the RESIZED frame, ``base`` the reference's
    ``img_sr``), plus ``input``, the frame ``process`` was given."""
    rec = {k: golden[f"{tag}.{k}"] for k in ("frame", "out", "orig", "T", "cfg", "base", "input")}
    rec.update({k: golden[f"fe.{k}"] for k in FE_SHARED})
    return rec


def fe_frame(tag):
    """The BGR uint8 frame ``[H, W, 3]`` of a not-aligned FaceEnhancement case."""
    H, W, aligned = FE_CASES[tag]
    assert not aligned
    return images_u8(sum(map(ord, tag)), 1, H, W, noise=10)[0]


def fe_solved(tag, img_bgr):
    """``solved`` for the image the case's RealESRNet pass sees (the frame, or the enhanced face of the aligned case), made once."""
    if tag not in _CASE:
        _CASE[tag] = solved(base_state_dict(*FE_NET), np.asarray(img_bgr)[None])
    return _CASE[tag]


def deep_case():
    """dict(sd, x float32 [bs, 3, h, w], want, e32) of the 23-block network case."""
    tag, scale, nf, nb, h, w, bs = DEEP_CASE
    if tag not in _CASE:
        x = (images_u8(sum(map(ord, tag)), bs, h, w).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).copy()
        sd = base_state_dict(scale, nf, nb)
        sd = calibrated(sd, network(sd, x))
        want = network(sd, x).numpy()
        _CASE[tag] = dict(sd=sd, x=x, want=want, e32=max_err(network(sd, x, torch.float32).numpy(), want), scale=scale)
    return _CASE[tag]
