"""The Real-ESRGAN step of the recolouring (row f11) restated directly, in float64 or float32: basicsr's ``RRDBNet(3, 3, 64, num_block, 32, scale=4)`` and
the two wrappers of ``RealESRBatchInfer`` (swap_face_fine/realesr/image_infer.py:60-80), with the seeded inputs and cases of the tests and single-change
mutants of itself.  basicsr is not installed and its architecture file is not in the reference tree, so there is no reference-made fixture for this row: this
model, written from the architecture's published description, is the pin.

    RDB      x1 = lrelu(conv1(x)); x_k = lrelu(conv_k(cat(x, x1 .. x_{k-1}))), k = 2 .. 4; out = conv5(cat(x, x1 .. x4)) * 0.2 + x      lrelu = LeakyReLU(0.2)
    RRDB     out = rdb3(rdb2(rdb1(x))) * 0.2 + x
    network  f = conv_first(x); f = f + conv_body(body(f)); f = lrelu(conv_up1(nearest_x2(f))); f = lrelu(conv_up2(nearest_x2(f)))
             out = conv_last(lrelu(conv_hr(f)))                                   every convolution 3x3, stride 1, zero pad 1, with bias
    batch    clamp(x * 0.5 + 0.5, 0, 1) -> bilinear (align_corners=True) to in_size -> network -> bilinear to out_hw -> clamp(r * 2 - 1, -1, 1)
    image    uint8 -> v / 127.5 - 1 -> batch(out_hw = out_size) -> * 127.5 + 127.5 -> clamp(0, 255) -> uint8 (truncating)

Weights: ``seeded.seeded_rrdbnet_state_dict`` (normal, 0.7 / sqrt(fan_in); biases over +-0.1), then conv_last's weight and bias rescaled per case so that the
float64 output on the case has mean 0.5 and standard deviation 0.25: the image behind the wrappers' clamps then spreads over the grey levels with 4 - 5 % of
the pixels clamped.  (At a gain of 1.0 without the rescale 96 % of the pixels saturate and a uint8 comparison sees nothing; basicsr's own 0.1-scaled
initialisation gives a flat output.)

``dtype=torch.float32`` runs the same expressions in float32: ``e32``, from which the tests take their bounds, ``bound = max(8 e32, 2e-7 max|want|)`` — the
convention of rows f9 / f10; it is never computed from the code under test.

The uint8 rule.  With ``u`` the float64 value before the clamp to [0, 255] and the truncation, and ``margin = 8 e32 * 255``, a pixel is *strict* when ``u``
is clamped (``u < 1 - margin`` truncates to 0 whatever side of 0 it lies on; ``u >= 255 + margin``) or lies farther than ``margin`` from an integer.  Strict
pixels must equal ``floor(clamp(u))``; the others may differ by one.  (A pixel clamped at 255 by LESS than the margin is not strict: an output inside the bound
may lie just below 255 there and truncate to 254.)"""
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

FLOOR = 2e-7
MARGIN = 8.0
MUTANT_MARGIN = 10.0                         # every mutant moves the float64 output by at least this many bounds on some case
WEIGHT_SEED = 23
SLOPE = 0.2
OUT_MEAN, OUT_STD = 0.5, 0.25

# network cases: tag -> (num_block, h, w, batch)
CASES = {
    "b1.5x3": (1, 5, 3, 1),                  # odd sizes, planes at odd offsets in the slabs
    "b2.12x20": (2, 12, 20, 1),
    "b23.7x9": (23, 7, 9, 1),                # the full depth
    "b23.8x8.bs2": (23, 8, 8, 2),
    "b1.20x20": (1, 20, 20, 1),              # 80 x 80 out: the tail spans tiles in both directions
}
# image cases: tag -> (num_block, H, W, batch, in_size, out_size)
IMAGE_CASES = {
    "img.40x36": (23, 40, 36, 2, 8, 32),
    "img.256x256": (23, 256, 256, 1, 8, 32),
}
# the reference's own sizes, once, with one block.  A float64 1024 x 1024 network is too slow for a test, so the model is evaluated on the two K x K corners of
# the network's 256 x 256 input: one block sees 17 pixels around itself before the upsampling and less than 2 more behind it, so the outermost 4 (K - 20)
# output pixels of each corner depend on nothing outside it, zero padding at the two image borders included.
REAL_CASE = ("img.real", 1, 300, 280, 1, 256, 1024)
REAL_K, REAL_REACH = 48, 20
MUTANTS = ("slope_0.1", "rdb_scale_0.25", "rrdb_residual_missing", "x3_dropped_from_conv5", "align_corners_false", "nearest_as_bilinear",
           "hr_lrelu_missing", "uint8_rounds")


def bound(e32, want):
    return max(MARGIN * float(e32), FLOOR * float(np.abs(np.asarray(want)).max()))


def max_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


# ------------------------------------------------------------------------------------------------ seeded inputs and weights
def images01(seed, bs, h, w):
    """float32 [bs, 3, h, w] in [0, 1]: what the network sees behind ``infer_batch``'s first clamp."""
    return (seeded.seeded_array(seed, "esr.x", (bs, 3, h, w)) / (2 * np.sqrt(3.0)) + 0.5).clip(0, 1).astype(np.float32)


def images_u8(seed, bs, H, W, noise=40):
    """uint8 [bs, H, W, 3]: smooth waves over the whole range plus uniform noise of +-``noise`` grey levels.  The kernel tests take the rough default.  The
    image cases take ``noise=1``: ATen's float32 source coordinate ``dst * scale`` is off by up to an ulp of the image width (1.5e-5 at 256), which moves a
    resized value by that times the difference of two neighbours; on a rough image that alone is several times the float32 network's own error and would
    leave fewer than 99 % of the pixels strict, on a smooth one it is below a float32 rounding."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rs = np.random.RandomState(seed)
    img = np.zeros((bs, H, W, 3))
    for b in range(bs):
        for c in range(3):
            fy, fx, ph = rs.uniform(0.5, 3.0), rs.uniform(0.5, 3.0), rs.uniform(0, 6.28)
            img[b, :, :, c] = 127.5 + 130 * np.sin(fy * yy / max(H, 2) * 6.28 + fx * xx / max(W, 2) * 6.28 + ph)
    img += rs.uniform(-noise, noise, img.shape)
    return img.clip(0, 255).astype(np.uint8)


def aten_coords(out, inp):
    """(i0, i1, l1) of ``F.interpolate(mode='bilinear', align_corners=True)`` along one axis as ATen forms them in float32: the scale, the product with the
    destination index, the truncation and the difference, each rounded to float32."""
    scale = np.float32(inp - 1) / np.float32(out - 1) if out > 1 else np.float32(0)
    src = (np.arange(out, dtype=np.float32) * scale).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32).astype(np.float64)


def esr_input_f32_coords(img_u8, oh, ow):
    """``esr_input`` in float64 at the float32 source coordinates every float32 implementation of the resize uses (``aten_coords``): what a kernel can be held
    to within a few roundings on ANY image."""
    v = np.asarray(img_u8).transpose(0, 3, 1, 2).astype(np.float64)
    v = np.clip((v / 127.5 - 1.) * 0.5 + 0.5, 0, 1)
    y0, y1, ly = aten_coords(oh, v.shape[2])
    x0, x1, lx = aten_coords(ow, v.shape[3])
    ly, lx = ly[:, None], lx[None, :]
    top = (1 - lx) * v[:, :, y0][:, :, :, x0] + lx * v[:, :, y0][:, :, :, x1]
    bottom = (1 - lx) * v[:, :, y1][:, :, :, x0] + lx * v[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bottom


_SD = {}


def base_state_dict(num_block, seed=WEIGHT_SEED):
    if (num_block, seed) not in _SD:
        _SD[num_block, seed] = seeded.seeded_rrdbnet_state_dict(seed, num_block)
    return _SD[num_block, seed]


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
    return F.conv2d(x, sd[p + ".weight"].to(x), sd[p + ".bias"].to(x), padding=1)                 # (dtype and device of x: the model also runs on the device)


def lrelu(x, mutant=None):
    return F.leaky_relu(x, 0.1 if mutant == "slope_0.1" else SLOPE)


def rdb(sd, p, x, mutant=None):
    xs = [x]
    for k in range(1, 5):
        xs.append(lrelu(conv(sd, f"{p}.conv{k}", torch.cat(xs, 1)), mutant))
    if mutant == "x3_dropped_from_conv5":
        xs[3] = torch.zeros_like(xs[3])
    return conv(sd, f"{p}.conv5", torch.cat(xs, 1)) * (0.25 if mutant == "rdb_scale_0.25" else 0.2) + x


def rrdb(sd, p, x, mutant=None):
    y = rdb(sd, p + ".rdb3", rdb(sd, p + ".rdb2", rdb(sd, p + ".rdb1", x, mutant), mutant), mutant) * 0.2
    return y if mutant == "rrdb_residual_missing" else y + x


def up2(x, mutant=None):
    if mutant == "nearest_as_bilinear":
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return F.interpolate(x, scale_factor=2, mode="nearest")


def num_blocks(sd):
    n = 0
    while f"body.{n}.rdb1.conv1.weight" in sd:
        n += 1
    return n


def network(sd, x, dtype=torch.float64, mutant=None):
    """``RRDBNet.forward``: ``x`` an array or tensor ``[bs, 3, h, w]``; returns a tensor of ``dtype`` ``[bs, 3, 4h, 4w]``."""
    x = torch.as_tensor(x).to(dtype)
    with torch.no_grad():
        feat = conv(sd, "conv_first", x)
        body = feat
        for i in range(num_blocks(sd)):
            body = rrdb(sd, f"body.{i}", body, mutant)
        feat = feat + conv(sd, "conv_body", body)
        feat = lrelu(conv(sd, "conv_up1", up2(feat, mutant)), mutant)
        feat = lrelu(conv(sd, "conv_up2", up2(feat, mutant)), mutant)
        hr = conv(sd, "conv_hr", feat)
        return conv(sd, "conv_last", hr if mutant == "hr_lrelu_missing" else lrelu(hr, mutant))


# ------------------------------------------------------------------------------------------------ the wrappers
def esr_input(img_u8, oh, ow, dtype=torch.float64, mutant=None):
    """The head of ``infer_image`` and ``infer_batch``: uint8 ``[bs, H, W, 3]`` to ``[bs, 3, oh, ow]`` in [0, 1]."""
    v = torch.as_tensor(img_u8).permute(0, 3, 1, 2).to(dtype)
    v = ((v / 127.5 - 1.) * 0.5 + 0.5).clamp(0, 1)
    return F.interpolate(v, size=(oh, ow), mode="bilinear", align_corners=mutant != "align_corners_false")


def infer_batch(sd, x, out_hw=None, in_size=256, dtype=torch.float64, mutant=None):
    x = torch.as_tensor(x).to(dtype)
    out_hw = tuple(x.shape[2:]) if out_hw is None else tuple(out_hw)
    s = F.interpolate((x * 0.5 + 0.5).clamp(0, 1), size=(in_size, in_size), mode="bilinear", align_corners=True)
    r = F.interpolate(network(sd, s, dtype, mutant), size=out_hw, mode="bilinear", align_corners=True)
    return (r * 2. - 1.).clamp(-1, 1)


def to_u8(r, mutant=None):
    """(u, uint8 image ``[bs, H, W, 3]``) of the network output ``r [bs, 3, H, W]``: ``u`` the value before the last clamp and the truncation, NHWC."""
    a = (torch.as_tensor(r) * 2. - 1.)
    u = (a * 127.5 + 127.5).permute(0, 2, 3, 1)
    v = (a.clamp(-1, 1) * 127.5 + 127.5).clamp(0, 255).permute(0, 2, 3, 1)
    if mutant == "uint8_rounds":
        v = torch.round(v)
    return u.numpy(), v.to(torch.uint8).numpy()


def image_network_output(sd, img_u8, in_size, out_size, dtype=torch.float64, mutant=None):
    """The network output ``r`` of ``infer_image`` on ``img_u8`` (``out_size == 4 in_size``, where the second resize is the identity)."""
    assert out_size == 4 * in_size
    return network(sd, esr_input(img_u8, in_size, in_size, dtype, mutant), dtype, mutant)


def strict_pixels(u, e32):
    margin = MARGIN * float(e32) * 255
    return (u < 1 - margin) | (u >= 255 + margin) | (np.abs(u - np.rint(u)) > margin)


def expected_u8(u):
    return np.floor(np.clip(u, 0, 255)).astype(np.uint8)


def check_u8(got, u, e32):
    """The uint8 rule on ``got`` against the float64 ``u``; returns (strict share, clamped share, standard deviation of the expected image)."""
    want, strict = expected_u8(u), strict_pixels(u, e32)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert (diff[strict] == 0).all(), f"{int((diff[strict] != 0).sum())} strict pixels differ"
    assert diff.max() <= 1, f"a pixel differs by {int(diff.max())}"
    return float(strict.mean()), float(((u <= 0) | (u >= 255)).mean()), float(want.astype(np.float64).std())


# ------------------------------------------------------------------------------------------------ the kernels alone
def tail_f32(x, weight, bias):
    """conv_last in float32 in the kernel's documented order: bias, then one multiply-add per (input channel, row, column), every pixel on its own chain
    (NumPy rounds the product before the sum, the kernel fuses them: the same class).  Elementwise float32 NumPy, so the same bits on every machine,
    which a float32 convolution of a library (blocked, threaded sums) is not."""
    x, w = np.asarray(x, np.float32), np.asarray(weight, np.float32)
    bs, C, H, W = x.shape
    xp = np.zeros((bs, C, H + 2, W + 2), np.float32)
    xp[:, :, 1:-1, 1:-1] = x
    acc = np.broadcast_to(np.asarray(bias, np.float32)[None, :, None, None], (bs, 3, H, W)).copy()
    for c in range(C):
        for ky in range(3):
            for kx in range(3):
                acc += w[None, :, c, ky, kx, None, None] * xp[:, None, c, ky:ky + H, kx:kx + W]
    return acc


def tail(x, weight, bias):
    """``e4s_esr_tail`` in float64: dict(r ``[bs, 3, H, W]``, bound, u, e32).  ``bound`` is (577 + 1) 2^-24 max(sum |w x| + |b|): 576 products and 577
    additions, each within half an ulp of a partial sum that never exceeds that maximum.  ``e32`` is ``tail_f32`` against float64: the margin of the uint8
    rule."""
    x, w, b = (torch.as_tensor(t) for t in (x, weight, bias))
    r = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    mag = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    return dict(r=r.numpy(), bound=578 * 2.0 ** -24 * float(mag.max()), u=to_u8(r)[0], e32=max_err(tail_f32(x.numpy(), w.numpy(), b.numpy()), r.numpy()))


# ------------------------------------------------------------------------------------------------ cases
_CASE = {}


def case(tag):
    """dict(sd, x, want, e32) of a network case, made once: calibrated weights, float32 input, float64 output, float32-model error."""
    if tag not in _CASE:
        nb, h, w, bs = CASES[tag]
        x = images01(sum(map(ord, tag)), bs, h, w)
        sd = base_state_dict(nb)
        sd = calibrated(sd, network(sd, x))
        want = network(sd, x).numpy()
        _CASE[tag] = dict(sd=sd, x=x, want=want, e32=max_err(network(sd, x, torch.float32).numpy(), want))
    return _CASE[tag]


def image_case(tag):
    """dict(sd, img, want, u, e32, in_size, out_size) of an image case, made once."""
    if tag not in _CASE:
        nb, H, W, bs, in_size, out_size = IMAGE_CASES[tag]
        img = images_u8(sum(map(ord, tag)), bs, H, W, noise=1)
        sd = base_state_dict(nb)
        sd = calibrated(sd, image_network_output(sd, img, in_size, out_size))
        want = image_network_output(sd, img, in_size, out_size)
        e32 = max_err(image_network_output(sd, img, in_size, out_size, torch.float32).numpy(), want.numpy())
        _CASE[tag] = dict(sd=sd, img=img, want=want.numpy(), u=to_u8(want)[0], e32=e32, in_size=in_size, out_size=out_size)
    return _CASE[tag]


def real_corners(x):
    """The two corner crops of the network's input ``[bs, 3, S, S]`` and where the output pixels they determine lie: [(crop, output slices)]."""
    n = 4 * (REAL_K - REAL_REACH)
    return [(x[:, :, :REAL_K, :REAL_K], (slice(0, n), slice(0, n)), (slice(0, n), slice(0, n))),
            (x[:, :, -REAL_K:, -REAL_K:], (slice(-n, None), slice(-n, None)), (slice(-n, None), slice(-n, None)))]


def real_case():
    """dict(sd, img, parts, e32) of the case at the reference's sizes: ``parts`` = [(output slices, float64 u of that corner)]."""
    tag, nb, H, W, bs, in_size, out_size = REAL_CASE
    if tag not in _CASE:
        img = images_u8(sum(map(ord, tag)), bs, H, W, noise=1)
        x64, x32 = esr_input(img, in_size, in_size), esr_input(img, in_size, in_size, torch.float32)
        sd = base_state_dict(nb)
        outs = [network(sd, crop)[:, :, own[0], own[1]] for crop, own, _ in real_corners(x64)]
        sd = calibrated(sd, torch.cat([o.reshape(-1) for o in outs]))
        parts, e32 = [], 0.0
        for (c64, own, where), (c32, _, _) in zip(real_corners(x64), real_corners(x32)):
            want = network(sd, c64)[:, :, own[0], own[1]]
            e32 = max(e32, max_err(network(sd, c32, torch.float32)[:, :, own[0], own[1]].numpy(), want.numpy()))
            parts.append((where, to_u8(want)[0]))
        _CASE[tag] = dict(sd=sd, img=img, parts=parts, e32=e32, in_size=in_size, out_size=out_size)
    return _CASE[tag]
