"""GPEN's generator (row f12) restated directly, in float64 or float32: ``FullGenerator.forward`` of swap_face_fine/gpen/face_model/gpen_model.py in eval mode
between the tensor ends of ``FaceGAN`` (face_gan.py:49-62), with the seeded inputs and cases of the tests and single-change mutants of itself.  Written from
the architecture's description, not by importing the reference; ``tests/golden/g23_gpen.npz`` holds what the reference's own module gives on the same cases.

    encoder   ecd0 = flrelu(conv1x1(x, W / sqrt(3)) + b); ecd_i = flrelu(conv3x3(blur(x, pad (2, 2)), W / sqrt(9 cin), stride 2, pad 0) + b), every level kept
              flrelu(v) = leaky_relu(v, 0.2) * sqrt(2);  blur = upfirdn2d with outer([1, 3, 3, 1]) / 64
    style     z = flrelu(flat(f4) @ (W / sqrt(16 C4))^T + b); w = MLP(pixelnorm(z)), n_mlp x flrelu(x @ (W 0.01 / sqrt(D))^T + 0.01 b); one w for every layer
    StyledConv  y = modconv(x, w); out = flrelu(cat(y, noise.weight * f_r) + bias[2C])          f_r: the encoder's feature of the layer's resolution
    modconv   s = w @ (M / sqrt(D))^T + m; W' = W s / sqrt(9 cin); W' *= rsqrt(sum W'^2 + 1e-8) per output; same resolution: conv pad 1; up: conv_transpose
              stride 2, then blur pad (1, 1) with 4 x the kernel
    ToRGB     1 x 1 modconv without demodulation + bias + upfirdn2d(skip, 4 x kernel, up 2, pad (2, 1))
    ends      uint8 -> v / 255 -> (v - 0.5) / 0.5;   x * 0.5 + 0.5 -> clip(0, 1) -> * 255 -> uint8 (truncating)                 (RGB throughout: no flips)

``dtype=torch.float32`` runs the same expressions in float32: ``e32``, from which the tests take their bounds, ``bound = max(8 e32, 2e-7 max|want|)`` — the
convention of rows f9 - f11; it is never computed from the code under test.

The uint8 rule (that of tests/rrdb_model.py).  With ``u = (x * 0.5 + 0.5) * 255`` in float64 and ``margin = 8 e32 * 127.5``, a pixel is *strict* when ``u`` is
clamped by more than the margin (``u < 1 - margin`` truncates to 0 on either side of 0; ``u >= 255 + margin``) or lies farther than ``margin`` from an integer.
Strict pixels must equal ``floor(clip(u, 0, 255))``; the others may differ by one.

Mutants whose plain form would not fit the shapes are made to fit in the least invasive way, stated at each."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

FLOOR = 2e-7
MARGIN = 8.0
PIXEL_TOL = 1e-3                             # the default route's bar on generated pixels (tests/test_gpu_synthesis.py)
MUTANT_MARGIN = 10.0                         # every mutant lies at least this many PIXEL_TOL from the fixture on some case
WEIGHT_SEED = 36                             # chosen among seeds 1 - 59: every case's output has a standard deviation of 0.32 - 0.39, at most 2 % outside (-1, 1)
N_MLP = 8
SQRT2 = math.sqrt(2.0)

# tag -> (size, narrow, style_dim, batch)
CASES = {
    "s16": (16, 1 / 32, 32, 2),
    "s32": (32, 1 / 16, 64, 2),
    "s64": (64, 1 / 8, 64, 1),
    "s128": (128, 1 / 4, 512, 1),            # 128-wide levels: 256 input channels, the small-map split-K routes
}
LATENT_CASE = "s32"                          # the case whose latents the fixture stores
MUTANTS = ("cat_swapped", "noise_added", "noise_weight_missing", "noise_not_shifted", "enc_sqrt2_missing", "enc_blur_pad11", "torgb_demodulated",
           "skip_nearest", "lr_mul_ignored", "pixelnorm_missing", "mod_bias_missing")


def bound(e32, want):
    return max(MARGIN * float(e32), FLOOR * float(np.abs(np.asarray(want)).max()))


def max_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


def channels(size, narrow, channel_multiplier=2):
    c = {r: int(512 * narrow) for r in (4, 8, 16, 32)}
    c.update({64: int(256 * channel_multiplier * narrow), 128: int(128 * channel_multiplier * narrow), 256: int(64 * channel_multiplier * narrow),
              512: int(32 * channel_multiplier * narrow), 1024: int(16 * channel_multiplier * narrow)})
    return c


# ------------------------------------------------------------------------------------------------ seeded inputs and weights
def images_u8(seed, bs, size, noise=25):
    """uint8 [bs, size, size, 3]: smooth waves over the whole range plus uniform noise of +-``noise`` grey levels."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    rs = np.random.RandomState(seed)
    img = np.zeros((bs, size, size, 3))
    for b in range(bs):
        for c in range(3):
            fy, fx, ph = rs.uniform(0.5, 3.0), rs.uniform(0.5, 3.0), rs.uniform(0, 6.28)
            img[b, :, :, c] = 127.5 + 130 * np.sin(fy * yy / size * 6.28 + fx * xx / size * 6.28 + ph)
    img += rs.uniform(-noise, noise, img.shape)
    return img.clip(0, 255).astype(np.uint8)


def img2tensor(img_u8, dtype=np.float32):
    """``FaceGAN.img2tensor`` without its flip on a batch: uint8 [bs, H, W, 3] -> [bs, 3, H, W]; each operation rounded to ``dtype``, ``/`` a true division."""
    v = np.asarray(img_u8).astype(dtype) / dtype(255.)
    v = (v - dtype(0.5)) / dtype(0.5)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2))


def tensor2img(x):
    """``FaceGAN.tensor2img`` without its flip on a batch, in the precision of ``x`` as NumPy computes it: [bs, 3, H, W] -> uint8 [bs, H, W, 3]."""
    v = np.asarray(x) * 0.5 + 0.5
    return (np.clip(v.transpose(0, 2, 3, 1), 0, 1) * 255.0).astype(np.uint8)


def to_u(x64):
    """``(x * 0.5 + 0.5) * 255`` before the clamp and the truncation, NHWC."""
    return ((np.asarray(x64, np.float64) * 0.5 + 0.5) * 255.0).transpose(0, 2, 3, 1)


def strict_pixels(u, e32):
    margin = MARGIN * float(e32) * 127.5
    return (u < 1 - margin) | (u >= 255 + margin) | (np.abs(u - np.rint(u)) > margin)


def expected_u8(u):
    return np.floor(np.clip(u, 0, 255)).astype(np.uint8)


def check_u8(got, u, e32):
    """The uint8 rule on ``got`` against the float64 ``u``; returns the strict share."""
    want, strict = expected_u8(u), strict_pixels(u, e32)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert (diff[strict] == 0).all(), f"{int((diff[strict] != 0).sum())} strict pixels differ"
    assert diff.max() <= 1, f"a pixel differs by {int(diff.max())}"
    return float(strict.mean())


_SD = {}


def state_dict(tag):
    size, narrow, sdim, _ = CASES[tag]
    if tag not in _SD:
        _SD[tag] = seeded.seeded_gpen_state_dict(WEIGHT_SEED, size, sdim, N_MLP, 2, narrow)
    return _SD[tag]


# ------------------------------------------------------------------------------------------------ the network
def flrelu(x, bias, scale=SQRT2):
    return F.leaky_relu(x + bias.to(x).view((1, -1) + (1,) * (x.dim() - 2)), 0.2) * scale


def fir(dtype, gain=1.0):
    k = torch.tensor([1., 3., 3., 1.], dtype=torch.float64)
    k = k[None, :] * k[:, None]
    return (k / k.sum() * gain).to(dtype)


def upfirdn(x, k, up, pad):
    """upfirdn2d without downsampling: zeros inserted BEHIND every sample, ``pad = (before, after)`` on both axes, correlation with the flipped kernel."""
    bs, c, h, w = x.shape
    if up > 1:
        z = x.new_zeros(bs, c, h, up, w, up)
        z[:, :, :, 0, :, 0] = x
        x = z.reshape(bs, c, h * up, w * up)
    x = F.pad(x, (pad[0], pad[1], pad[0], pad[1]))
    out = F.conv2d(x.reshape(bs * c, 1, x.shape[2], x.shape[3]), torch.flip(k, [0, 1])[None, None])
    return out.reshape(bs, c, out.shape[2], out.shape[3])


def modconv(sd, p, x, w, up=False, demodulate=True, mutant=None):
    W = sd[p + ".weight"].to(x)[0]                                                # [cout, cin, k, k]
    cout, cin, k, _ = W.shape
    sdim = w.shape[1]
    s = w @ (sd[p + ".modulation.weight"].to(x) * (1 / math.sqrt(sdim))).t()
    if mutant != "mod_bias_missing":
        s = s + sd[p + ".modulation.bias"].to(x)
    Wm = (1 / math.sqrt(cin * k * k)) * W[None] * s[:, None, :, None, None]       # [bs, cout, cin, k, k]
    if demodulate:
        Wm = Wm * torch.rsqrt(Wm.pow(2).sum([2, 3, 4]) + 1e-8)[:, :, None, None, None]
    bs, _, h, wd = x.shape
    xg = x.reshape(1, bs * cin, h, wd)
    if up:
        out = F.conv_transpose2d(xg, Wm.transpose(1, 2).reshape(bs * cin, cout, k, k), stride=2, groups=bs)
        out = out.reshape(bs, cout, out.shape[2], out.shape[3])
        return upfirdn(out, fir(x.dtype, 4.0), 1, (1, 1))
    out = F.conv2d(xg, Wm.reshape(bs * cout, cin, k, k), padding=k // 2, groups=bs)
    return out.reshape(bs, cout, h, wd)


def styled_conv(sd, p, x, w, noise, up=False, mutant=None):
    y = modconv(sd, p + ".conv", x, w, up=up, mutant=mutant)
    if noise.shape[2:] != y.shape[2:]:                                            # (noise_not_shifted: the smaller level's feature, made to fit)
        noise = F.interpolate(noise, size=y.shape[2:], mode="nearest")
    n = noise if mutant == "noise_weight_missing" else sd[p + ".noise.weight"].to(x) * noise
    if mutant == "cat_swapped":
        cat = torch.cat((n, y), 1)
    elif mutant == "noise_added":                                                 # NoiseInjection(isconcat=False) on the first half; the second stays empty
        cat = torch.cat((y + n, torch.zeros_like(n)), 1)
    else:
        cat = torch.cat((y, n), 1)
    return flrelu(cat, sd[p + ".activate.bias"])


def to_rgb(sd, p, x, w, skip, mutant=None):
    out = modconv(sd, p + ".conv", x, w, demodulate=mutant == "torgb_demodulated", mutant=mutant) + sd[p + ".bias"].to(x)
    if skip is not None:
        if mutant == "skip_nearest":
            out = out + F.interpolate(skip, scale_factor=2, mode="nearest")
        else:
            out = out + upfirdn(skip, fir(x.dtype, 4.0), 2, (2, 1))
    return out


def encoder(sd, x, mutant=None):
    """The features [f_size, ..., f4] and the style vector ``final_linear`` makes of f4."""
    log_size = int(round(math.log2(x.shape[2])))
    scale = 1.0 if mutant == "enc_sqrt2_missing" else SQRT2
    feats = []
    W = sd["ecd0.0.0.weight"].to(x)
    x = flrelu(F.conv2d(x, W * (1 / math.sqrt(W.shape[1]))), sd["ecd0.0.1.bias"], scale)
    feats.append(x)
    for i in range(1, log_size - 1):
        W = sd[f"ecd{i}.0.1.weight"].to(x)
        w = W * (1 / math.sqrt(W.shape[1] * 9))
        if mutant == "enc_blur_pad11":                                            # (the convolution then pads by 1 so that the map still halves)
            x = F.conv2d(upfirdn(x, fir(x.dtype), 1, (1, 1)), w, stride=2, padding=1)
        else:
            x = F.conv2d(upfirdn(x, fir(x.dtype), 1, (2, 2)), w, stride=2)
        x = flrelu(x, sd[f"ecd{i}.0.2.bias"], scale)
        feats.append(x)
    W = sd["final_linear.0.weight"].to(x)
    z = flrelu(x.reshape(x.shape[0], -1) @ (W * (1 / math.sqrt(W.shape[1]))).t(), sd["final_linear.0.bias"])
    return feats, z


def style_mlp(sd, z, mutant=None):
    if mutant != "pixelnorm_missing":
        z = z * torch.rsqrt(torch.mean(z ** 2, dim=1, keepdim=True) + 1e-8)
    lr_mul = 1.0 if mutant == "lr_mul_ignored" else 0.01
    i = 1
    while f"generator.style.{i}.weight" in sd:
        W = sd[f"generator.style.{i}.weight"].to(z)
        z = flrelu(z @ (W * ((1 / math.sqrt(W.shape[1])) * lr_mul)).t(), sd[f"generator.style.{i}.bias"].to(z) * lr_mul)
        i += 1
    return z


def network(sd, x, dtype=torch.float64, mutant=None, return_latents=False):
    """``FullGenerator.forward``: ``x`` an array or tensor ``[bs, 3, size, size]``; returns a tensor of ``dtype`` (and the latent ``[bs, n_latent, style_dim]``)."""
    x = torch.as_tensor(x).to(dtype)
    with torch.no_grad():
        feats, z = encoder(sd, x, mutant)
        w = style_mlp(sd, z, mutant)
        noise = [f for f in feats[::-1] for _ in (0, 1)]                          # [f4, f4, f8, f8, ..., f_size, f_size]
        if mutant == "noise_not_shifted":                                         # ([1:] dropped where the channel counts allow; the map is made to fit)
            noise = [lo if lo.shape[1] == hi.shape[1] else hi for lo, hi in zip(noise, noise[1:])]
        else:
            noise = noise[1:]
        g = "generator."
        out = sd[g + "input.input"].to(x).repeat(x.shape[0], 1, 1, 1)
        out = styled_conv(sd, g + "conv1", out, w, noise[0], mutant=mutant)
        skip = to_rgb(sd, g + "to_rgb1", out, w, None, mutant)
        for j in range(len(feats) - 1):
            out = styled_conv(sd, f"{g}convs.{2 * j}", out, w, noise[1 + 2 * j], up=True, mutant=mutant)
            out = styled_conv(sd, f"{g}convs.{2 * j + 1}", out, w, noise[2 + 2 * j], mutant=mutant)
            skip = to_rgb(sd, f"{g}to_rgbs.{j}", out, w, skip, mutant)
    if return_latents:
        return skip, w[:, None].repeat(1, 2 * len(feats), 1)
    return skip


# ------------------------------------------------------------------------------------------------ cases
_CASE = {}


def case_image(tag):
    size, _, _, bs = CASES[tag]
    return images_u8(sum(map(ord, tag)), bs, size)


def case(tag):
    """dict(sd, img, x, want, latent, e32, e32_latent, u) of a case, made once: seeded weights, uint8 image, its float32 tensor, the float64 output and latent,
    the float32 model's errors, the float64 value before the uint8 truncation."""
    if tag not in _CASE:
        sd = state_dict(tag)
        img = case_image(tag)
        x = img2tensor(img)
        want, latent = network(sd, x, return_latents=True)
        got32, lat32 = network(sd, x, torch.float32, return_latents=True)
        want, latent = want.numpy(), latent.numpy()
        _CASE[tag] = dict(sd=sd, img=img, x=x, want=want, latent=latent, e32=max_err(got32.numpy(), want), e32_latent=max_err(lat32.numpy(), latent),
                          u=to_u(want))
    return _CASE[tag]
