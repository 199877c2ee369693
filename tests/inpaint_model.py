"""The GCFSR inpainting generator (row f25) restated directly, in float64 or float32: ``FaceInpaintingArch.forward`` of swap_face_fine/gcfsr_arch.py in eval mode
with explicit noise, the two ends of ``inpainting()`` (swap_face_fine/face_inpainting.py), the arithmetic of the five kernels of csrc/gcfsr.hip in numpy float32,
the seeded inputs and cases of the tests and single-change mutants of the network.  Written from the architecture's description, not by importing the
reference; ``tests/golden/g35_inpaint.npz`` holds what the reference's own module gives on the same cases.

    flrelu(v)  = leaky_relu(v + bias, 0.2) * sqrt(2);  blur = upfirdn2d with outer([1, 3, 3, 1]) / 64
    encoder    f_S = flrelu(conv3x3(x [4 planes], W / sqrt(36), pad 1)); f_{r/2} = flrelu(conv3x3(blur(f_r, pad (2, 2)), W / sqrt(9 cin), stride 2)) down to 16
    condition  per level r = S .. 16: s1 = w1 c + b1, s2 = w2 c + b2 (c = the hole share), shift_r = conv3x3(f_r, W / sqrt(9 C), pad 1) + b; lists reversed
    latent     flrelu(flat(down(down(f_16))) @ (W / sqrt(4096))^T) viewed [num_latent, 512]
    StyleConv  flrelu(modconv(x, latent[i]) + weight * noise)                                  (the up layers: conv_transpose stride 2, blur pad (1, 1), 4 x kernel)
    norm layer y = modconv(x, latent[i]) + weight * noise; n = s1^2 + s2^2 + 1e-8; flrelu(y * s1 rsqrt(n) + shift * s2 rsqrt(n))
    ToRGB      1 x 1 modconv without demodulation + bias + upfirdn2d(skip, 4 x kernel, up 2, pad (2, 1)); latent rows 1, then 2 j + 3
    ends       x = float32(byte / 255.) * (1 - m), m; out = round((x (1 - m) + clamp(net, 0, 1) m) * 255), half to even

``dtype=torch.float32`` runs the same expressions in float32: ``e32``, from which the tests take their bounds with ``gpen_model.bound``.

The uint8 rule (``gpen_model.check_u8`` restated for rounding boundaries at k + 0.5).  With ``u = v * 255`` in float64 and ``margin = 8 e32 * 255``, a pixel is
*strict* when it lies outside the hole or ``u`` lies farther than ``margin`` from every k + 0.5 (the clamp is 1-Lipschitz: it widens no error).  Strict pixels
must equal ``rint(u)``; the others may differ by one.  Outside the hole the input bytes come back exactly.

Mutants whose plain form would not fit the shapes are made to fit in the least invasive way, stated at each."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

import gpen_model as GM

FLOOR, MARGIN, PIXEL_TOL, MUTANT_MARGIN = GM.FLOOR, GM.MARGIN, GM.PIXEL_TOL, GM.MUTANT_MARGIN
bound, max_err = GM.bound, GM.max_err
WEIGHT_SEED = 7
SQRT2 = math.sqrt(2.0)
SDIM = 512

# tag -> (size, batch)
CASES = {"i32": (32, 2), "i64": (64, 1), "i256": (256, 1)}
MUTANTS = ("scales_swapped", "norm2scale_missing", "shift_after_act", "cond_not_reversed", "noise_after_scaling", "cond_bias_missing", "shift_bias_missing",
           "enc_sqrt2_missing", "torgb_row_i1", "mask_plane_missing", "stored_noise_upsampled")
SAMPLES = 4096                               # what the fixture keeps of an array over 16384 elements
# (source side, network side): the copy, the exact 2 : 1, three ragged pairs (up, down, down past 2 : 1)
MASK_PAIRS = ((32, 32, 32), (64, 64, 32), (23, 29, 32), (50, 37, 32), (97, 70, 32))


def noise_sizes(size):
    return [16] + [2 ** i for i in range(5, int(math.log2(size)) + 1) for _ in (0, 1)]


# ------------------------------------------------------------------------------------------------ seeded inputs and weights
_SD = {}


def state_dict(size):
    if size not in _SD:
        _SD[size] = seeded.seeded_inpaint_state_dict(WEIGHT_SEED, size)
    return _SD[size]


def hole_masks(tag):
    """uint8 0/1 [bs, S, S]: an ellipse off the centre for the first sample, an EMPTY hole for the second of a batch (distinct hole shares)."""
    size, bs = CASES[tag]
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    m = np.zeros((bs, size, size), np.uint8)
    m[0] = (((yy - 0.55 * size) / (0.3 * size)) ** 2 + ((xx - 0.45 * size) / (0.22 * size)) ** 2 < 1).astype(np.uint8)
    return m


def case_noise(tag):
    size, bs = CASES[tag]
    return [seeded.seeded_array(sum(map(ord, tag)), f"inpaint.noise.{i}", (bs, 1, r, r), dist="normal") for i, r in enumerate(noise_sizes(size))]


# ------------------------------------------------------------------------------------------------ the five kernels' arithmetic, numpy float32
def input_model(faces_u8, hole_u8):
    """(x float32 [n, 4, S, S], in_size float32 [n], count int32 [n]) as e4s_gcfsr_input forms them."""
    faces_u8, hole = np.asarray(faces_u8), np.asarray(hole_u8) != 0
    v = (faces_u8.astype(np.float64) / 255.0).astype(np.float32).transpose(0, 3, 1, 2)
    x = np.concatenate([np.where(hole[:, None], np.float32(0), v), hole[:, None].astype(np.float32)], 1)
    count = hole.reshape(len(hole), -1).sum(1).astype(np.int32)
    S = faces_u8.shape[1]
    return np.ascontiguousarray(x), (count.astype(np.float32) / np.float32(S * S)).astype(np.float32), count


def condition_model(in_size, levels):
    """(s1n, s2n) float32 [bs, sum C] as e4s_gcfsr_condition forms them; ``levels``: per level (w1 [C, 1], b1 [C], w2, b2) float32 arrays."""
    f = np.float32
    c = np.asarray(in_size, f).reshape(-1, 1)
    o1, o2 = [], []
    for w1, b1, w2, b2 in levels:
        s1 = (np.asarray(w1, f).reshape(1, -1) * c).astype(f) + np.asarray(b1, f)[None]
        s2 = (np.asarray(w2, f).reshape(1, -1) * c).astype(f) + np.asarray(b2, f)[None]
        n = ((s1 * s1).astype(f) + (s2 * s2).astype(f)).astype(f) + f(1e-8)
        r = (f(1) / np.sqrt(n.astype(f))).astype(f)
        o1.append((s1 * r).astype(f))
        o2.append((s2 * r).astype(f))
    return np.concatenate(o1, 1), np.concatenate(o2, 1)


def scale_shift_act_model(y, shift, s1n, s2n, bias):
    """e4s_gcfsr_scale_shift_act in numpy float32, every operation rounded on its own."""
    f = np.float32
    y, shift = np.asarray(y, f), np.asarray(shift, f)
    t = (y * np.asarray(s1n, f)[:, :, None, None]).astype(f) + (shift * np.asarray(s2n, f)[:, :, None, None]).astype(f)
    t = (t.astype(f) + np.asarray(bias, f)[None, :, None, None]).astype(f)
    t = np.where(t < 0, (t * f(0.2)).astype(f), t)
    return (t * f(SQRT2)).astype(f)


def tail_model(img, faces_u8, hole_u8):
    """e4s_gcfsr_tail in numpy float32: uint8 [n, S, S, 3]."""
    f = np.float32
    hole = (np.asarray(hole_u8) != 0)[..., None]
    x = (np.asarray(faces_u8).astype(np.float64) / 255.0).astype(f)
    o = np.clip(np.asarray(img, f), f(0), f(1)).transpose(0, 2, 3, 1)
    v = np.where(hole, o, x)
    return np.rint((v * f(255.0)).astype(f)).astype(np.uint8)


def _support_axis(src, dst, area):
    d = np.arange(dst, dtype=np.float64)
    if area:
        return (2 * d).astype(np.int64), np.full(dst, 2, np.int64)
    fx = ((d + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5).astype(np.float32)
    s = np.floor(fx).astype(np.int64)
    fx = fx - s.astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    fx = np.where(lo | hi, np.float32(0), fx)
    return s, 1 + (fx != 0).astype(np.int64)


def mask_support_model(mask, S):
    """The table rule of e4s_cv_mask_support: uint8 0/1 [bs, S, S]."""
    mask = np.asarray(mask)
    bs, H, W = mask.shape
    area = H == 2 * S and W == 2 * S
    ys, yc = _support_axis(H, S, area)
    xs, xc = _support_axis(W, S, area)
    pos = mask > 0
    out = np.zeros((bs, S, S), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = np.minimum(ys + dy, H - 1), np.minimum(xs + dx, W - 1)
            ok = (dy < yc)[:, None] & (dx < xc)[None, :]
            out |= pos[:, yy][:, :, xx] & ok[None]
    return out.astype(np.uint8)


def mask_support_brute(mask, S):
    """``cv2.resize(mask.astype(float64), (S, S)) > 0`` by brute force in float64: the copy, the 2 x 2 block mean at the exact 2 : 1, otherwise the bilinear blend
    with OpenCV's float32 coordinate and its clamps at both borders, every output pixel formed on its own."""
    m = np.asarray(mask).astype(np.float64)
    bs, H, W = m.shape
    out = np.zeros((bs, S, S), np.float64)
    if (H, W) == (S, S):
        out = m.copy()
    elif (H, W) == (2 * S, 2 * S):
        out = m.reshape(bs, S, 2, S, 2).mean((2, 4))
    else:
        def coord(d, src):
            f = np.float32((d + 0.5) * (np.float64(src) / np.float64(S)) - 0.5)
            s = int(np.floor(f))
            f = np.float32(f - np.float32(s))
            if s < 0:
                s, f = 0, np.float32(0)
            if s >= src - 1:
                s, f = src - 1, np.float32(0)
            return s, float(f)
        for y in range(S):
            sy, fy = coord(y, H)
            for x in range(S):
                sx, fx = coord(x, W)
                y1, x1 = min(sy + 1, H - 1), min(sx + 1, W - 1)
                out[:, y, x] = ((1 - fy) * ((1 - fx) * m[:, sy, sx] + fx * m[:, sy, x1]) + fy * ((1 - fx) * m[:, y1, sx] + fx * m[:, y1, x1]))
    return (out > 0).astype(np.uint8)


def mask_case(seed, H, W, soft):
    """A [2, H, W] mask: random blobs, 0/1 uint8 or soft non-negative float32 (zeros kept exact)."""
    rs = np.random.RandomState(seed)
    m = (rs.uniform(size=(2, H, W)) < 0.08).astype(np.float32)
    m[1, : H // 3] = 0
    if soft:
        return (m * rs.uniform(1e-3, 3.0, size=m.shape)).astype(np.float32)
    return m.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the network
def flrelu(x, bias, scale=SQRT2):
    return F.leaky_relu(x + bias.to(x).view((1, -1) + (1,) * (x.dim() - 2)), 0.2) * scale


fir, upfirdn = GM.fir, GM.upfirdn


def conv_layer(sd, p, x, down=False, activate=True, scale=SQRT2, bias=True):
    i = 1 if down else 0
    W = sd[f"{p}.{i}.weight"].to(x)
    w = W * (1 / math.sqrt(W.shape[1] * 9))
    y = F.conv2d(upfirdn(x, fir(x.dtype), 1, (2, 2)), w, stride=2) if down else F.conv2d(x, w, padding=1)
    if activate:
        return flrelu(y, sd[f"{p}.{i + 1}.bias"], scale)
    return y + sd[f"{p}.{i}.bias"].to(x).view(1, -1, 1, 1) if bias else y


def modconv(sd, p, x, w, up=False, demodulate=True):
    W = sd[p + ".weight"].to(x)[0]
    cout, cin, k, _ = W.shape
    s = w @ (sd[p + ".modulation.weight"].to(x) * (1 / math.sqrt(w.shape[1]))).t() + sd[p + ".modulation.bias"].to(x)
    Wm = (1 / math.sqrt(cin * k * k)) * W[None] * s[:, None, :, None, None]
    if demodulate:
        Wm = Wm * torch.rsqrt(Wm.pow(2).sum([2, 3, 4]) + 1e-8)[:, :, None, None, None]
    bs, _, h, wd = x.shape
    xg = x.reshape(1, bs * cin, h, wd)
    if up:
        out = F.conv_transpose2d(xg, Wm.transpose(1, 2).reshape(bs * cin, cout, k, k), stride=2, groups=bs)
        return upfirdn(out.reshape(bs, cout, out.shape[2], out.shape[3]), fir(x.dtype, 4.0), 1, (1, 1))
    return F.conv2d(xg, Wm.reshape(bs * cout, cin, k, k), padding=k // 2, groups=bs).reshape(bs, cout, h, wd)


def style_conv(sd, p, x, w, noise, up=False, cond=None, mutant=None):
    y = modconv(sd, p + ".modulated_conv", x, w, up)
    n = sd[p + ".weight"].to(x) * noise
    bias = sd[p + ".activate.bias"]
    if cond is None:
        return flrelu(y + n, bias)
    s1, s2, shift = cond
    if mutant == "scales_swapped":
        s1, s2 = s2, s1
    if mutant != "norm2scale_missing":
        r = torch.rsqrt(s1 ** 2 + s2 ** 2 + 1e-8)
        s1, s2 = s1 * r, s2 * r
    s1, s2 = s1.view(-1, y.shape[1], 1, 1), s2.view(-1, y.shape[1], 1, 1)
    if mutant == "shift_after_act":
        return flrelu((y + n) * s1, bias) + shift * s2
    if mutant == "noise_after_scaling":
        return flrelu(y * s1 + shift * s2 + n, bias)
    return flrelu((y + n) * s1 + shift * s2, bias)


def to_rgb(sd, p, x, w, skip):
    out = modconv(sd, p + ".modulated_conv", x, w, demodulate=False) + sd[p + ".bias"].to(x)
    if skip is not None:
        out = out + upfirdn(skip, fir(x.dtype, 4.0), 2, (2, 1))
    return out


def network(sd, x, in_size, noise, dtype=torch.float64, mutant=None, return_latents=False):
    """``FaceInpaintingArch.forward(x, in_size, noise=noise)``: ``x`` an array ``[bs, 4, S, S]``, ``in_size [bs]``, ``noise`` a list of arrays; returns a tensor of
    ``dtype`` (and the latent ``[bs, num_latent, 512]``)."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    c = torch.as_tensor(np.asarray(in_size)).to(dtype).reshape(-1, 1)
    noise = [torch.as_tensor(np.asarray(n)).to(dtype) for n in noise]
    bs, size = x.shape[0], x.shape[2]
    n_cond = int(math.log2(size)) - 3
    enc_scale = 1.0 if mutant == "enc_sqrt2_missing" else SQRT2
    with torch.no_grad():
        if mutant == "mask_plane_missing":
            x = torch.cat([x[:, :3], torch.zeros_like(x[:, 3:])], 1)
        if mutant == "stored_noise_upsampled":                                    # the stored buffers (4, 8, 8, 16, ...) made to fit by nearest upsampling
            noise = [F.interpolate(sd[f"noises.noise{i}"].to(dtype), size=n.shape[2:], mode="nearest").expand_as(n) for i, n in enumerate(noise)]
        feat = conv_layer(sd, "conv_body_first", x, scale=enc_scale)
        cond = []
        for j in range(n_cond):
            if j:
                feat = conv_layer(sd, f"conv_body_down.{j - 1}", feat, down=True, scale=enc_scale)
            s = []
            for k in (1, 2):
                v = c @ sd[f"condition_scale{k}.{j}.weight"].to(x).t()
                s.append(v if mutant == "cond_bias_missing" else v + sd[f"condition_scale{k}.{j}.bias"].to(x))
            cond.append((s[0], s[1], conv_layer(sd, f"condition_shift.{j}", feat, activate=False, bias=mutant != "shift_bias_missing")))
        good = cond[::-1]
        if mutant == "cond_not_reversed":       # level j takes the other end's entries where the channel counts allow; the shift map is made to fit (nearest)
            cond = [(o[0], o[1], F.interpolate(o[2], size=g[2].shape[2:], mode="nearest")) if o[2].shape[1] == g[2].shape[1] else g for o, g in zip(cond, good)]
        else:
            cond = good
        tmp = conv_layer(sd, "final_down2", conv_layer(sd, "final_down1", feat, down=True, scale=enc_scale), down=True, scale=enc_scale)
        W = sd["final_linear.weight"].to(x)
        latent = flrelu(tmp.reshape(bs, -1) @ (W * (1 / math.sqrt(W.shape[1]))).t(), sd["final_linear.bias"]).view(bs, -1, SDIM)
        out = conv_layer(sd, "final_conv", feat, scale=enc_scale)
        out = style_conv(sd, "style_conv1", out, latent[:, 0], noise[0], cond=cond[0], mutant=mutant)
        skip = to_rgb(sd, "to_rgb1", out, latent[:, 1], None)
        for j in range(n_cond - 1):
            out = style_conv(sd, f"style_convs.{2 * j}", out, latent[:, 2 * j + 1], noise[2 * j + 1], up=True)
            out = style_conv(sd, f"style_convs.{2 * j + 1}", out, latent[:, 2 * j + 2], noise[2 * j + 2], cond=cond[j + 1], mutant=mutant)
            skip = to_rgb(sd, f"to_rgbs.{j}", out, latent[:, 2 * j + (2 if mutant == "torgb_row_i1" else 3)], skip)
    return (skip, latent) if return_latents else skip


# ------------------------------------------------------------------------------------------------ the uint8 rule, boundaries at k + 0.5
def composite(want, faces_u8, hole_u8):
    """``v`` before the rounding, float64 [n, S, S, 3]: the input outside the hole (its float32 value), the clamped network output inside."""
    hole = (np.asarray(hole_u8) != 0)[..., None]
    x = (np.asarray(faces_u8).astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    return np.where(hole, np.clip(np.asarray(want, np.float64).transpose(0, 2, 3, 1), 0, 1), x)


def check_u8(got, want, faces_u8, hole_u8, e32):
    """The uint8 rule on ``got`` against the float64 network output ``want``; returns the strict share."""
    hole = np.broadcast_to((np.asarray(hole_u8) != 0)[..., None], got.shape)
    u = composite(want, faces_u8, hole_u8) * 255.0                                # (the clamp is 1-Lipschitz: an error of the network moves u by no more)
    margin = MARGIN * float(e32) * 255.0
    strict = ~hole | (np.abs(u - np.floor(u) - 0.5) > margin)
    expected = np.rint(u).astype(np.int32)
    diff = np.abs(got.astype(np.int32) - expected)
    assert (got[~hole] == np.asarray(faces_u8)[~hole]).all(), "a pixel outside the hole changed"
    assert (diff[strict] == 0).all(), f"{int((diff[strict] != 0).sum())} strict pixels differ"
    assert diff.max() <= 1, f"a pixel differs by {int(diff.max())}"
    return float(strict.mean())


# ------------------------------------------------------------------------------------------------ cases and the fixture's sampling
_CASE = {}


def case(tag):
    """dict(sd, faces, hole, x, in_size, noise, want, latent, e32, e32_latent) of a case, made once: seeded weights, uint8 faces and hole masks, the network's input, the
    seeded noise, the float64 output and latent, the float32 model's error."""
    if tag not in _CASE:
        size, bs = CASES[tag]
        sd = state_dict(size)
        faces, hole = GM.images_u8(sum(map(ord, tag)), bs, size), hole_masks(tag)
        x, in_size, _ = input_model(faces, hole)
        noise = case_noise(tag)
        want, latent = network(sd, x, in_size, noise, return_latents=True)
        got32, lat32 = network(sd, x, in_size, noise, torch.float32, return_latents=True)
        want, latent = want.numpy(), latent.numpy()
        _CASE[tag] = dict(sd=sd, faces=faces, hole=hole, x=x, in_size=in_size, noise=noise, want=want, latent=latent, e32=max_err(got32.numpy(), want),
                          e32_latent=max_err(lat32.numpy(), latent))
    return _CASE[tag]


def sample_stride(n):
    """1 for an array the fixture stores whole; otherwise an odd stride that spreads SAMPLES picks over the flat index."""
    return 1 if n <= 16384 else (n // SAMPLES) | 1


def sampled(a):
    """What the fixture keeps of ``a``, in ``a``'s own precision."""
    a = np.asarray(a)
    s = sample_stride(a.size)
    return a if s == 1 else a.reshape(-1)[::s][:SAMPLES]


def stored(a):
    return sampled(a).astype(np.float32)


def hole_inside_share(out, hole_u8):
    """The share of the raw output values inside the hole that lie strictly inside (0, 1)."""
    hole = np.broadcast_to((np.asarray(hole_u8) != 0)[:, None], out.shape)
    v = np.asarray(out)[hole]
    return float(((v > 0) & (v < 1)).mean())
