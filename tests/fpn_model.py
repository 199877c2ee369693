"""The feature networks of the Blender recolouring network (row f10) restated directly, in float64 or float32, with the seeded inputs and cases of their
fixture (``tests/golden/g22_fpn.npz``) and tests, single-change mutants of the model, and the operations of the two kernels of ``csrc/spade.hip`` alone.

    w(conv)          = weight_orig / (u . W_mat v)                         spectral norm in eval mode: no power iteration
    inorm(x)         = (x - mean) / sqrt(biased var + 1e-5)                per sample and channel
    encoder          x = inorm(conv(leaky0.2(x))) for layer1..5 (3x3, zero padding 1, strides 1 2 1 2 1, no bias), no activation before layer1 or after layer5
    spade(x, img)    = inorm(x) * (1 + gamma) + beta;  seg = nearest(img, size of x);  actv = relu(conv3x3(reflpad1(seg)));  gamma, beta = conv3x3(reflpad1(actv))
    block            x_s = conv_s(spade_s(x)) (1x1, only when the width changes, else x);  dx = conv_0(reflpad1(leaky(spade_0(x))));
                     dx = conv_1(reflpad1(leaky(spade_1(dx))));  out = x_s + dx
    network          head_0 (512 -> 512), G_middle_0 (512 -> 512), G_middle_1 (512 -> 256) after the encoder
    SmallFPN         conv2(conv1(x)), two 1x1 stride-2 convolutions with bias
    features         feats_a = fpn(img_a);  feats_t = fpn(flip(img_t, -1)) when flipped, NOT flipped back

``dtype=torch.float32`` runs the same expressions in float32 — the reference's arithmetic class: ``e32``, from which the tests take their bounds
(``bound = max(8 e32, 2e-7 max|want|)``: row f9's form and factor; the floor is three float32 ulps at the output's size)."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

FLOOR = 2e-7
MARGIN = 8.0
MUTANT_MARGIN = 10.0                         # every mutant moves the float64 output by at least this many bounds on some case
EPS = 1e-5
WEIGHT_SEED = 22
LAYERS = (("layer1", 1), ("layer2", 2), ("layer3", 1), ("layer4", 2), ("layer5", 1))
BLOCKS = (("head_0", False), ("G_middle_0", False), ("G_middle_1", True))            # (name, learned shortcut)

# tag -> (H, W, batch, small)
CASES = {
    "8x8.b2": (8, 8, 2, False),              # feature map 2 x 2: reflection reads index 1 and 0
    "20x12": (20, 12, 1, False),             # 5 x 3
    "34x26.b3": (34, 26, 3, False),          # 17 x 13 -> 9 x 7: odd sizes through both stride-2 layers
    "256x256": (256, 256, 1, False),         # the workload's own shape, once
    "30x22.b2.small": (30, 22, 2, True),     # SmallFPN: 15 x 11 -> 8 x 6
}
SAMPLED = {"256x256": 8192}                  # the fixture holds this many seeded positions of the output instead of all of it
SMALL_CASES = tuple(t for t in CASES if t not in SAMPLED)
# what BlenderInfer builds its network from: the defaults of get_base_parser() + add_hyper (utils/parser.py, inference.py:19-32), eval_only set
PARSER_DEFAULTS = dict(norm_G="spectralspadeinstance3x3", norm_E="spectralinstance", eqlr_sn=False, adaptor_kernel=3, warp_stride=4, ngf=64,
                       adaptor_nonlocal=False, adaptor_se=False, adaptor_res_deeper=False, dilation_conv=False, PONO=False, PONO_C=False,
                       CBN_intype="warp_mask", small_FPN=False, eval_only=True, lambda_CYC=1.0, lambda_CYC2=10.0)
MUTANTS = ("gamma_for_one_plus_gamma", "zero_padding", "nearest_rounds", "slope_0.1", "sigma_left_out", "unbiased_variance", "eps_1e-3",
           "activation_after_layer5", "features_flipped_back")


def bound(e32, want):
    return max(MARGIN * float(e32), FLOOR * float(np.abs(want).max()))


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)


# ------------------------------------------------------------------------------------------------ seeded inputs and weights
def images(seed, bs, H, W):
    """float32 [bs, 3, H, W] of ImageNet-normalised scale: smooth ramps plus noise, so that neighbouring pixels differ and a wrong pick shows."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.sin(0.37 * yy[None, None] + rs.uniform(0, 6, (bs, 3, 1, 1))) + np.cos(0.23 * xx[None, None] + rs.uniform(0, 6, (bs, 3, 1, 1)))
    return (0.8 * ramp + 0.6 * rs.randn(bs, 3, H, W)).astype(np.float32)


def case_inputs(tag):
    H, W, bs, _ = CASES[tag]
    return images(2000 + 7 * H + W + bs, bs, H, W)


_SD = {}


def state_dict(small=False, seed=WEIGHT_SEED):
    if (small, seed) not in _SD:
        _SD[small, seed] = seeded.seeded_small_fpn_state_dict(seed) if small else seeded.seeded_fpn_state_dict(seed)
    return _SD[small, seed]


def sample_positions(tag):
    """Flat positions into the case's output [bs, 256, h, w] that the fixture records (seeded, ascending, distinct)."""
    H, W, bs, _ = CASES[tag]
    h, w = out_size(H, W)
    return np.sort(np.random.RandomState(78).choice(bs * 256 * h * w, SAMPLED[tag], replace=False))


def out_size(H, W):
    return ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1


# ------------------------------------------------------------------------------------------------ the operations
def reflpad1(x, mutant=None):
    return F.pad(x, (1, 1, 1, 1)) if mutant == "zero_padding" else F.pad(x, (1, 1, 1, 1), mode="reflect")


def nearest_index(out, inp, mutant=None):
    """PyTorch's 'nearest' source index: floor(dst * scale) with scale = in / out formed in float32, clamped."""
    scale = np.float32(inp) / np.float32(out)
    pos = np.arange(out, dtype=np.float32) * scale
    idx = np.rint(pos) if mutant == "nearest_rounds" else np.floor(pos)
    return torch.from_numpy(np.minimum(idx.astype(np.int64), inp - 1))


def nearest(img, h, w, mutant=None):
    return img[:, :, nearest_index(h, img.shape[2], mutant)][:, :, :, nearest_index(w, img.shape[3], mutant)]


def inorm(x, mutant=None):
    mean = x.mean(dim=(2, 3), keepdim=True)
    var = x.var(dim=(2, 3), keepdim=True, unbiased=mutant == "unbiased_variance")
    return (x - mean) / torch.sqrt(var + (1e-3 if mutant == "eps_1e-3" else EPS))


def leaky(x, mutant=None):
    return F.leaky_relu(x, 0.1 if mutant == "slope_0.1" else 0.2)


def sn_weight(sd, p, dtype, mutant=None):
    w = sd[p + ".weight_orig"].to(dtype)
    if mutant == "sigma_left_out":
        return w
    return w / torch.dot(sd[p + ".weight_u"].to(dtype), torch.mv(w.reshape(w.shape[0], -1), sd[p + ".weight_v"].to(dtype)))


def shared_mlp(sd, p, img, h, w, mutant=None):
    """relu(conv3x3(reflpad1(nearest(img)))) of the norm ``p``: [bs, 128, h, w]."""
    return torch.relu(F.conv2d(reflpad1(nearest(img, h, w, mutant), mutant), sd[p + ".mlp_shared.1.weight"].to(img.dtype), sd[p + ".mlp_shared.1.bias"].to(img.dtype)))


def spade(sd, p, x, img, mutant=None):
    actv = reflpad1(shared_mlp(sd, p, img, x.shape[2], x.shape[3], mutant), mutant)
    gamma = F.conv2d(actv, sd[p + ".mlp_gamma.weight"].to(x.dtype), sd[p + ".mlp_gamma.bias"].to(x.dtype))
    beta = F.conv2d(actv, sd[p + ".mlp_beta.weight"].to(x.dtype), sd[p + ".mlp_beta.bias"].to(x.dtype))
    return inorm(x, mutant) * (gamma if mutant == "gamma_for_one_plus_gamma" else 1 + gamma) + beta


def block(sd, p, x, img, learned, mutant=None):
    x_s = F.conv2d(spade(sd, p + ".norm_s", x, img, mutant), sn_weight(sd, p + ".conv_s", x.dtype, mutant)) if learned else x
    dx = F.conv2d(reflpad1(leaky(spade(sd, p + ".norm_0", x, img, mutant), mutant), mutant), sn_weight(sd, p + ".conv_0", x.dtype, mutant),
                  sd[p + ".conv_0.bias"].to(x.dtype))
    dx = F.conv2d(reflpad1(leaky(spade(sd, p + ".norm_1", dx, img, mutant), mutant), mutant), sn_weight(sd, p + ".conv_1", x.dtype, mutant),
                  sd[p + ".conv_1.bias"].to(x.dtype))
    return x_s + dx


def forward(sd, img, dtype=torch.float64, mutant=None):
    """A feature network (which one is read off the keys) on ``img`` (array or tensor ``[bs, 3, H, W]``) in ``dtype``; a float64 array ``[bs, 256, h, w]``.
    ``features_flipped_back`` is a mutant of ``features``, not of this function."""
    assert mutant is None or mutant in MUTANTS
    with torch.no_grad():
        img = torch.as_tensor(img).to(dtype)
        if "conv1.weight" in sd:
            x = F.conv2d(img, sd["conv1.weight"].to(dtype), sd["conv1.bias"].to(dtype), stride=2)
            return F.conv2d(x, sd["conv2.weight"].to(dtype), sd["conv2.bias"].to(dtype), stride=2).double().numpy()
        x = img
        for i, (name, stride) in enumerate(LAYERS):
            if i:
                x = leaky(x, mutant)
            x = inorm(F.conv2d(x, sn_weight(sd, name + ".0", dtype, mutant), None, stride=stride, padding=1), mutant)
        if mutant == "activation_after_layer5":
            x = leaky(x)
        for name, learned in BLOCKS:
            x = block(sd, name, x, img, learned, mutant)
        return x.double().numpy()


def features(sd, img_a, img_t, flip, dtype=torch.float64, mutant=None):
    """``(feats_a, feats_t)`` of ``Referencer.forward``: the target mirrored before its features are taken when ``flip``, the features left as they come."""
    feats_t = forward(sd, np.ascontiguousarray(np.asarray(img_t)[..., ::-1]) if flip else img_t, dtype, mutant)
    if flip and mutant == "features_flipped_back":
        feats_t = np.ascontiguousarray(feats_t[..., ::-1])
    return forward(sd, img_a, dtype, mutant), feats_t


def modulate(x, mean, rstd, gamma_beta, leaky_slope, padded):
    """The modulation kernel's operation in float64 on float32 inputs: ``(value, magnitude)``; the magnitude is |x - mean| rstd |1 + gamma| + |beta|, the size
    of the terms its roundings are relative to."""
    x, mean, rstd = (np.asarray(a, np.float64) for a in (x, mean, rstd))
    bs, C, h, w = x.shape
    n = (x - mean.reshape(bs, C, 1, 1)) * rstd.reshape(bs, C, 1, 1)
    mag = np.abs(n)
    if gamma_beta is not None:
        gb = np.asarray(gamma_beta, np.float64)
        n, mag = n * (1 + gb[:, :C]) + gb[:, C:], mag * np.abs(1 + gb[:, :C]) + np.abs(gb[:, C:])
    v = np.where(n > 0, n, n * leaky_slope)
    if padded:
        v, mag = (np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="reflect") for a in (v, mag))
    return v, mag


_OUT = {}


def reference_output(tag, dtype=torch.float64, mutant=None):
    """The model's output of a named case, computed once per session and shared (do not write into the array)."""
    key = (tag, dtype, mutant)
    if key not in _OUT:
        _OUT[key] = forward(state_dict(CASES[tag][3]), case_inputs(tag), dtype, mutant)
    return _OUT[key]


def max_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())


def e32(tag):
    """The float32 model against the float64 model on the case."""
    return max_err(reference_output(tag, torch.float32), reference_output(tag))
