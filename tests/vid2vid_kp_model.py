"""Row f17: face-vid2vid's ``KPDetector`` and ``HEEstimator`` (swap_face_fine/face_vid2vid/modules/keypoint_detector.py, modules/util.py) and
``keypoint_transformation`` (drive_demo.py:67-180) restated in float64, the cases of tests/golden/g28_vid2vid_kp.npz, and single-change mutants.  Not a test
module: test_vid2vid_kp_cpu.py and test_gpu_vid2vid_kp.py import it, and so does tests/golden/make_golden_vid2vid_kp.py.

The networks are read off the keys of a state_dict alone (``predictor.down_blocks.down<i>``, ``predictor.up_blocks.up<i>``, ``block<j>.b<j>_<i>``, a ``skip``
where there is one), never off the code under test; what no key holds (temperature, scale factor, depth) comes from the case's configuration.  The bar of a case
and output is ``max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against itself in float64."""
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

FLOOR = 2e-7
MARGIN = 8.0
MUTANT_MARGIN = 100.0                        # every mutant lies at least this many bars from the fixture on its named case
WEIGHT_SEED = 17
BN_EPS = 1e-5
NUM_BINS = 66

# tag -> (KPDetector configuration, (bs, H, W))
KP_CASES = {
    "K-A": (dict(block_expansion=8, max_features=32, num_blocks=3, reshape_depth=4, reshape_channel=128, num_kp=5, scale_factor=0.25, estimate_jacobian=True),
            (2, 64, 64)),                                     # volume (4, 16, 16)
    "K-B": (dict(block_expansion=12, max_features=48, num_blocks=2, reshape_depth=3, reshape_channel=144, num_kp=15, scale_factor=1, estimate_jacobian=False),
            (1, 24, 40)),                                     # 24 and 48 channels, an odd depth, volume (3, 24, 40)
    "K-C": (dict(block_expansion=8, max_features=16, num_blocks=1, reshape_depth=2, reshape_channel=32, num_kp=3, scale_factor=0.25, estimate_jacobian=True),
            (3, 52, 36)),                                     # anti-alias 13 x 9, pooled with flooring to 6 x 4, volume (2, 12, 8)
}
# tag -> (num_kp, (bs, H, W))
HE_CASES = {
    "H-A": (15, (2, 64, 64)),
    "H-B": (5, (1, 40, 56)),                                  # 20 x 28 -> 10 x 14 -> 5 x 7 -> 3 x 4 -> 2 x 2: every stride-2 layer on an odd size
    "H-C": (3, (1, 32, 32)),                                  # the last map is 1 x 1
}
# tag -> (head outputs of, keypoints of (their first sample where the batches differ), free_view angles or None)
T_CASES = {
    "T-A": ("H-A", "K-B", None),                              # one canonical set (no Jacobian) for a batch of two frames
    "T-B": ("H-B", "K-A", None),
    "T-C": ("H-C", "K-C", None),
    "T-hand": ("hand", "K-A", None),                          # hand-made rows: degrees near -60 and +60
    "T-free": ("H-A", "K-B", (20.0, -35.0, None)),            # free_view: fixed yaw and pitch, the roll of the logits
}
CASES = {**KP_CASES, **HE_CASES, **T_CASES}
KP_OUTPUTS, HE_OUTPUTS, T_OUTPUTS = ("value", "jacobian"), ("yaw", "pitch", "roll", "t", "exp"), ("value", "jacobian", "deg", "rot")
STORED_VOLUME = "K-A"                                         # the one case whose logits and heatmap the fixture holds
# mutant -> (the case it is held to, the output it is read on)
MUTANTS = {
    "heads_uncrossed": ("H-A", "yaw"), "pi": ("T-hand", "value"), "roll_pitch_yaw": ("T-hand", "value"), "minus_96": ("T-hand", "value"),
    "temperature_dropped": ("K-A", "value"), "softmax_per_slice": ("K-A", "value"), "grid_half_pixel": ("K-A", "value"), "grid_zyx": ("K-A", "value"),
    "trilinear_up": ("K-A", "value"), "depth_up": ("K-C", "value"), "maxpool_down": ("K-C", "value"), "aa_no_zero_pad": ("K-C", "value"),
    "aa_sigma_2": ("K-A", "value"), "aa_from_2": ("K-A", "value"), "bn_eps_1e3": ("K-B", "value"), "he_bn_eps_1e3": ("H-B", "exp"),
    "relu_after_add_dropped": ("H-C", "exp"), "skip_norm4_dropped": ("H-B", "exp"), "exp_before_rotation": ("T-B", "value"),
    "jacobian_from_the_right": ("T-B", "jacobian"),
}


def bound(e32, want):
    return max(MARGIN * float(e32), FLOOR * float(np.abs(np.asarray(want)).max()))


def max_err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


def images_u8(seed, bs, H, W, noise=40):
    """uint8 [bs, 3, H, W]: smooth waves over the whole range plus uniform noise; the float32 image is ``img / 255`` (in [0, 1], as the callers feed it)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rs = np.random.RandomState(seed)
    out = np.empty((bs, 3, H, W))
    for b in range(bs):
        for c in range(3):
            fy, fx, ph = rs.uniform(0.5, 2.5), rs.uniform(0.5, 2.5), rs.uniform(0, 2 * np.pi)
            out[b, c] = 127.5 + 90 * np.sin(2 * np.pi * (fy * yy / H + fx * xx / W) + ph)
    return np.clip(out + rs.uniform(-noise, noise, out.shape), 0, 255).astype(np.uint8)


def to_float(img_u8):
    return (np.asarray(img_u8).astype(np.float32) / np.float32(255)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ shared layers
def _bn(sd, p, y, eps=BN_EPS):
    v = lambda k: sd[f"{p}.{k}"].to(y).view((1, -1) + (1,) * (y.dim() - 2))      # noqa: E731
    return (y - v("running_mean")) / torch.sqrt(v("running_var") + eps) * v("weight") + v("bias")


def _conv(sd, p, x, **kw):
    fn = F.conv3d if sd[p + ".weight"].dim() == 5 else F.conv2d
    return fn(x, sd[p + ".weight"].to(x), sd[p + ".bias"].to(x), **kw)


# ------------------------------------------------------------------------------------------------ KPDetector
def _gaussian(k, sigma, dtype):
    ax = torch.arange(k, dtype=dtype)
    g = torch.exp(-(ax - (k - 1) / 2) ** 2 / (2 * sigma ** 2))
    kern = g[:, None] * g[None, :]
    return kern / kern.sum()


def _antialias(sd, x, scale, m):
    s = int(round(1 / scale))
    kern = sd["down.weight"].to(x)                       # the module's own float32 buffer: data, like any weight
    k = kern.shape[-1]
    if m == "aa_sigma_2":
        kern = _gaussian(k, 2.0, x.dtype).view(1, 1, k, k).repeat(x.shape[1], 1, 1, 1)
    pad = F.pad(x, (k // 2,) * 4, mode="replicate") if m == "aa_no_zero_pad" else F.pad(x, (k // 2,) * 4)
    out = F.conv2d(pad, kern, groups=x.shape[1])
    first = 2 if m == "aa_from_2" else 0
    return out[:, :, first::s, first::s]


def grid_xyz(D, H, W, dtype, m=None):
    """make_coordinate_grid: 2 i / (n - 1) - 1 per axis, stacked in (x, y, z) order: [D, H, W, 3]."""
    if m == "grid_half_pixel":
        ax = lambda n: (2 * torch.arange(n, dtype=dtype) + 1) / n - 1      # noqa: E731
    else:
        ax = lambda n: 2 * (torch.arange(n, dtype=dtype) / (n - 1)) - 1    # noqa: E731
    x, y, z = ax(W).view(1, 1, W).expand(D, H, W), ax(H).view(1, H, 1).expand(D, H, W), ax(D).view(D, 1, 1).expand(D, H, W)
    return torch.stack((z, y, x) if m == "grid_zyx" else (x, y, z), 3)


def heatmap_expectation(prediction, jac_planes, temperature, m=None):
    """(heatmap, value, jacobian or None) of logits [bs, K, D, H, W] (and planes [bs, 9 K, D, H, W]) in their dtype."""
    bs, K, D, H, W = prediction.shape
    logits = prediction if m == "temperature_dropped" else prediction / temperature
    if m == "softmax_per_slice":
        heat = F.softmax(logits.reshape(bs, K, D, -1), dim=3).view(bs, K, D, H, W) / D
    else:
        heat = F.softmax(logits.reshape(bs, K, -1), dim=2).view(bs, K, D, H, W)
    value = (heat.unsqueeze(-1) * grid_xyz(D, H, W, prediction.dtype, m)[None, None]).sum(dim=(2, 3, 4))
    jac = None
    if jac_planes is not None:
        jac = (heat.unsqueeze(2) * jac_planes.reshape(bs, K, 9, D, H, W)).reshape(bs, K, 9, -1).sum(-1).view(bs, K, 3, 3)
    return heat, value, jac


def kp_network(sd, x, cfg, dtype=torch.float64, mutant=None):
    """``KPDetector.forward`` in eval mode: dict(value, jacobian or None, prediction, heatmap) as tensors of ``dtype``."""
    m = mutant
    x = torch.as_tensor(x).to(dtype)
    eps = 1e-3 if m == "bn_eps_1e3" else BN_EPS
    with torch.no_grad():
        if cfg["scale_factor"] != 1:
            x = _antialias(sd, x, cfg["scale_factor"], m)
        i = 0
        while f"predictor.down_blocks.down{i}.conv.weight" in sd:
            p = f"predictor.down_blocks.down{i}"
            x = F.relu(_bn(sd, p + ".norm", _conv(sd, p + ".conv", x, padding=1), eps))
            x = F.max_pool2d(x, 2) if m == "maxpool_down" else F.avg_pool2d(x, 2)
            i += 1
        x = _conv(sd, "predictor.conv", x)
        bs, c, h, w = x.shape
        depth = cfg["reshape_depth"]
        x = x.view(bs, c // depth, depth, h, w)
        i = 0
        while f"predictor.up_blocks.up{i}.conv.weight" in sd:
            p = f"predictor.up_blocks.up{i}"
            if m == "trilinear_up":
                x = F.interpolate(x, scale_factor=(1, 2, 2), mode="trilinear")
            else:
                x = F.interpolate(x, scale_factor=(2, 2, 2) if m == "depth_up" else (1, 2, 2))
            x = F.relu(_bn(sd, p + ".norm", _conv(sd, p + ".conv", x, padding=1), eps))
            i += 1
        prediction = _conv(sd, "kp", x, padding=1)
        planes = _conv(sd, "jacobian", x, padding=1) if "jacobian.weight" in sd else None
        heat, value, jac = heatmap_expectation(prediction, planes, cfg["temperature"], m)
        return dict(value=value, jacobian=jac, prediction=prediction, heatmap=heat)


# ------------------------------------------------------------------------------------------------ HEEstimator
def _bottleneck(sd, p, x, eps, m):
    stride = 2 if p + ".skip.weight" in sd else 1
    out = F.relu(_bn(sd, p + ".norm1", _conv(sd, p + ".conv1", x), eps))
    out = F.relu(_bn(sd, p + ".norm2", _conv(sd, p + ".conv2", out, padding=1, stride=stride), eps))
    out = _bn(sd, p + ".norm3", _conv(sd, p + ".conv3", out), eps)
    if stride != 1:
        x = _conv(sd, p + ".skip", x, stride=stride)
        if m != "skip_norm4_dropped":
            x = _bn(sd, p + ".norm4", x, eps)
    out = out + x
    return out if m == "relu_after_add_dropped" else F.relu(out)


def he_network(sd, x, dtype=torch.float64, mutant=None):
    """``HEEstimator.forward`` in eval mode: dict(yaw, pitch, roll, t, exp), the head names crossed as the reference crosses them."""
    m = mutant
    x = torch.as_tensor(x).to(dtype)
    eps = 1e-3 if m == "he_bn_eps_1e3" else BN_EPS
    lin = lambda p, v: F.linear(v, sd[p + ".weight"].to(v), sd[p + ".bias"].to(v))      # noqa: E731
    with torch.no_grad():
        out = F.max_pool2d(F.relu(_bn(sd, "norm1", _conv(sd, "conv1", x, padding=3, stride=2), eps)), 3, 2, 1)
        out = F.relu(_bn(sd, "norm2", _conv(sd, "conv2", out), eps))
        for i in range(3):
            out = _bottleneck(sd, f"block1.b1_{i}", out, eps, m)
        for j, n in ((3, 3), (4, 5), (5, 2)):                 # conv3 / block2 / block3 x 3, conv4 / block4 / block5 x 5, conv5 / block6 / block7 x 2
            out = F.relu(_bn(sd, f"norm{j}", _conv(sd, f"conv{j}", out), eps))
            out = _bottleneck(sd, f"block{2 * j - 4}", out, eps, m)
            for i in range(n):
                out = _bottleneck(sd, f"block{2 * j - 3}.b{2 * j - 3}_{i}", out, eps, m)
        out = out.mean(dim=(2, 3))
        a, b = ("fc_yaw", "fc_roll") if m == "heads_uncrossed" else ("fc_roll", "fc_yaw")
        return dict(yaw=lin(a, out), pitch=lin("fc_pitch", out), roll=lin(b, out), t=lin("fc_t", out), exp=lin("fc_exp", out))


# ------------------------------------------------------------------------------------------------ keypoint_transformation
def degrees(row, dtype=torch.float64, m=None):
    p = F.softmax(torch.as_tensor(row).to(dtype), dim=1)
    return (p * torch.arange(NUM_BINS, dtype=dtype)).sum(1) * 3 - (96 if m == "minus_96" else 99)


def rotation(yaw, pitch, roll, m=None):
    pi = np.pi if m == "pi" else 3.14
    yaw, pitch, roll = (a / 180 * pi for a in (yaw, pitch, roll))
    o, z = torch.ones_like(yaw), torch.zeros_like(yaw)
    mat = lambda *e: torch.stack(e, 1).view(-1, 3, 3)      # noqa: E731
    P = mat(o, z, z, z, torch.cos(pitch), -torch.sin(pitch), z, torch.sin(pitch), torch.cos(pitch))
    Y = mat(torch.cos(yaw), z, torch.sin(yaw), z, o, z, -torch.sin(yaw), z, torch.cos(yaw))
    R = mat(torch.cos(roll), -torch.sin(roll), z, torch.sin(roll), torch.cos(roll), z, z, z, o)
    return R @ P @ Y if m == "roll_pitch_yaw" else P @ Y @ R


def transform(kp_value, kp_jac, he, fixed=None, dtype=torch.float64, mutant=None):
    """``keypoint_transformation``: dict(value, jacobian or None, deg [bs, 3], rot); ``fixed``: free_view's (yaw, pitch, roll), None keeps the logits'."""
    m = mutant
    T = lambda a: torch.as_tensor(a).to(dtype)      # noqa: E731
    deg = [degrees(he[k], dtype, m) for k in ("yaw", "pitch", "roll")]
    if fixed is not None:
        deg = [d if f is None else torch.full_like(d, f) for d, f in zip(deg, fixed)]
    rot = rotation(*deg, m=m)
    kp, t, exp = T(kp_value), T(he["t"]).view(-1, 1, 3), T(he["exp"])
    exp = exp.view(exp.shape[0], -1, 3)
    if m == "exp_before_rotation":
        value = torch.einsum("bmp,bkp->bkm", rot, kp + exp) + t
    else:
        value = torch.einsum("bmp,bkp->bkm", rot, kp.expand(rot.shape[0], -1, -1)) + t + exp
    jac = None
    if kp_jac is not None:
        j = T(kp_jac).expand(rot.shape[0], -1, -1, -1)
        jac = torch.einsum("bkms,bsp->bkmp", j, rot) if m == "jacobian_from_the_right" else torch.einsum("bmp,bkps->bkms", rot, j)
    return dict(value=value, jacobian=jac, deg=torch.stack(deg, 1), rot=rot)


# ------------------------------------------------------------------------------------------------ the cases
def kp_config(tag):
    return dict(feature_channel=32, image_channel=3, temperature=0.1, **KP_CASES[tag][0])


def he_config(tag):
    return dict(block_expansion=64, feature_channel=32, num_kp=HE_CASES[tag][0], image_channel=3, max_features=2048, num_bins=NUM_BINS)


def make_module(tag):
    """The mirror module of a case (the code under test's: its keys are checked against the reference's in test_vid2vid_kp_cpu.py)."""
    from e4s2024_amd import ops
    return (ops.KPDetector(**kp_config(tag)) if tag in KP_CASES else ops.HEEstimator(**he_config(tag))).eval()


_SD, _CASE = {}, {}


def state_dict(tag):
    if tag not in _SD:
        with torch.device("meta"):
            template = make_module(tag).state_dict()
        fn = seeded.seeded_kp_detector_state_dict if tag in KP_CASES else seeded.seeded_he_estimator_state_dict
        _SD[tag] = fn(template, WEIGHT_SEED)
    return _SD[tag]


def case_image(tag):
    bs, H, W = CASES[tag][1]
    return images_u8(sum(map(ord, tag)) + 17, bs, H, W)


def hand_he(bs=2, K=5):
    """Hand-made head outputs: logit rows peaked near bins 13 and 53 (-60 and +60 degrees) and between, seeded ``t`` and ``exp``."""
    idx = np.arange(NUM_BINS, dtype=np.float64)
    peak = lambda c, w: (-(idx - c) ** 2 / (2 * w ** 2)).astype(np.float32)      # noqa: E731
    rows = dict(yaw=np.stack([peak(13.2, 1.5), peak(52.7, 2.0)]), pitch=np.stack([peak(53.1, 1.2), peak(30.4, 3.0)]),
                roll=np.stack([peak(24.6, 2.5), peak(12.9, 1.4)]))
    rows["t"] = seeded.seeded_array(WEIGHT_SEED, "hand.t", (bs, 3), 0.0, 0.3)
    rows["exp"] = seeded.seeded_array(WEIGHT_SEED, "hand.exp", (bs, 3 * K), 0.0, 0.1)
    return rows


def _errs(f32, f64, names):
    return {k: max_err(f32[k].numpy(), f64[k].numpy()) for k in names if f64.get(k) is not None}


def case(tag):
    """dict of a case, made once.  K and H cases: ``sd``, ``img`` (uint8), ``x`` (float32), ``out64`` (the float64 model's outputs as arrays) and ``e32`` (the
    float32 model's errors per output).  T cases: ``he`` and ``kp`` / ``jac`` (float32 arrays: inputs), ``fixed``, ``out64``, ``e32``."""
    if tag in _CASE:
        return _CASE[tag]
    if tag in T_CASES:
        he_tag, kp_tag, fixed = T_CASES[tag]
        kc = case(kp_tag)
        he = hand_he() if he_tag == "hand" else {k: v.astype(np.float32) for k, v in case(he_tag)["out64"].items()}
        bs = he["yaw"].shape[0]
        n = kc["out64"]["value"].shape[0]
        sel = slice(0, n if n == bs else 1)
        kp = kc["out64"]["value"][sel].astype(np.float32)
        jac = None if kc["out64"]["jacobian"] is None else kc["out64"]["jacobian"][sel].astype(np.float32)
        c = dict(he=he, kp=kp, jac=jac, fixed=fixed)
        c.update(transform_outputs(c))
        _CASE[tag] = c
        return c
    sd, img = state_dict(tag), case_image(tag)
    x = to_float(img)
    if tag in KP_CASES:
        cfg = kp_config(tag)
        o64, o32 = kp_network(sd, x, cfg), kp_network(sd, x, cfg, dtype=torch.float32)
        names = KP_OUTPUTS + ("prediction", "heatmap")
    else:
        o64, o32 = he_network(sd, x), he_network(sd, x, dtype=torch.float32)
        names = HE_OUTPUTS
    _CASE[tag] = dict(sd=sd, img=img, x=x, out64={k: (None if o64.get(k) is None else o64[k].numpy()) for k in names}, e32=_errs(o32, o64, names))
    return _CASE[tag]


def transform_outputs(c, he=None, kp=None, jac=None):
    """``out64`` and ``e32`` of the transformation on the given float32 inputs (default: the T case's own)."""
    he, kp, jac = he or c["he"], c["kp"] if kp is None else kp, c["jac"] if jac is None else jac
    o64, o32 = transform(kp, jac, he, c["fixed"]), transform(kp, jac, he, c["fixed"], dtype=torch.float32)
    return dict(out64={k: (None if o64[k] is None else o64[k].numpy()) for k in T_OUTPUTS}, e32=_errs(o32, o64, T_OUTPUTS))


def effective_support(p, axis=None):
    """1 / sum p^2 of distributions along ``axis`` (all trailing axes of a [bs, K, ...] heatmap by default)."""
    p = np.asarray(p, dtype=np.float64)
    if axis is None:
        p = p.reshape(p.shape[0], p.shape[1], -1)
        axis = 2
    return 1.0 / (p ** 2).sum(axis)


def softmax(row):
    e = np.exp(np.asarray(row, dtype=np.float64) - np.asarray(row, dtype=np.float64).max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def check_conditions(tag, outputs, heatmap=None):
    """The conditions that keep a pass from being empty, on a case's outputs (the reference's or the model's); returns figures to print."""
    c = case(tag)
    info = {}
    if tag in KP_CASES:
        if heatmap is not None:
            n = int(np.prod(heatmap.shape[2:]))
            sup = effective_support(heatmap)
            info["support"] = (float(sup.min()), float(sup.max()), n)
            assert 8 <= sup.min() and sup.max() <= n / 4, (tag, sup.min(), sup.max(), n)
        names = KP_OUTPUTS
    elif tag in HE_CASES:
        deg = []
        for k in ("yaw", "pitch", "roll"):
            sup = effective_support(softmax(outputs[k]), axis=-1)
            assert sup.min() >= 3, (tag, k, sup.min())
            deg.append(degrees(outputs[k]).numpy())
        deg = np.stack(deg)
        info["degrees"] = (float(deg.min()), float(deg.max()))
        assert deg.max() - deg.min() >= 20, (tag, deg)
        names = HE_OUTPUTS
    else:
        names = T_OUTPUTS
    for k in names:
        if c["out64"].get(k) is not None:
            assert c["e32"][k] <= 1e-4 * c["out64"][k].std(), (tag, k, c["e32"][k], c["out64"][k].std())
    return info


def mutant_output(m):
    """The float64 model with the single change ``m`` on its case: the array of the output it is read on."""
    tag, name = MUTANTS[m]
    c = case(tag)
    if tag in KP_CASES:
        return kp_network(c["sd"], c["x"], kp_config(tag), mutant=m)[name].numpy()
    if tag in HE_CASES:
        return he_network(c["sd"], c["x"], mutant=m)[name].numpy()
    return transform(c["kp"], c["jac"], c["he"], c["fixed"], mutant=m)[name].numpy()
