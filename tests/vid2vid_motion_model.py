"""Row f18: face-vid2vid's ``DenseMotionNetwork`` (swap_face_fine/face_vid2vid/modules/dense_motion.py with ``Hourglass``, ``kp2gaussian`` and
``make_coordinate_grid`` of modules/util.py) restated in float64, the cases of tests/golden/g29_vid2vid_motion.npz, and single-change mutants.  Not a test
module: test_vid2vid_motion_cpu.py and test_gpu_vid2vid_motion.py import it, and so does tests/golden/make_golden_vid2vid_motion.py.

The network is read off the keys of a state_dict alone (``hourglass.encoder.down_blocks.<i>``, ``hourglass.decoder.up_blocks.<i>``, ``occlusion`` where there
is one), never off the code under test.  The bar of a case and output is ``vid2vid_kp_model.bound(e32, want) = max(8 e32, 2e-7 max|want|)`` with ``e32`` the
model in float32 against itself in float64."""
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded
from vid2vid_kp_model import BN_EPS, MUTANT_MARGIN, _bn, _conv, bound, grid_xyz, max_err  # noqa: F401

WEIGHT_SEED = 18
KP_VARIANCE = 0.01

# tag -> (DenseMotionNetwork configuration, feature shape, Jacobians in the keypoint dicts, (std of the source keypoints, of driving - source))
CASES = {
    "D-A": (dict(block_expansion=8, num_blocks=3, max_features=32, num_kp=5, feature_channel=8, reshape_depth=4, compress=4, estimate_occlusion_map=True),
            (2, 8, 4, 16, 16), False, (0.35, 0.3)),
    "D-B": (dict(block_expansion=6, num_blocks=2, max_features=24, num_kp=3, feature_channel=5, reshape_depth=3, compress=2, estimate_occlusion_map=True),
            (1, 5, 3, 8, 24), True, (0.3, 0.2)),                              # an odd depth, W above one 16-wide tile, Jacobians
    "D-C": (dict(block_expansion=8, num_blocks=2, max_features=32, num_kp=5, feature_channel=8, reshape_depth=3, compress=4, estimate_occlusion_map=False),
            (1, 8, 3, 12, 20), False, (0.35, 0.3)),                            # no occlusion head; 12 x 20: ragged tiles
    "D-D": (dict(block_expansion=4, num_blocks=1, max_features=16, num_kp=20, feature_channel=6, reshape_depth=4, compress=2, estimate_occlusion_map=True),
            (1, 6, 4, 8, 20), True, (0.25, 0.15)),                              # 21 mask outputs: the ragged 32-channel form of the 7-tap kernel
}
OUTPUTS = ("mask", "deformation", "occlusion_map")
INTERMEDIATES = ("compressed", "input", "sparse", "logits", "prediction")
# mutant -> (the case it is held to, the output it is read on)
MUTANTS = {
    "align_corners_true": ("D-A", "mask"), "border_padding": ("D-A", "mask"), "grid_zyx": ("D-C", "deformation"), "kp_variance_01": ("D-A", "mask"),
    "heatmap_source_minus_driving": ("D-A", "mask"), "background_heatmap_nonzero": ("D-C", "mask"), "feature_then_heatmap": ("D-A", "mask"),
    "jac_d_inv_s": ("D-B", "deformation"), "jacobian_after_kp_s": ("D-B", "deformation"), "softmax_over_depth": ("D-A", "mask"),
    "deformation_without_background": ("D-C", "deformation"), "pool_before_relu": ("D-B", "mask"), "skip_in_front": ("D-A", "mask"),
    "depth_pool_and_up": ("D-D", "mask"), "bn_eps_1e3": ("D-B", "mask"), "sigmoid_missing": ("D-A", "occlusion_map"), "k7_pad_2": ("D-D", "mask"),
}


def _hourglass(sd, x, eps, m):
    deep = m == "depth_pool_and_up"                           # nearest upsampling in depth too (and, to keep the shapes, the pooling)
    outs, i = [x], 0
    while f"hourglass.encoder.down_blocks.{i}.conv.weight" in sd:
        p = f"hourglass.encoder.down_blocks.{i}"
        y = _bn(sd, p + ".norm", _conv(sd, p + ".conv", outs[-1], padding=1), eps)
        pool = (2, 2, 2) if deep else (1, 2, 2)
        outs.append(F.relu(F.avg_pool3d(y, pool)) if m == "pool_before_relu" else F.avg_pool3d(F.relu(y), pool))
        i += 1
    out, j = outs.pop(), 0
    while f"hourglass.decoder.up_blocks.{j}.conv.weight" in sd:
        p = f"hourglass.decoder.up_blocks.{j}"
        out = F.interpolate(out, scale_factor=(2, 2, 2) if deep else (1, 2, 2))
        out = F.relu(_bn(sd, p + ".norm", _conv(sd, p + ".conv", out, padding=1), eps))
        skip = outs.pop()
        out = torch.cat([skip, out] if m == "skip_in_front" else [out, skip], dim=1)
        j += 1
    return F.relu(_bn(sd, "hourglass.decoder.norm", _conv(sd, "hourglass.decoder.conv", out, padding=1), eps))


def hourglass_input(f, kd, ks, jd=None, js=None, m=None):
    """(hourglass input [bs, (K + 1)(c + 1), d, h, w], sparse motions [bs, K + 1, d, h, w, 3]) of the compressed feature ``f`` and the keypoints, in f's dtype."""
    bs, c, d, h, w = f.shape
    K = kd.shape[1]
    grid = grid_xyz(d, h, w, f.dtype, "grid_zyx" if m == "grid_zyx" else None).view(1, 1, d, h, w, 3)
    kdv, ksv = kd.view(bs, K, 1, 1, 1, 3), ks.view(bs, K, 1, 1, 1, 3)
    motion = grid - kdv
    if m == "jacobian_after_kp_s":
        motion = motion + ksv
    if jd is not None:
        jac = jd @ torch.linalg.inv(js) if m == "jac_d_inv_s" else js @ torch.linalg.inv(jd)
        motion = (jac.view(bs, K, 1, 1, 1, 3, 3) @ motion.unsqueeze(-1)).squeeze(-1)
    if m != "jacobian_after_kp_s":
        motion = motion + ksv
    sparse = torch.cat([grid.expand(bs, -1, -1, -1, -1, -1), motion], dim=1)
    deformed = F.grid_sample(f.unsqueeze(1).expand(-1, K + 1, -1, -1, -1, -1).reshape(bs * (K + 1), c, d, h, w), sparse.reshape(bs * (K + 1), d, h, w, 3),
                             mode="bilinear", padding_mode="border" if m == "border_padding" else "zeros",
                             align_corners=m == "align_corners_true").view(bs, K + 1, c, d, h, w)
    var = 0.1 if m == "kp_variance_01" else KP_VARIANCE
    gauss = lambda kp: torch.exp(-0.5 * ((grid - kp) ** 2).sum(-1) / var)      # noqa: E731
    heat = gauss(ksv) - gauss(kdv) if m == "heatmap_source_minus_driving" else gauss(kdv) - gauss(ksv)
    back = torch.ones_like(heat[:, :1]) if m == "background_heatmap_nonzero" else torch.zeros_like(heat[:, :1])
    heat = torch.cat([back, heat], dim=1).unsqueeze(2)
    return torch.cat([deformed, heat] if m == "feature_then_heatmap" else [heat, deformed], dim=2).view(bs, -1, d, h, w), sparse


def combine(logits, sparse, m=None):
    """(mask, deformation) of the mask head's logits and the sparse motions."""
    mask = F.softmax(logits, dim=2 if m == "softmax_over_depth" else 1)
    weighted = sparse.permute(0, 1, 5, 2, 3, 4) * mask.unsqueeze(2)
    if m == "deformation_without_background":
        weighted = weighted[:, 1:]
    return mask, weighted.sum(dim=1).permute(0, 2, 3, 4, 1)


def dm_network(sd, feature, kp_d, kp_s, jac_d=None, jac_s=None, dtype=torch.float64, mutant=None):
    """``DenseMotionNetwork.forward`` in eval mode: dict(mask, deformation, occlusion_map or None, and the intermediates compressed, input, sparse, logits,
    prediction) as tensors of ``dtype``."""
    m = mutant
    T = lambda a: None if a is None else torch.as_tensor(a).to(dtype)      # noqa: E731
    x, kd, ks, jd, js = T(feature), T(kp_d), T(kp_s), T(jac_d), T(jac_s)
    eps = 1e-3 if m == "bn_eps_1e3" else BN_EPS
    with torch.no_grad():
        bs, _, d, h, w = x.shape
        f = F.relu(_bn(sd, "norm", _conv(sd, "compress", x), eps))
        inp, sparse = hourglass_input(f, kd, ks, jd, js, m)
        prediction = _hourglass(sd, inp, eps, m)
        if m == "k7_pad_2":                                   # two zeros in front, four behind: every tap one position off
            logits = _conv(sd, "mask", F.pad(prediction, (2, 4, 2, 4, 2, 4)))
        else:
            logits = _conv(sd, "mask", prediction, padding=3)
        mask, deformation = combine(logits, sparse, m)
        occ = None
        if "occlusion.weight" in sd:
            occ = _conv(sd, "occlusion", prediction.reshape(bs, -1, h, w), padding=3)
            if m != "sigmoid_missing":
                occ = torch.sigmoid(occ)
        return dict(mask=mask, deformation=deformation, occlusion_map=occ, compressed=f, input=inp, sparse=sparse, logits=logits, prediction=prediction)


# ------------------------------------------------------------------------------------------------ the cases
def config(tag):
    return dict(CASES[tag][0])


def make_module(tag):
    """The mirror module of a case (the code under test's: its keys are checked against the reference's in test_vid2vid_motion_cpu.py)."""
    from e4s2024_amd import ops
    return ops.DenseMotionNetwork(**config(tag)).eval()


_SD, _CASE = {}, {}


def state_dict(tag):
    if tag not in _SD:
        with torch.device("meta"):
            template = make_module(tag).state_dict()
        _SD[tag] = seeded.seeded_dense_motion_state_dict(template, WEIGHT_SEED)
    return _SD[tag]


def case_inputs(tag):
    """(feature, kp_d, kp_s, jac_d, jac_s) as float32 arrays: a smooth volume plus noise; keypoints inside the cube with source and driving a few tenths
    apart, which sends a part of every sparse motion outside [-1, 1]; Jacobians near the identity (condition number below 10)."""
    cfg, (bs, C, D, H, W), jac, (spread, apart) = CASES[tag]
    K = cfg["num_kp"]
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, D), np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    rs = np.random.RandomState(sum(map(ord, tag)) + 18)
    feature = np.empty((bs, C, D, H, W))
    for b in range(bs):
        for ch in range(C):
            fz, fy, fx, ph = rs.uniform(0.3, 1.2), rs.uniform(0.5, 2.0), rs.uniform(0.5, 2.0), rs.uniform(0, 2 * np.pi)
            feature[b, ch] = np.sin(np.pi * (fz * zz + fy * yy + fx * xx) + ph)
    feature = (feature + seeded.seeded_array(WEIGHT_SEED, tag + ".feature", feature.shape, 0.0, 0.5, "normal")).astype(np.float32)
    kp_s = seeded.seeded_array(WEIGHT_SEED, tag + ".kp_s", (bs, K, 3), 0.0, spread).astype(np.float32)
    kp_d = (kp_s + seeded.seeded_array(WEIGHT_SEED, tag + ".kp_d", (bs, K, 3), 0.0, apart)).astype(np.float32)
    jac_d = jac_s = None
    if jac:
        eye = np.eye(3, dtype=np.float32)[None, None]
        jac_d = (eye + seeded.seeded_array(WEIGHT_SEED, tag + ".jac_d", (bs, K, 3, 3), 0.0, 0.15)).astype(np.float32)
        jac_s = (eye + seeded.seeded_array(WEIGHT_SEED, tag + ".jac_s", (bs, K, 3, 3), 0.0, 0.15)).astype(np.float32)
    return feature, kp_d, kp_s, jac_d, jac_s


def case(tag):
    """dict of a case, made once: ``sd``, the inputs ``feature``, ``kp_d``, ``kp_s``, ``jac_d``, ``jac_s`` (float32 arrays or None), ``out64`` (the float64
    model's outputs and intermediates as arrays) and ``e32`` (the float32 model's errors per array)."""
    if tag not in _CASE:
        sd = state_dict(tag)
        feature, kp_d, kp_s, jac_d, jac_s = case_inputs(tag)
        o64 = dm_network(sd, feature, kp_d, kp_s, jac_d, jac_s)
        o32 = dm_network(sd, feature, kp_d, kp_s, jac_d, jac_s, dtype=torch.float32)
        names = [k for k in OUTPUTS + INTERMEDIATES if o64[k] is not None]
        _CASE[tag] = dict(sd=sd, feature=feature, kp_d=kp_d, kp_s=kp_s, jac_d=jac_d, jac_s=jac_s, out64={k: o64[k].numpy() for k in names},
                          e32={k: max_err(o32[k].numpy(), o64[k].numpy()) for k in names})
    return _CASE[tag]


def kp_dicts(tag, to=torch.from_numpy):
    """(kp_driving, kp_source) of a case as the network takes them."""
    c = case(tag)
    kd, ks = {"value": to(c["kp_d"])}, {"value": to(c["kp_s"])}
    if c["jac_d"] is not None:
        kd["jacobian"], ks["jacobian"] = to(c["jac_d"]), to(c["jac_s"])
    return kd, ks


def check_conditions(tag, outputs):
    """The conditions that keep a pass from being empty, on a case's outputs (the reference's or the model's); returns figures to print."""
    c = case(tag)
    K = CASES[tag][0]["num_kp"]
    sparse = c["out64"]["sparse"]
    outside = float((np.abs(sparse) > 1).any(-1).mean())
    assert 0.05 <= outside <= 0.5, (tag, outside)                 # the zero padding is exercised without dominating
    count = float((1.0 / (np.asarray(outputs["mask"], dtype=np.float64) ** 2).sum(1)).mean())
    assert 1.5 <= count <= (K + 1) / 2, (tag, count)              # the softmax neither one-hot nor uniform
    info = dict(outside=outside, count=count)
    if outputs.get("occlusion_map") is not None:
        occ = outputs["occlusion_map"]
        info["occlusion"] = (float(occ.min()), float(occ.max()))
        assert occ.min() <= 0.2 and occ.max() >= 0.8, (tag, info["occlusion"])
    if c["jac_d"] is not None:
        cond = max(float(np.linalg.cond(c[k].astype(np.float64)).max()) for k in ("jac_d", "jac_s"))
        info["cond"] = cond
        assert cond <= 10, (tag, cond)
    for k in OUTPUTS:
        if c["out64"].get(k) is not None:
            assert c["e32"][k] <= 1e-4 * c["out64"][k].std(), (tag, k, c["e32"][k], c["out64"][k].std())
    return info


def mutant_output(m):
    """The float64 model with the single change ``m`` on its case: the array of the output it is read on."""
    tag, name = MUTANTS[m]
    c = case(tag)
    return dm_network(c["sd"], c["feature"], c["kp_d"], c["kp_s"], c["jac_d"], c["jac_s"], mutant=m)[name].numpy()
