"""Row f16 (the RealESRNet pass of GPEN's ``FaceEnhancement.process``, the resize of the frame, the drop-ins) without a GPU: the mirror module's keys, the
restatement ``gpen_sr_model`` against what the reference's own code gave (tests/golden/g27_gpen_sr.npz), the fixed-point resize on cases checked by hand, the
bars of the GPU tests pinned from the other side by single-change mutants, the conditioning of the seeded cases, the names, the drop-ins and the argument
errors that must raise before any launch.

The bound of a case is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64; uint8 images follow the model's uint8 rule."""
import os

import numpy as np
import pytest
import torch

import gpen_paste_model as PM
import gpen_sr_model as M
from conftest import GOLDEN

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_gsr_input", "e4s_gsr_tail", "e4s_cv_resize_linear_u8"}
NAMES = ("GPEN_SR_FEATS", "GPEN_SR_SCALES", "GpenSRNet", "PreparedGpenSRNet", "gpen_sr_state_dict_shapes", "gpen_sr_weight_tensors", "gpen_sr_output_size",
         "gpen_sr_forward", "gpen_sr_image", "cv_resize_linear")
MUTANT_LEVEL = 1.0 / 255.0                   # one grey level of a uint8 end, in the float range [0, 1]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "g27_gpen_sr.npz")) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ the mirror module
@pytest.mark.parametrize("scale,cin", [(4, 3), (2, 12), (1, 48)])
@pytest.mark.parametrize("nf", [32, 64])
def test_mirror_has_the_keys_of_the_checkpoint(scale, cin, nf):
    from e4s2024_amd import ops
    sd = ops.GpenSRNet(2, nf, scale).state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert list(ops.gpen_sr_state_dict_shapes(2, nf, scale).items()) == list(shapes.items()) and len(sd) == 72
    want = {"conv_first": (nf, cin), "conv_body": (nf, nf), "conv_up1": (nf, nf), "conv_up2": (nf, nf), "conv_hr": (nf, nf), "conv_last": (3, nf)}
    for i in range(2):
        for r in (1, 2, 3):
            for k in range(1, 6):
                want[f"body.{i}.rdb{r}.conv{k}"] = (32 if k < 5 else nf, nf + 32 * (k - 1))
    assert shapes == {f"{p}.{s}": ((co, ci, 3, 3) if s == "weight" else (co,)) for p, (co, ci) in want.items() for s in ("weight", "bias")}
    ops.GpenSRNet(2, nf, scale).load_state_dict(M.base_state_dict(scale, nf, 2), strict=True)
    # a mapping tells its configuration through its keys and conv_first's shape
    from e4s2024_amd import ops_gpen_sr
    assert ops_gpen_sr._validated("t", {"params_ema": dict(sd)}, ops_gpen_sr._GSR_NET)[1] == (2, nf, scale)


def test_mirror_defaults_and_refusals():
    from e4s2024_amd import ops, ops_gpen_sr
    net = ops.GpenSRNet()
    assert (net.num_block, net.num_feat, net.scale) == (23, 32, 2) and len(net.state_dict()) == 702
    assert tuple(net.conv_first.weight.shape) == (32, 12, 3, 3)
    assert ops_gpen_sr._validated("t", {"params": net.state_dict()}, ops_gpen_sr._GSR_NET)[1] == (23, 32, 2)
    for bad in (dict(num_block=0), dict(num_feat=48), dict(scale=3)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            ops.GpenSRNet(**bad)
    assert ops.gpen_sr_output_size(7, 9, 2) == ((15, 19), (1, 1)) and ops.gpen_sr_output_size(12, 20, 2) == ((24, 40), (0, 0))
    assert ops.gpen_sr_output_size(5, 6, 1) == ((5, 6), (3, 2)) and ops.gpen_sr_output_size(5, 6, 4) == ((20, 24), (0, 0))
    for s in (1, 2, 4):
        for H, W in M.GOLDEN_SIZES:
            assert ops.gpen_sr_output_size(H, W, s) == (M.output_size(H, W, s), M.pads(H, W, s))


def test_seeded_weights_depend_on_the_seed_alone():
    from e4s2024_amd import seeded
    assert "seeded_gpen_sr_state_dict" in seeded.__all__
    a, b = seeded.seeded_gpen_sr_state_dict(5, 1, 32, 2), seeded.seeded_gpen_sr_state_dict(5, 1, 32, 2)
    assert all(torch.equal(a[k], b[k]) for k in a) and len(a) == 2 * (15 + 6)
    assert not torch.equal(a["conv_hr.weight"], seeded.seeded_gpen_sr_state_dict(6, 1, 32, 2)["conv_hr.weight"])
    w = a["body.0.rdb2.conv3.weight"].double()                                                # row f11's distribution: normal, gain / sqrt(fan_in)
    assert abs(float(w.std()) * np.sqrt(96 * 9) - seeded.RRDB_GAIN) < 0.02 and float(a["conv_hr.bias"].abs().max()) <= 0.1


@pytest.mark.parametrize("tag", list(M.IMAGE_CASES))
def test_mirror_on_the_cpu_against_the_model(tag):
    from e4s2024_amd import ops
    c = M.image_case(tag)
    scale, nf, nb, H, W = M.IMAGE_CASES[tag]
    net = ops.GpenSRNet(nb, nf, scale).eval()
    net.load_state_dict(c["sd"], strict=True)
    with torch.no_grad():
        got = net(M.sr_input(c["img"], scale, True, torch.float32)).numpy()
    assert got.shape == c["r"].shape
    assert M.max_err(got, c["r"]) <= M.bound(c["e32"], c["r"])


# ------------------------------------------------------------------------------------------------ the model against the reference's own code
@pytest.mark.parametrize("tag", list(M.IMAGE_CASES))
def test_model_against_the_reference(tag, golden):
    """The reference's ``RRDBNet`` (float32, on the CPU) within the bound of the float64 model; its ``RealESRNet.process`` by the uint8 rule; the case is
    conditioned: >= 99 % strict, < 10 % clamped, a standard deviation over 30 grey levels, all three from the model alone."""
    c = M.image_case(tag)
    scale, nf, nb, H, W = M.IMAGE_CASES[tag]
    assert np.array_equal(golden[f"{tag}.img"], c["img"][0])
    r, out = golden[f"{tag}.r"], golden[f"{tag}.out"]
    ph, pw = M.pads(H, W, scale)
    assert r.shape == (3, scale * (H + ph), scale * (W + pw)) and out.shape == M.output_size(H, W, scale) + (3,) and out.dtype == np.uint8
    err = M.max_err(r[None], c["r"])
    print(f"{tag}: the reference's float32 network against the model {err:.3e} = {err / c['e32']:.2f} e32")
    assert err <= M.bound(c["e32"], c["r"])
    strict, clamped, std = M.check_u8(out[None], c["u"], c["e32"])
    assert strict >= 0.99 and clamped < 0.10 and std > 30
    strict, clamped, std = M.check_u8(c["out"], c["u"], c["e32"])                             # the model's own image: the conditioning without the golden
    assert strict >= 0.99 and clamped < 0.10 and std > 30
    assert c["e32"] <= 1e-4 * c["r"].std()


@pytest.mark.parametrize("tag", ["fe.full", "fe.odd"])
def test_face_enhancement_control_flow_against_the_reference(tag, golden):
    """``FaceEnhancement.process(img)`` with ``use_sr``: the reference resized the frame to the SR size (the model's resize), detected and cropped on the resized
    frame and pasted over ``img_sr``: row f15's model on (resized frame, img_sr) gives its result exactly, and its ``img_sr`` is the RealESRNet model's."""
    rec = M.fe_record(golden, tag)
    H, W, _ = M.FE_CASES[tag]
    Ho, Wo = M.output_size(H, W, M.FE_NET[0])
    assert rec["input"].shape == (H, W, 3) and np.array_equal(rec["input"], M.fe_frame(tag))
    assert rec["out"].shape == rec["base"].shape == rec["frame"].shape == (Ho, Wo, 3)
    assert np.array_equal(M.resize_linear(rec["input"], (Wo, Ho)), rec["frame"])
    out, orig = PM.model_outputs(rec)[:2]
    assert np.array_equal(out, rec["out"]) and np.array_equal(orig, rec["orig"]) and not np.array_equal(out, rec["base"])
    c = M.fe_solved(tag, rec["input"])
    strict, clamped, std = M.check_u8(rec["base"][None], c["u"], c["e32"])
    assert strict >= 0.99 and clamped < 0.10 and std > 30
    # pasted over the frame itself, or cropped from the frame before the resize, the result is another one
    other = dict(rec)
    del other["base"]
    assert not np.array_equal(PM.model_outputs(other)[0], rec["out"])


def test_aligned_branch_against_the_reference(golden):
    """``process(img, aligned=True)``: the generator's face through RealESRNet, nothing else."""
    ef, out = golden["fe.aligned.ef"], golden["fe.aligned.out"]
    assert np.array_equal(ef, golden["fe.ef"][0]) and out.shape == (64, 64, 3)
    c = M.fe_solved("fe.aligned", ef)
    strict, clamped, std = M.check_u8(out[None], c["u"], c["e32"])
    assert strict >= 0.99 and clamped < 0.10 and std > 30


@pytest.mark.parametrize("C,H,W", M.TAIL_CASES)
def test_tail_cases_are_conditioned(C, H, W):
    """The cases of the tail kernel alone (tests/test_gpu_gpen_sr.py), under the model: every crop leaves >= 99 % strict, < 10 % clamped, std over 30."""
    m = M.tail_case(C, H, W)
    assert m["f32"].shape == m["r"].shape == (2, 3, H, W) and m["e32"] > 0
    for crop in M.TAIL_CROPS:
        for bgr in (False, True):
            u, img = M.to_u8(m["r"], crop, bgr=bgr)
            assert img.shape == (2, H - crop[0], W - crop[1], 3)
            strict, clamped, std = M.check_u8(M.to_u8(m["f32"], crop, bgr=bgr)[1], u, m["e32"])
            assert strict >= 0.99 and clamped < 0.10 and std > 30, (crop, strict, clamped, std)


# ------------------------------------------------------------------------------------------------ the resize by hand
def _ramp(values, rows=2):
    return np.tile(np.array(values, np.uint8)[None, :, None], (rows, 1, 3))


def test_resize_on_cases_checked_by_hand():
    # x2 of a ramp: f = -0.25 (clamped), 0.25, 0.75, 0.25, 0.75 ..., the last clamped: quarters of the step of 64
    got = M.resize_linear(_ramp([0, 64, 128, 192]), (8, 2))
    assert got.shape == (2, 8, 3) and got[0, :, 0].tolist() == [0, 16, 48, 80, 112, 144, 176, 192] and np.array_equal(got[0], got[1])
    # x4 of a two-pixel ramp: f = -0.375, -0.125 (clamped), 0.125, 0.375, 0.625, 0.875, then the clamp at the last source pixel
    assert M.resize_linear(_ramp([0, 128]), (8, 2))[1, :, 2].tolist() == [0, 0, 16, 48, 80, 112, 128, 128]
    # the same along the other axis
    assert M.resize_linear(_ramp([0, 64, 128, 192]).transpose(1, 0, 2), (2, 8))[:, 1, 1].tolist() == [0, 16, 48, 80, 112, 144, 176, 192]
    # a constant image stays constant, up and down, at any ratio
    for v in (0, 1, 77, 254, 255):
        for dsize in ((11, 15), (3, 2), (7, 5)):
            assert (M.resize_linear(np.full((5, 7, 3), v, np.uint8), dsize) == v).all()
    # a source one pixel wide: every column is that pixel's column; at equal height the rows are picked, not blended
    col = np.arange(0, 15, dtype=np.uint8).reshape(5, 1, 3) * 17
    got = M.resize_linear(col, (4, 5))
    assert got.shape == (5, 4, 3) and all(np.array_equal(got[:, x], col[:, 0]) for x in range(4))
    # the identity, and the refusal of what cv2 hands to INTER_AREA
    img = M.images_u8(3, 1, 6, 8)[0]
    assert np.array_equal(M.resize_linear(img, (8, 6)), img)
    with pytest.raises(ValueError, match="INTER_AREA"):
        M.resize_linear(img, (4, 3))
    assert M.resize_linear(img, (4, 4)).shape == (4, 4, 3)                                    # 2 : 1 on one axis alone is INTER_LINEAR
    assert M.resize_linear(np.stack([img, img]), (5, 9)).shape == (2, 9, 5, 3)


def test_fma32_is_one_rounding():
    """``gpen_sr_model.fma32`` against exact rational arithmetic on values chosen to sit on double-rounding edges."""
    from fractions import Fraction
    rs = np.random.RandomState(4)
    a = rs.randn(4000).astype(np.float32)
    b = rs.randn(4000).astype(np.float32)
    c = (rs.randn(4000) * np.float32(2.0) ** rs.randint(-30, 4, 4000)).astype(np.float32)
    got = M.fma32(a.astype(np.float64), b.astype(np.float64), c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(exact - Fraction(float(g))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))


# ------------------------------------------------------------------------------------------------ mutants
def test_every_mutant_is_told_apart():
    """Each single-change mutant of the model lies at least ten bounds from it on some case (a uint8 end: one grey level is 1 / 255 of the float range; the
    integer resize: at least one grey level on some pixel)."""
    worst_bound = max(M.bound(M.image_case(t)["e32"], M.image_case(t)["r"]) for t in M.IMAGE_CASES)
    assert MUTANT_LEVEL / worst_bound >= M.MUTANT_MARGIN
    far = {m: 0.0 for m in M.MUTANTS}
    for tag in M.IMAGE_CASES:
        c = M.image_case(tag)
        b = M.bound(c["e32"], c["r"])
        for m in M.NET_MUTANTS:
            far[m] = max(far[m], M.max_err(M.process(c["sd"], c["img"], mutant=m)[0].numpy(), c["r"]) / b)
        for m in M.END_MUTANTS:
            out = M.process(c["sd"], c["img"], mutant=m)[2]
            d = np.inf if out.shape != c["out"].shape else np.abs(out.astype(int) - c["out"].astype(int)).max() * MUTANT_LEVEL
            far[m] = max(far[m], d / b)
    # half-up and half-to-even part on exact ties only, which a seeded float64 image never has: values whose float32 product with 255 is k + 0.5
    ties = M.tie_values()
    assert len(ties) >= 200
    r = np.zeros(3 * ((len(ties) + 2) // 3), np.float32)
    r[:len(ties)] = ties
    r = r.reshape(1, 3, 1, -1)
    even, up = M.to_u8(r, (0, 0))[1], M.to_u8(r, (0, 0), mutant="half_up")[1]
    assert (np.abs(up.astype(int) - even.astype(int)) <= 1).all() and (up != even).sum() >= 100 and (even % 2 == 0).sum() >= len(ties) - 2
    far["half_up"] = max(far["half_up"], MUTANT_LEVEL / worst_bound)
    for (H, W), dsize in (((5, 7), (15, 11)), ((8, 8), (32, 32)), ((40, 36), (23, 17))):
        img = M.images_u8(H * 100 + W, 1, H, W)[0]
        want = M.resize_linear(img, dsize).astype(int)
        for m in M.RESIZE_MUTANTS:
            d = np.abs(M.resize_linear(img, dsize, mutant=m).astype(int) - want).max()
            far[m] = max(far[m], M.MUTANT_MARGIN if d >= 1 else 0.0)
    print({m: (f"{v:.1f}" if np.isfinite(v) else "shape") for m, v in far.items()})
    assert all(v >= M.MUTANT_MARGIN for v in far.values()), far


# ------------------------------------------------------------------------------------------------ names, overrides, entry points, drop-ins
def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_gpen_sr, pipeline
    assert set(NAMES) == set(ops_gpen_sr.__all__)
    for name in NAMES:
        assert getattr(ops, name) is getattr(ops_gpen_sr, name)
    assert ops.GPEN_SR_FEATS == (32, 64) and ops.GPEN_SR_SCALES == (1, 2, 4)
    assert e4s2024_amd.GPEN_SR_OVERRIDES == {
        "swap_face_fine.gpen.sr_model.rrdbnet_arch": "swap_face_fine/gpen/sr_model/rrdbnet_arch.py",
        "swap_face_fine.gpen.sr_model.real_esrnet": "swap_face_fine/gpen/sr_model/real_esrnet.py",
        "swap_face_fine.gpen.face_enhancement": "swap_face_fine/gpen/face_enhancement.py"}
    assert set(e4s2024_amd.GPEN_SR_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert all(os.path.isfile(os.path.join(e4s2024_amd.DROPIN_DIR, rel)) for rel in e4s2024_amd.GPEN_SR_OVERRIDES.values())
    assert "GPEN_SR_OVERRIDES" in e4s2024_amd.install.__doc__
    assert not any(m.endswith("sr_model.arch_util") for m in e4s2024_amd._redirected())
    for name in ("gpen_super_resolve", "gpen_face_enhancement"):
        assert callable(getattr(pipeline, name))


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert [len(_lib._PROTOS[n]) for n in sorted(ENTRY_POINTS)] == [8, 8, 13]
    assert _lib.ABI_VERSION == 1


def test_dropins_import_without_cv2_basicsr_skimage(tmp_path):
    import importlib.util
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    for lib in ("cv2", "basicsr", "skimage"):
        assert importlib.util.find_spec(lib) is None and lib not in sys.modules
    from swap_face_fine.gpen import face_enhancement
    from swap_face_fine.gpen.sr_model import real_esrnet, rrdbnet_arch
    for mod in (face_enhancement, real_esrnet, rrdbnet_arch):
        assert mod.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    for lib in ("cv2", "basicsr", "skimage"):
        assert lib not in sys.modules
    from e4s2024_amd import ops
    net = rrdbnet_arch.RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=32, num_block=1, num_grow_ch=32, scale=2)
    assert isinstance(net, ops.GpenSRNet) and (net.num_block, net.num_feat, net.scale) == (1, 32, 2)
    assert tuple(rrdbnet_arch.RRDBNet(3, 3).conv_first.weight.shape) == (64, 3, 3, 3)         # the reference's defaults: scale 4, num_feat 64
    with pytest.raises(ValueError, match="num_in_ch"):
        rrdbnet_arch.RRDBNet(1, 3)
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(torch.zeros(1, 3, 2, 2))
    # the checkpoint: <base_dir>/weights/realesrnet_x2.pth without a model name (whatever the scale), <model>_x<scale>.pth with one
    base = str(tmp_path)
    assert real_esrnet.checkpoint_path(base, None, 4) == os.path.join(base, "weights", "realesrnet_x2.pth")
    assert real_esrnet.checkpoint_path(base, "realesrnet", 4) == os.path.join(base, "weights", "realesrnet_x4.pth")
    with pytest.raises(FileNotFoundError, match="realesrnet_x4.pth"):
        real_esrnet.RealESRNet(base, "realesrnet", 4, device="cpu")
    os.makedirs(os.path.join(base, "weights"))
    torch.save({"params_ema": M.base_state_dict(4, 32, 23)}, os.path.join(base, "weights", "realesrnet_x4.pth"))
    sr = real_esrnet.RealESRNet(base, "realesrnet", 4, device="cpu")                          # strict=True load of params_ema
    assert sr.scale == 4 and not sr.srmodel.training and torch.equal(sr.srmodel.conv_hr.bias, M.base_state_dict(4, 32, 23)["conv_hr.bias"])
    torch.save({"params_ema": M.base_state_dict(2, 32, 23)}, os.path.join(base, "weights", "realesrnet_x2.pth"))
    with pytest.raises(RuntimeError, match="conv_first.weight"):                              # an x2 checkpoint does not load into the x4 network
        real_esrnet.RealESRNet(base, None, 4, device="cpu")
    with pytest.raises(NotImplementedError, match="out_size"):
        face_enhancement.FaceEnhancement(base, in_size=512, out_size=1024)
    with pytest.raises(FileNotFoundError, match="RetinaFace-R50.pth"):                        # the constructor's order: the detector first, as the reference
        face_enhancement.FaceEnhancement(base, model="GPEN-BFR-512")
    with pytest.raises(TypeError, match="uint8"):
        real_esrnet.RealESRNet.process(sr, np.zeros((4, 4, 3), np.float32))


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops
    sd = M.base_state_dict(2, 32, 1)
    net = ops.GpenSRNet(1, 32, 2).eval()
    net.load_state_dict(sd)
    good = torch.zeros(1, 3, 8, 8)
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for weights in (net, sd, {"params_ema": sd}, {"params." + k: v for k, v in sd.items()}):
        with pytest.raises(RuntimeError, match="x must be a CUDA tensor"):
            ops.gpen_sr_forward(good, weights)
        with pytest.raises(RuntimeError, match="img_u8 must be a CUDA tensor"):
            ops.gpen_sr_image(img, weights)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.gpen_sr_forward(good.transpose(2, 3), net)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.gpen_sr_forward(good.numpy(), net)
    with pytest.raises(TypeError, match="module or a mapping"):
        ops.gpen_sr_forward(good, None)
    with pytest.raises(KeyError, match="conv_first.weight"):
        ops.gpen_sr_forward(good, {"conv.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="body.0.rdb1.conv1.weight"):
        ops.gpen_sr_forward(good, {"conv_first.weight": sd["conv_first.weight"]})
    with pytest.raises(KeyError, match="conv_hr.bias"):
        ops.gpen_sr_forward(good, {k: v for k, v in sd.items() if k != "conv_hr.bias"})
    with pytest.raises(ValueError, match=r"body.0.rdb2.conv5.weight.*\(32, 160, 3, 3\)"):
        ops.gpen_sr_forward(good, {**sd, "body.0.rdb2.conv5.weight": torch.zeros(32, 160, 1, 1)})
    with pytest.raises(ValueError, match="conv_first.weight"):                                # 5 input channels are no scale
        ops.gpen_sr_forward(good, {**sd, "conv_first.weight": torch.zeros(32, 5, 3, 3)})
    with pytest.raises(ValueError, match="conv_first.weight"):                                # 48 features are no width of this network
        ops.gpen_sr_forward(good, {**sd, "conv_first.weight": torch.zeros(48, 12, 3, 3)})
    with pytest.raises(ValueError, match="conv_up1.bias.*float64"):
        ops.gpen_sr_forward(good, {**sd, "conv_up1.bias": sd["conv_up1.bias"].double()})
    with pytest.raises(ValueError, match="float32"):
        ops.gpen_sr_forward(good.double(), net)
    with pytest.raises(ValueError, match="float32"):
        ops.gpen_sr_forward(good[0], net)                                                     # rank
    with pytest.raises(ValueError, match=r"\[bs, 3, h, w\]"):
        ops.gpen_sr_forward(torch.zeros(1, 4, 8, 8), net)
    with pytest.raises(ValueError, match="divisible"):
        ops.gpen_sr_forward(torch.zeros(1, 3, 7, 8), net)
    with pytest.raises(ValueError, match="divisible"):
        ops.gpen_sr_forward(torch.zeros(1, 3, 8, 6), M.base_state_dict(1, 64, 1))             # scale 1 unshuffles by 4
    with pytest.raises(ValueError, match="16384"):
        ops.gpen_sr_forward(torch.zeros(1, 3, 2, 8194), net)
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.gpen_sr_forward(good, ops.GpenSRNet(1).to("meta"))
    # the image entry
    with pytest.raises(ValueError, match="uint8"):
        ops.gpen_sr_image(img.float(), net)
    with pytest.raises(ValueError, match=r"\[bs, H, W, 3\]"):
        ops.gpen_sr_image(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), net)
    with pytest.raises(ValueError, match="reflect pad"):
        ops.gpen_sr_image(torch.zeros(1, 1, 8, 3, dtype=torch.uint8), net)                    # one row, one row of pad
    with pytest.raises(ValueError, match="reflect pad"):
        ops.gpen_sr_image(torch.zeros(1, 8, 2, 3, dtype=torch.uint8), M.base_state_dict(1, 64, 1))        # two columns, two of pad
    with pytest.raises(ValueError, match="16384"):
        ops.gpen_sr_image(torch.zeros(1, 2, 8193, 3, dtype=torch.uint8), net)
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.gpen_sr_image(img, ops.GpenSRNet(1).to("meta"))
    # the resize
    with pytest.raises(RuntimeError, match="img_u8 must be a CUDA tensor"):
        ops.cv_resize_linear(img, (16, 16))
    with pytest.raises(ValueError, match="uint8"):
        ops.cv_resize_linear(img.float(), (16, 16))
    with pytest.raises(ValueError, match="INTER_AREA"):
        ops.cv_resize_linear(img, (4, 4))
    for bad in ((0, 4), (4, 16385), (4.0, 4), (True, 4), 7, (1, 2, 3)):
        with pytest.raises(ValueError, match="dsize"):
            ops.cv_resize_linear(img, bad)


def test_face_enhancement_argument_rules():
    from e4s2024_amd import ops, pipeline
    sr = ops.GpenSRNet(1, 32, 2).eval()
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for aligned in (False, True):
        with pytest.raises(ValueError, match="frames_u8"):
            pipeline.gpen_face_enhancement(None, None, None, sr, frames.float(), aligned=aligned)
        with pytest.raises(ValueError, match="bs >= 1"):
            pipeline.gpen_face_enhancement(None, None, None, sr, frames[:0], aligned=aligned)
        with pytest.raises(KeyError, match="conv_first.weight"):
            pipeline.gpen_face_enhancement(None, None, None, {"a": torch.zeros(1)}, frames, aligned=aligned)
        with pytest.raises(RuntimeError, match="device mismatch"):
            pipeline.gpen_face_enhancement(None, None, None, ops.GpenSRNet(1).to("meta"), frames, aligned=aligned)
        with pytest.raises(RuntimeError, match="frames_u8 must be a CUDA tensor"):
            pipeline.gpen_face_enhancement(None, None, None, sr, frames, aligned=aligned)
        with pytest.raises(RuntimeError, match="frames_u8 must be a CUDA tensor"):
            pipeline.gpen_face_enhancement(None, None, None, None, frames, aligned=aligned)
    with pytest.raises(RuntimeError, match="img_u8 must be a CUDA tensor"):
        pipeline.gpen_super_resolve(sr, frames)
