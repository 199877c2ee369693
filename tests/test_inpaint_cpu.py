"""Row f25 (the GCFSR inpainting generator) without a GPU: the reference's stored outputs against the float64 restatement ``inpaint_model``, the mirror module's
keys against the reference's, the mirror on stock PyTorch, the bars of the GPU tests pinned from the other side by single-change mutants, the models of the
kernels' arithmetic, the mask-support rule against a brute-force resize, the drop-in and the argument errors that must raise before any launch.

The bound of a case is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64.  Every mutant of the model lies at least ten
times the default route's bar (1e-3 on the raw output) from the reference's output on some case, so a kernel inside either bar has none of these mistakes."""
import os
import zlib

import numpy as np
import pytest
import torch

import inpaint_model as M
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_gcfsr_input", "e4s_gcfsr_condition", "e4s_gcfsr_scale_shift_act", "e4s_gcfsr_tail", "e4s_cv_mask_support"}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g35_inpaint")


@pytest.mark.parametrize("tag", list(M.CASES))
def test_reference_outputs_lie_within_the_bound_of_the_model(tag, golden):
    c = M.case(tag)
    size, bs = M.CASES[tag]
    assert int(golden[f"{tag}.crc"]) == zlib.crc32(c["x"].tobytes())                           # the same seeded input as when the fixture was made
    ref, stride = golden[f"{tag}.out"], int(golden[f"{tag}.stride"])
    assert ref.dtype == np.float32 and stride == M.sample_stride(c["want"].size) and ref.shape == M.stored(c["want"]).shape
    assert (stride == 1) == (c["want"].size <= 16384)
    err, ref_err = M.max_err(ref, M.sampled(c["want"])), float(golden[f"{tag}.ref_err"])
    print(f"{tag}: the reference against the model {ref_err:.3e} = {ref_err / c['e32']:.2f} e32 (stored part {err:.3e}), e32 {c['e32']:.3e}")
    bar = M.bound(c["e32"], c["want"])
    assert err <= ref_err <= bar
    if stride > 1:
        assert M.max_err(golden[f"{tag}.cmean"], c["want"].reshape(bs, 3, -1).mean(2)) <= bar
    assert c["e32"] <= 1e-4 * c["want"].std()                                                 # the case is well conditioned
    # the clamp must not hide the network: at least half of the raw values inside the hole lie strictly inside (0, 1), on the reference and on the model
    assert float(golden[f"{tag}.share"]) >= 0.5 and M.hole_inside_share(c["want"], c["hole"]) >= 0.5
    assert abs(float(golden[f"{tag}.share"]) - M.hole_inside_share(c["want"], c["hole"])) < 1e-3


def test_cases_have_distinct_hole_shares_and_one_empty_hole():
    c = M.case("i32")
    assert c["in_size"][1] == 0 and 0.1 < c["in_size"][0] < 0.5 and c["hole"][1].max() == 0
    assert [len(M.noise_sizes(s)) for s in (32, 64, 256)] == [3, 5, 9] and M.noise_sizes(256) == [16, 32, 32, 64, 64, 128, 128, 256, 256]
    assert c["latent"].shape == (2, 4, 512) and M.case("i64")["latent"].shape == (1, 6, 512)
    assert c["x"].shape == (2, 4, 32, 32) and np.array_equal(c["x"][:, 3], c["hole"].astype(np.float32)) and (c["x"][0, :3][:, c["hole"][0] != 0] == 0).all()


def test_every_mutant_is_ten_pixel_bars_from_the_fixture_on_some_case(golden):
    assert len(M.MUTANTS) == 11
    for m in M.MUTANTS:
        far = 0.0
        for tag in M.CASES:                                                                   # smallest case first; a mutant far enough there is done
            c = M.case(tag)
            far = max(far, M.max_err(M.stored(M.network(c["sd"], c["x"], c["in_size"], c["noise"], mutant=m).numpy()), golden[f"{tag}.out"]))
            if far >= M.MUTANT_MARGIN * M.PIXEL_TOL:
                break
        print(f"mutant {m}: {far:.3e} from the fixture")
        assert far >= M.MUTANT_MARGIN * M.PIXEL_TOL, m
    # and the unmutated model is not: the bar separates them
    assert all(M.max_err(M.stored(M.case(tag)["want"]), golden[f"{tag}.out"]) < 1e-2 * M.PIXEL_TOL for tag in ("i32", "i64"))


def test_mirror_has_the_reference_keys_in_order(golden):
    from e4s2024_amd import ops
    want = [(line.split("|")[0], tuple(int(d) for d in line.split("|")[1].split("x"))) for line in str(golden["keys.default"]).split("\n")]
    with torch.device("meta"):
        sd = ops.FaceInpainting().state_dict()
    assert len(want) == 122 and [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert list(ops.inpaint_state_dict_shapes().items()) == want
    # the stored noise keeps the reference's (wrong) shapes: 4, 8, 8, 16, ... for layers that run at 16, 32, 32, 64, ...
    assert [dict(want)[f"noises.noise{i}"][-1] for i in range(9)] == [4, 8, 8, 16, 16, 32, 32, 64, 64]
    assert not any("kernel" in k for k, _ in want)                                            # the FIR kernels are plain attributes there, not keys
    small = ops.inpaint_state_dict_shapes(32)
    assert len(small) == 50 and sum(int(np.prod(s)) for s in small.values()) == 29788569
    for bad in (48, 16, 2048, 256.0, True):
        with pytest.raises(ValueError, match="power of two"):
            ops.FaceInpainting(bad)


def test_seeded_weights_depend_on_the_seed_alone():
    from e4s2024_amd import seeded
    assert "seeded_inpaint_state_dict" in seeded.__all__
    a, b = M.state_dict(32), seeded.seeded_inpaint_state_dict(M.WEIGHT_SEED, 32)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["final_conv.0.weight"], seeded.seeded_inpaint_state_dict(M.WEIGHT_SEED + 1, 32)["final_conv.0.weight"])
    for k, v in a.items():                                  # what the reference initialises to zero or one must be well away from both here
        if k.startswith(("condition_scale", "condition_shift")) and k.endswith("bias") or k.endswith("conv1.weight") or k.startswith("style_convs") and k.count(".") == 2:
            assert float(v.abs().min()) >= 0.15 and float((v - 1).abs().min()) >= 0.15, k
        if k.startswith("condition_scale") and k.endswith("weight"):
            assert float(v.abs().min()) >= 0.3, k
        if k.endswith("bias"):
            assert float(v.abs().max()) > 0, k
    # no other family's bytes moved: the rule tables are looked up by name
    assert torch.equal(seeded.seeded_gpen_state_dict(5, 16, 32, 2, 2, 1 / 32)["ecd1.0.1.weight"], seeded.seeded_state_dict(
        {"ecd1.0.1.weight": torch.empty(16, 16, 3, 3, device="meta")}, 5, "gpen")["ecd1.0.1.weight"])


@pytest.mark.parametrize("tag", ["i32", "i64"])
def test_mirror_on_the_cpu_against_the_model(tag):
    from e4s2024_amd import ops
    c = M.case(tag)
    net = ops.FaceInpainting(M.CASES[tag][0]).eval()
    net.load_state_dict(c["sd"], strict=True)
    noise = [T(n) for n in c["noise"]]
    out, latent = net(T(c["x"]), T(c["in_size"]), noise, return_latents=True)
    assert net(T(c["x"]), T(c["in_size"]).view(-1, 1), noise)[1] is None
    assert M.max_err(out.numpy(), c["want"]) <= M.bound(c["e32"], c["want"])
    assert M.max_err(latent.numpy(), c["latent"]) <= M.bound(c["e32_latent"], c["latent"])
    assert net(T(c["x"]), T(c["in_size"]))[0].shape == out.shape                              # noise=None: fresh draws
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(c["x"]), T(c["in_size"]), noise)


def test_kernel_models_restate_the_float32_composition():
    """The numpy models the GPU tests compare the kernels with, against stock PyTorch in float32 on the CPU: the same bits where PyTorch rounds every operation
    (the epilogue, the ends), Norm2Scale up to rsqrt's last bits."""
    rs = np.random.RandomState(3)
    y, shift = rs.standard_normal((2, 5, 7, 9)).astype(np.float32), rs.standard_normal((2, 5, 7, 9)).astype(np.float32)
    s1n, s2n, bias = (rs.uniform(-1, 1, s).astype(np.float32) for s in ((2, 5), (2, 5), (5,)))
    want = torch.nn.functional.leaky_relu(T(y) * T(s1n).view(2, 5, 1, 1) + T(shift) * T(s2n).view(2, 5, 1, 1) + T(bias).view(1, 5, 1, 1), 0.2) * 2 ** 0.5
    assert np.array_equal(M.scale_shift_act_model(y, shift, s1n, s2n, bias), want.numpy())
    levels = [tuple(rs.uniform(-1, 1, s).astype(np.float32) for s in ((c, 1), (c,), (c, 1), (c,))) for c in (6, 3)]
    in_size = np.float32([0, 1, 0.37])
    a, b = M.condition_model(in_size, levels)
    assert a.shape == b.shape == (3, 9) and a.dtype == np.float32
    for l, col in ((0, 0), (1, 6)):
        w1, b1, w2, b2 = (T(t).double() for t in levels[l])
        s1, s2 = T(in_size).double().view(-1, 1) @ w1.t() + b1, T(in_size).double().view(-1, 1) @ w2.t() + b2
        r = torch.rsqrt(s1 ** 2 + s2 ** 2 + 1e-8)
        C = w1.shape[0]
        assert M.max_err(a[:, col:col + C], (s1 * r).numpy()) <= 4e-7 and M.max_err(b[:, col:col + C], (s2 * r).numpy()) <= 4e-7
    assert np.abs(a * a + b * b - 1).max() <= 1e-6
    # the ends: every byte survives the round trip outside the hole, the hole takes the clamped network value
    faces = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    hole = np.zeros((1, 16, 16), np.uint8)
    x, in_size, count = M.input_model(faces, hole)
    assert x.shape == (1, 4, 16, 16) and count[0] == 0 and in_size[0] == 0
    assert torch.equal(T(x[:, :3]), (torch.from_numpy(faces / 255.).permute(0, 3, 1, 2)).float())
    img = rs.uniform(-0.5, 1.5, (1, 3, 16, 16)).astype(np.float32)
    assert np.array_equal(M.tail_model(img, faces, hole), faces)
    hole[:, 4:9, 3:11] = 1
    x, in_size, count = M.input_model(faces, hole)
    assert count[0] == 40 and in_size[0] == np.float32(40) / np.float32(256) and (x[0, :3, 4:9, 3:11] == 0).all() and x[0, 3].sum() == 40
    got = M.tail_model(img, faces, hole)
    want = (np.clip(img, 0, 1) * np.float32(255.0)).round().astype(np.uint8).transpose(0, 2, 3, 1)
    assert np.array_equal(got[hole != 0], want[hole != 0]) and np.array_equal(got[hole == 0], faces[hole == 0])
    assert {0, 255} <= set(got[hole != 0].ravel().tolist())                                    # the clamp acted on both sides


@pytest.mark.parametrize("H,W,S", M.MASK_PAIRS)
@pytest.mark.parametrize("soft", [False, True])
def test_mask_support_agrees_with_a_brute_force_resize(H, W, S, soft):
    from e4s2024_amd import ops_inpaint
    mask = M.mask_case(H * 1000 + W + soft, H, W, soft)
    got, want = M.mask_support_model(mask, S), M.mask_support_brute(mask, S)
    assert got.dtype == np.uint8 and got.shape == (2, S, S) and np.array_equal(got, want)
    assert 0 < got[0].mean() < 1
    # the host tables the device kernel takes are the model's
    area = H == 2 * S and W == 2 * S
    for src in (H, W):
        s, c = ops_inpaint.mask_support_axis(src, S, area)
        ms, mc = M._support_axis(src, S, area)
        assert s.dtype == c.dtype == np.int32 and np.array_equal(s, ms) and np.array_equal(c, mc)
        assert s.min() >= 0 and (s + c - 1).max() <= src - 1 and set(c.tolist()) <= {1, 2}
    if (H, W) == (S, S):
        assert np.array_equal(got, (mask > 0).astype(np.uint8))


def test_the_uint8_rule_accepts_and_refuses():
    c = M.case("i32")
    u = M.composite(c["want"], c["faces"], c["hole"]) * 255.0
    want = np.rint(u).astype(np.uint8)
    share = M.check_u8(want, c["want"], c["faces"], c["hole"], c["e32"])
    print(f"i32: {share:.4f} of the values are strict, margin {M.MARGIN * c['e32'] * 255:.2e} levels")
    assert share >= 0.99
    hole = np.broadcast_to((c["hole"] != 0)[..., None], want.shape)
    bad = want.copy()
    i = tuple(np.argwhere(hole & (want < 255) & (np.abs(u - np.floor(u) - 0.5) > 0.1))[0])
    bad[i] += 1
    with pytest.raises(AssertionError, match="strict"):
        M.check_u8(bad, c["want"], c["faces"], c["hole"], c["e32"])
    bad = want.copy()
    bad[tuple(np.argwhere(~hole & (want < 255))[0])] += 1
    with pytest.raises(AssertionError, match="outside the hole"):
        M.check_u8(bad, c["want"], c["faces"], c["hole"], c["e32"])


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_inpaint, pipeline
    for name in ("FaceInpainting", "PreparedInpaint", "inpaint_forward", "inpaint_input", "inpaint_condition", "scale_shift_act", "inpaint_tail", "cv_mask_support",
                 "inpaint_state_dict_shapes", "inpaint_image"):
        assert name in ops_inpaint.__all__ and getattr(ops, name) is getattr(ops_inpaint, name)
    assert ops_inpaint.ARITH == "sb" and ops_inpaint.UP_COMPOSED_MAX_WIDTH == 32 and callable(pipeline.inpaint_faces)
    assert e4s2024_amd.INPAINT_OVERRIDES == {"swap_face_fine.face_inpainting": "swap_face_fine/face_inpainting.py"}
    assert set(e4s2024_amd.INPAINT_OVERRIDES) <= set(e4s2024_amd._all_redirected()) and set(e4s2024_amd._redirected()) <= set(e4s2024_amd._all_redirected())
    assert "INPAINT_OVERRIDES" in e4s2024_amd.install.__doc__
    assert os.path.isfile(os.path.join(e4s2024_amd.DROPIN_DIR, "swap_face_fine", "face_inpainting.py"))
    assert "swap_face_fine.gcfsr_arch" not in e4s2024_amd._all_redirected()


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols())
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert [len(_lib._PROTOS[n]) for n in sorted(ENTRY_POINTS)] == [12, 11, 9, 10, 7]


def test_dropin_resolves_and_imports_without_cv2_or_basicsr():
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    from swap_face_fine import face_inpainting
    assert face_inpainting.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    assert "cv2" not in sys.modules and "basicsr" not in sys.modules and "swap_face_fine.gcfsr_arch" not in sys.modules
    assert face_inpainting.model_path == './pretrained/inpainting/net_g_50000.pth' and face_inpainting._model is None      # nothing loaded at import
    import inspect
    assert list(inspect.signature(face_inpainting.inpainting).parameters) == ["face_img", "mask"]


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops, ops_inpaint, pipeline
    c = M.case("i32")
    net = ops.FaceInpainting(32).eval()
    x, in_size, noise = T(c["x"]), T(c["in_size"]), [T(n) for n in c["noise"]]
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.inpaint_forward(x, in_size, net)
    net.load_state_dict(c["sd"], strict=True)
    with pytest.raises(RuntimeError, match="CUDA"):                                           # a CPU tensor
        ops.inpaint_forward(x, in_size, net, noise)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.inpaint_image(T(c["faces"]), T(c["hole"]), net)
    with pytest.raises(RuntimeError, match="CUDA"):
        pipeline.inpaint_faces(net, T(c["faces"]), T(c["hole"]))
    with pytest.raises(ValueError, match="float32"):
        ops.inpaint_forward(x.double(), in_size, net)
    with pytest.raises(ValueError, match="size is 32"):
        ops.inpaint_forward(x[:, :, :, :16], in_size, net)
    with pytest.raises(ValueError, match="size is 32"):
        ops.inpaint_forward(x[:, :3], in_size, net)
    with pytest.raises(ValueError, match="in_size"):
        ops.inpaint_forward(x, in_size[:1], net)
    with pytest.raises(ValueError, match="in_size"):
        ops.inpaint_forward(x, in_size.double(), net)
    with pytest.raises(ValueError, match="list of 3"):
        ops.inpaint_forward(x, in_size, net, noise[:2])
    with pytest.raises(ValueError, match=r"noise\[1\]"):
        ops.inpaint_forward(x, in_size, net, [noise[0], noise[1][:, :, :16, :16], noise[2]])
    with pytest.raises(ValueError, match=r"noise\[0\]"):
        ops.inpaint_forward(x, in_size, net, [noise[0].double()] + noise[1:])
    with pytest.raises(ValueError, match="another batch"):
        ops.inpaint_image(T(c["faces"]), T(c["hole"])[:1], net)
    with pytest.raises(ValueError, match="another batch"):
        pipeline.inpaint_faces(net, T(c["faces"]), T(c["hole"])[:1])
    with pytest.raises(ValueError, match="32, 32, 3"):
        ops.inpaint_image(T(c["faces"])[:, :16, :16], T(c["hole"])[:, :16, :16], net)
    with pytest.raises(ValueError, match="uint8"):
        ops.inpaint_image(T(c["faces"]).float(), T(c["hole"]), net)
    with pytest.raises(ValueError, match="float32 or uint8"):
        ops.cv_mask_support(T(c["hole"]).double(), 32)
    with pytest.raises(ValueError, match="size"):
        ops.cv_mask_support(T(c["hole"]), 0)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.inpaint_forward(x, in_size, net.train(), noise)
    net.eval()
    with pytest.raises(KeyError, match="conv_body_first.0.weight"):
        ops.inpaint_forward(x, in_size, {"conv.weight": x})
    sd = dict(c["sd"])
    del sd["style_convs.1.weight"]
    with pytest.raises(KeyError, match="style_convs.1.weight"):
        ops.inpaint_forward(x, in_size, sd)
    narrow = dict(c["sd"])
    narrow["style_conv1.modulated_conv.weight"] = c["sd"]["style_conv1.modulated_conv.weight"][:, :256]
    with pytest.raises(ValueError, match="narrow"):
        ops.inpaint_forward(x, in_size, narrow)
    cm = dict(c["sd"])
    cm["conv_body_first.0.weight"] = c["sd"]["conv_body_first.0.weight"][:256]
    with pytest.raises(ValueError, match="channel_multiplier"):
        ops.inpaint_forward(x, in_size, cm)
    assert [tuple(t.shape) for t in ops.inpaint_weight_tensors(c["sd"])] == [tuple(v.shape) for v in c["sd"].values()]
    assert ops.inpaint_size(c["sd"]) == 32 and ops.inpaint_size(net) == 32
    ops_inpaint.ARITH = "bf16"
    try:
        with pytest.raises((ValueError, RuntimeError), match="ARITH|CUDA"):                   # (a CPU tensor is refused first)
            ops.inpaint_forward(x, in_size, net, noise)
    finally:
        ops_inpaint.ARITH = "sb"
