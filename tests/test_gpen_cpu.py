"""Row f12 (GPEN's generator) without a GPU: the reference's stored outputs against the float64 restatement ``gpen_model``, the mirror module's keys against
the reference's, the mirror on stock PyTorch, the bars of the GPU tests pinned from the other side by single-change mutants, the uint8 ends, the drop-in and
the argument errors that must raise before any launch.

The bound of a case is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64.  Every mutant of the model lies at least ten
times the default route's bar (1e-3 on generated pixels) from the reference's output on some case, so a kernel inside either bar has none of these mistakes."""
import zlib

import numpy as np
import pytest
import torch

import gpen_model as GM
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_gpen_stem", "e4s_gpen_noise_half", "e4s_gpen_to_u8"}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g23_gpen")


@pytest.mark.parametrize("tag", list(GM.CASES))
def test_reference_outputs_lie_within_the_bound_of_the_model(tag, golden):
    c = GM.case(tag)
    size, _, sdim, bs = GM.CASES[tag]
    ref = golden[f"{tag}.out"]
    assert int(golden[f"{tag}.crc"]) == zlib.crc32(c["x"].tobytes())                           # the same seeded input as when the fixture was made
    assert ref.dtype == np.float32 and ref.shape == (bs, 3, size, size) == c["want"].shape
    err = GM.max_err(ref, c["want"])
    print(f"{tag}: the reference against the model {err:.3e} = {err / c['e32']:.2f} e32, e32 {c['e32']:.3e}, output std {ref.std():.3f}")
    assert err <= GM.bound(c["e32"], c["want"])
    assert c["e32"] <= 1e-4 * c["want"].std()                                                 # the case is well conditioned
    assert 0.3 <= ref.std() <= 0.5 and (np.abs(ref) >= 1).mean() <= 0.05                      # an image, not a saturated or flat map
    if tag == GM.LATENT_CASE:
        assert golden[f"{tag}.latent"].shape == (bs, 2 * int(np.log2(size)) - 2, sdim)
        assert GM.max_err(golden[f"{tag}.latent"], c["latent"]) <= GM.bound(c["e32_latent"], c["latent"])


def test_every_mutant_is_ten_pixel_bars_from_the_fixture_on_some_case(golden):
    assert len(GM.MUTANTS) == 11
    for m in GM.MUTANTS:
        far = max(GM.max_err(GM.network(GM.case(tag)["sd"], GM.case(tag)["x"], mutant=m).numpy(), golden[f"{tag}.out"]) for tag in GM.CASES)
        print(f"mutant {m}: {far:.3e} from the fixture")
        assert far >= GM.MUTANT_MARGIN * GM.PIXEL_TOL, m
    # and the unmutated model is not: the bar separates them
    assert all(GM.max_err(GM.case(tag)["want"], golden[f"{tag}.out"]) < 1e-2 * GM.PIXEL_TOL for tag in GM.CASES)


def test_mirror_has_the_reference_keys_in_order(golden):
    from e4s2024_amd import ops
    want = [(line.split("|")[0], tuple(int(d) for d in line.split("|")[1].split("x"))) for line in str(golden["keys.default"]).split("\n")]
    sd = ops.GPEN().state_dict()
    assert len(want) == 163 and [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert list(ops.gpen_state_dict_shapes().items()) == want
    assert sum(int(np.prod(s)) for _, s in want) == 71005559
    assert set(dict(want)) >= {"generator.input.input", "generator.convs.0.conv.blur.kernel", "generator.to_rgbs.0.upsample.kernel", "ecd1.0.0.kernel"}
    with pytest.raises(ValueError, match="power of two"):
        ops.GPEN(48)


def test_seeded_weights_depend_on_the_seed_alone():
    from e4s2024_amd import seeded
    assert "seeded_gpen_state_dict" in seeded.__all__
    a, b = seeded.seeded_gpen_state_dict(5, 16, 32, 2, 2, 1 / 32), seeded.seeded_gpen_state_dict(5, 16, 32, 2, 2, 1 / 32)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["ecd1.0.1.weight"], seeded.seeded_gpen_state_dict(6, 16, 32, 2, 2, 1 / 32)["ecd1.0.1.weight"])
    for k, v in a.items():                                                                    # what the reference initialises to zero must not be zero here
        if k.endswith(("noise.weight", "activate.bias")) or (".to_rgb" in k and k.endswith(".bias")):
            assert float(v.abs().min()) > 0, k
        if k.endswith("noise.weight"):
            assert float(v.abs()) >= 0.3
    assert torch.equal(a["ecd1.0.0.kernel"] * 4, a["generator.convs.0.conv.blur.kernel"]) and abs(float(a["ecd1.0.0.kernel"].sum()) - 1) < 1e-6


@pytest.mark.parametrize("tag", list(GM.CASES))
def test_mirror_on_the_cpu_against_the_model(tag):
    from e4s2024_amd import ops
    c = GM.case(tag)
    size, narrow, sdim, _ = GM.CASES[tag]
    net = ops.GPEN(size, sdim, GM.N_MLP, 2, narrow).eval()
    net.load_state_dict(c["sd"], strict=True)
    out, latent = net(T(c["x"]), return_latents=True)
    assert net(T(c["x"]))[1] is None
    assert GM.max_err(out.numpy(), c["want"]) <= GM.bound(c["e32"], c["want"])
    assert GM.max_err(latent.numpy(), c["latent"]) <= GM.bound(c["e32_latent"], c["latent"])
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(c["x"]))


def test_uint8_ends_reproduce_numpy_on_all_levels():
    img = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    x = GM.img2tensor(img)
    want = ((img.astype(np.float32) / np.float32(255.)) - np.float32(0.5)) / np.float32(0.5)
    assert x.dtype == np.float32 and np.array_equal(x, want.transpose(0, 3, 1, 2))
    assert x.min() == -1 and x.max() == 1
    # torch on the CPU, as FaceGAN.img2tensor runs it for the fixture: the same bits
    t = (torch.from_numpy(img) / 255. - 0.5) / 0.5
    assert torch.equal(t.permute(0, 3, 1, 2), T(x))
    # the way back is the identity on every level, in float32 as in float64, and follows NumPy's expression
    back = GM.tensor2img(x)
    assert back.dtype == np.uint8 and np.array_equal(back, (np.clip(x.transpose(0, 2, 3, 1) * 0.5 + 0.5, 0, 1) * 255.0).astype(np.uint8))
    assert np.abs(back.astype(int) - img.astype(int)).max() <= 1                               # (truncation: a level may land one below)
    assert np.array_equal(GM.expected_u8(GM.to_u(np.array([[[[-3.0]], [[0.0]], [[3.0]]]]))), np.uint8([[[[0, 127, 255]]]]))


@pytest.mark.parametrize("tag", ["s16", "s64"])
def test_image_cases_are_well_conditioned(tag):
    c = GM.case(tag)
    strict = GM.strict_pixels(c["u"], c["e32"])
    print(f"{tag}: {strict.mean():.4f} of the values are strict, margin {GM.MARGIN * c['e32'] * 127.5:.2e} levels")
    assert strict.mean() >= 0.99
    want = GM.expected_u8(c["u"])
    assert want.std() > 30 and np.array_equal(GM.check_u8(want, c["u"], c["e32"]) >= 0.99, True)
    off = want.copy()
    off[~strict] = np.clip(off[~strict].astype(int) + 1, 0, 255).astype(np.uint8)             # allowed: one level on a value that is not strict
    GM.check_u8(off, c["u"], c["e32"])
    bad = want.copy()
    i = tuple(np.argwhere(strict & (want < 255))[0])
    bad[i] += 1
    with pytest.raises(AssertionError, match="strict"):
        GM.check_u8(bad, c["u"], c["e32"])


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_gpen, pipeline
    for name in ("GPEN", "PreparedGPEN", "gpen_state_dict_shapes", "gpen_weight_tensors", "gpen_forward", "gpen_image", "gpen_to_u8"):
        assert name in ops_gpen.__all__ and getattr(ops, name) is getattr(ops_gpen, name)
    assert ops_gpen.ARITH == "sb" and callable(pipeline.gpen_enhance)
    assert e4s2024_amd.GPEN_OVERRIDES == {"swap_face_fine.gpen.face_model.gpen_model": "swap_face_fine/gpen/face_model/gpen_model.py"}
    assert set(e4s2024_amd.GPEN_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert "GPEN_OVERRIDES" in e4s2024_amd.install.__doc__
    assert e4s2024_amd.ENHANCE_OVERRIDES == {"swap_face_fine.realesr.image_infer": "swap_face_fine/realesr/image_infer.py"}
    assert not any(m.startswith("swap_face_fine.gpen.face_model.op") for m in e4s2024_amd._redirected())


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert [len(_lib._PROTOS[n]) for n in sorted(ENTRY_POINTS)] == [12, 10, 6]


def test_dropin_resolves_and_imports_without_cv2_or_torchvision():
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    from swap_face_fine.gpen.face_model import gpen_model
    assert gpen_model.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    assert "cv2" not in sys.modules and "torchvision" not in sys.modules and "swap_face_fine.gpen.face_model.op" not in sys.modules
    from e4s2024_amd import ops
    full = gpen_model.FullGenerator(16, 32, GM.N_MLP, channel_multiplier=2, narrow=1 / 32, device="cuda")
    assert isinstance(full, ops.GPEN) and list(full.state_dict()) == list(GM.case("s16")["sd"])
    full.load_state_dict(GM.case("s16")["sd"], strict=True)
    x = T(GM.case("s16")["x"])
    for kwargs, why in ((dict(truncation=0.5), "truncation"), (dict(inject_index=3), "inject_index"), (dict(input_is_latent=True), "input_is_latent")):
        with pytest.raises(NotImplementedError, match=why):
            full.eval()(x, **kwargs)
    with pytest.raises(NotImplementedError, match="eval"):
        full.train()(x)
    with pytest.raises(NotImplementedError, match="isconcat"):
        gpen_model.FullGenerator(16, 32, 8, isconcat=False)
    for name in ("FullGenerator_SR", "Generator", "Discriminator"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(gpen_model, name)(16, 32, 8)


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops
    c = GM.case("s16")
    net = ops.GPEN(16, 32, GM.N_MLP, 2, 1 / 32).eval()
    x = T(c["x"])
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.gpen_forward(x, net)
    net.load_state_dict(c["sd"], strict=True)
    with pytest.raises(RuntimeError, match="CUDA"):                                           # a CPU tensor
        ops.gpen_forward(x, net)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.gpen_image(T(c["img"]), net)
    with pytest.raises(ValueError, match="float32"):
        ops.gpen_forward(x.double(), net)
    with pytest.raises(ValueError, match="size is 16"):
        ops.gpen_forward(x[:, :, :, :8], net)
    with pytest.raises(ValueError, match="size is 16"):
        ops.gpen_image(T(c["img"])[:, :8], net)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.gpen_forward(x, net.train())
    with pytest.raises(KeyError, match="ecd0.0.0.weight"):
        ops.gpen_forward(x, {"conv.weight": x})
    sd = dict(c["sd"])
    del sd["generator.convs.1.noise.weight"]
    with pytest.raises(KeyError, match="noise.weight"):
        ops.gpen_forward(x, sd)
    assert [tuple(t.shape) for t in ops.gpen_weight_tensors(c["sd"])] == [tuple(v.shape) for v in c["sd"].values()]


def test_a_module_hands_over_its_own_configuration():
    """``narrow`` and ``channel_multiplier`` cannot be read back off the shapes where ``int()`` truncated: at (64, multiplier 3, narrow 0.3) the 64 x 64 level
    has int(768 * 0.3) = 230 channels, and 153 / 512 read off the 4 x 4 level would give 229.  A module is checked against what it was built with."""
    from e4s2024_amd import ops, ops_gpen
    net = ops.GPEN(64, 32, 2, 3, 0.3).eval()
    assert net.ecd0[0][0].weight.shape[0] == 230 and net.generator.input.input.shape[1] == 153
    ts = ops.gpen_weight_tensors(net)
    assert [tuple(t.shape) for t in ts] == [tuple(v.shape) for v in net.state_dict().values()]
    assert ops_gpen._net_of(net) is ops_gpen._net_of(ops.GPEN(64, 32, 2, 3, 0.3)) and ops_gpen._net_of({}) is ops_gpen._GPEN_NET
    assert ops_gpen._validated("gpen_forward", net, ops_gpen._net_of(net))[1] == (64, 32, 2, 3, 0.3)
