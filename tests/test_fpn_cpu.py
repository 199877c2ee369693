"""Row f10 (Blender recolouring, stage 3) without a GPU: the float64 restatement ``fpn_model`` against the reference's own ``AdaptiveFeatureGenerator`` and
``SmallFPN`` (``g22_fpn.npz``), the bar of the GPU tests pinned from the other side by single-change mutants, the mirror modules, the drop-in's constructor,
the flip rule and the argument errors that must raise before any launch.

The bound of a case is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64 (the reference's arithmetic class, 1e-6 .. 1.4e-5
over the cases, computed here).  Every mutant of the model moves the float64 output by at least ten bounds on some case (measured: 4168 bounds for the
nearest one, eps 1e-3, on the 2 x 2 feature map; a rounding nearest index shows only where the sizes do not divide, at 34 x 26), so a kernel inside the
bound has none of these mistakes."""
import argparse

import numpy as np
import pytest
import torch

import fpn_model as FM
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_spade_shared", "e4s_spade_modulate"}
DEFAULTS = FM.PARSER_DEFAULTS


def _keys(g, name):
    return [(line.split("|")[0], tuple(int(d) for d in line.split("|")[1].split("x") if d)) for line in str(g[name]).split("\n")]


@pytest.mark.parametrize("tag", FM.SMALL_CASES)
def test_model_against_the_reference(tag):
    g = load_golden("g22_fpn")
    assert FM.crc(FM.case_inputs(tag)) == int(g[f"{tag}.crc"]), "the seeded inputs are not the ones the fixture was made from"
    out = FM.reference_output(tag)
    H, W, bs, _ = FM.CASES[tag]
    assert out.shape == (bs, 256) + FM.out_size(H, W) and g[f"{tag}.out"].dtype == np.float32
    err, e32 = FM.max_err(out, g[f"{tag}.out"]), FM.e32(tag)
    print(f"{tag}: model against the reference {err:.3e} (when the fixture was made {float(g[f'{tag}.ref_err']):.3e}), e32 {e32:.3e} (then "
          f"{float(g[f'{tag}.e32']):.3e}), bound {FM.bound(e32, out):.3e}")
    assert err <= FM.bound(e32, out)
    assert e32 <= 1e-3 * out.std()                                                            # the case is well conditioned


def test_fixture_of_the_large_case():
    g = load_golden("g22_fpn")
    tag = "256x256"
    assert FM.crc(FM.case_inputs(tag)) == int(g[f"{tag}.crc"])
    assert g[f"{tag}.out"].shape == (FM.SAMPLED[tag],) and len(np.unique(FM.sample_positions(tag))) == FM.SAMPLED[tag]
    e32, ref_err, absmax = (float(g[f"{tag}.{k}"]) for k in ("e32", "ref_err", "absmax"))
    assert 0 < ref_err <= max(FM.MARGIN * e32, FM.FLOOR * absmax) and e32 <= 1e-3 * g[f"{tag}.out"].std()


def test_flipped_target_against_the_reference():
    g = load_golden("g22_fpn")
    tag = "20x12"
    x = FM.case_inputs(tag)
    feats_a, feats_t = FM.features(FM.state_dict(), x, x, True)
    bound = FM.bound(FM.e32(tag), feats_t)
    assert FM.max_err(feats_a, g[f"{tag}.out"]) <= bound and FM.max_err(feats_t, g[f"{tag}.flip.out"]) <= bound
    assert FM.max_err(FM.features(FM.state_dict(), x, x, False)[1], g[f"{tag}.out"]) <= bound


def test_every_mutant_is_ten_bounds_away_on_some_case():
    g = load_golden("g22_fpn")
    tags = [t for t in FM.SMALL_CASES if not FM.CASES[t][3]]
    worst = {}
    for mutant in FM.MUTANTS:
        for tag in tags if mutant != "features_flipped_back" else ["20x12"]:
            x, bound = FM.case_inputs(tag), FM.bound(FM.e32(tag), FM.reference_output(tag))
            if mutant == "features_flipped_back":
                moved = FM.max_err(FM.features(FM.state_dict(), x, x, True, mutant=mutant)[1], g[f"{tag}.flip.out"])
            else:
                moved = FM.max_err(FM.forward(FM.state_dict(), x, mutant=mutant), g[f"{tag}.out"])
            print(f"{tag}: {mutant} lies {moved:.3e} = {moved / bound:.0f} bounds from the fixture")
            worst[mutant] = max(worst.get(mutant, 0.0), moved / bound)
    assert all(v >= FM.MUTANT_MARGIN for v in worst.values()), worst


def test_seeded_spectral_norm_has_unit_vectors_and_sigma():
    from e4s2024_amd import seeded
    sd = FM.state_dict()
    prefixes = [k[:-len(".weight_orig")] for k in sd if k.endswith(".weight_orig")]
    assert len(prefixes) == 5 + 2 + 2 + 3
    for p in prefixes:
        w, u, v = (sd[p + s].double() for s in (".weight_orig", ".weight_u", ".weight_v"))
        assert abs(float(u.norm()) - 1) < 1e-6 and abs(float(v.norm()) - 1) < 1e-6
        assert abs(float(torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))) - seeded.FPN_SIGMA) < 1e-5
    assert seeded.FPN_SIGMA != 1.0 and {"seeded_fpn_state_dict", "seeded_small_fpn_state_dict"} <= set(seeded.__all__)
    again = seeded.seeded_fpn_state_dict(FM.WEIGHT_SEED)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["layer3.0.weight_orig"], seeded.seeded_fpn_state_dict(FM.WEIGHT_SEED + 1)["layer3.0.weight_orig"])


@pytest.mark.parametrize("small", [False, True])
def test_mirror_has_the_reference_keys_and_shapes(small):
    from e4s2024_amd import ops
    g = load_golden("g22_fpn")
    want = _keys(g, "keys.small" if small else "keys.fpn")
    net = ops.SmallFPN() if small else ops.BlenderFPN()
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    assert list(ops.fpn_state_dict_shapes(small).items()) == want
    net.load_state_dict(FM.state_dict(small), strict=True)
    if not small:
        assert not any(k.startswith("layer") and k.endswith("bias") for k, _ in want) and "head_0.conv_0.bias" in dict(want) and "G_middle_1.conv_s.bias" not in dict(want)
    prefixed = {"referencer.FPN." + k: v for k, v in FM.state_dict(small).items()}            # latest_netG.pth's entries: the prefix taken off
    type(net)().load_state_dict({k[len("referencer.FPN."):]: v for k, v in prefixed.items()}, strict=True)
    whole = ops.BlenderNet(small_FPN=small).state_dict()
    assert {k[len("referencer.FPN."):] for k in whole if k.startswith("referencer.FPN.")} == set(dict(want)) and "referencer.trainable_tao" in whole
    assert {k[len("unet."):] for k in whole if k.startswith("unet.")} == set(ops.resunet_state_dict_shapes(16 if small else 64))


@pytest.mark.parametrize("tag", FM.SMALL_CASES)
def test_mirror_on_the_cpu_against_the_model(tag):
    from e4s2024_amd import ops
    small = FM.CASES[tag][3]
    net = (ops.SmallFPN() if small else ops.BlenderFPN()).eval()
    net.load_state_dict(FM.state_dict(small))
    x = T(FM.case_inputs(tag))
    with torch.no_grad():
        got = net(x).numpy()
        assert np.array_equal(got, net(x, x).numpy())
    want = FM.reference_output(tag)
    err, e32 = FM.max_err(got, want), FM.e32(tag)
    print(f"{tag}: the mirror in float32 against the model {err:.3e} = {err / e32:.2f} e32")
    assert err <= FM.bound(e32, want)


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_recolor, pipeline
    for name in ("BlenderFPN", "SmallFPN", "BlenderNet", "PreparedFPN", "fpn_state_dict_shapes", "blender_fpn", "blender_features", "blender_forward",
                 "flip_choice", "FPN_CHANNELS"):
        assert name in ops_recolor.__all__ and getattr(ops, name) is getattr(ops_recolor, name)
    assert e4s2024_amd.RECOLOR_FPN_OVERRIDES == {"swap_face_fine.Blender.model_center.backbone": "swap_face_fine/Blender/model_center/backbone.py"}
    assert set(e4s2024_amd.RECOLOR_FPN_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert callable(pipeline.blender_infer_image) and pipeline.BLENDER_SIZE == 256


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)


def _dropin():
    from conftest import install_dropin
    install_dropin()
    import e4s2024_amd
    from swap_face_fine.Blender.model_center import backbone
    assert backbone.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    return backbone


def test_dropin_accepts_the_defaults_and_has_the_reference_keys():
    m = _dropin()
    g = load_golden("g22_fpn")
    net = m.AdaptiveFeatureGenerator(argparse.Namespace(**DEFAULTS))
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == _keys(g, "keys.fpn")
    net.load_state_dict(FM.state_dict(), strict=True)
    small = m.SmallFPN()
    assert [(k, tuple(v.shape)) for k, v in small.state_dict().items()] == _keys(g, "keys.small")
    small.load_state_dict(FM.state_dict(True), strict=True)
    x = T(FM.case_inputs("8x8.b2"))
    for n in (net, small):
        with pytest.raises(NotImplementedError, match="eval"):
            n.train()(x, x)
    with pytest.raises(NotImplementedError, match="image itself"):
        net.eval()(x, x + 1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):                          # as far as a machine without the device goes
        net.eval()(x, x.clone())


@pytest.mark.parametrize("option,value", [("eqlr_sn", True), ("adaptor_nonlocal", True), ("adaptor_se", True), ("adaptor_res_deeper", True), ("PONO", True),
                                          ("warp_stride", 2), ("adaptor_kernel", 4), ("norm_G", "spectralspadesyncbatch3x3"),
                                          ("norm_G", "spadeinstance3x3"), ("norm_E", "spectralbatch"), ("ngf", 32)])
def test_dropin_refuses_every_unsupported_option(option, value):
    m = _dropin()
    with pytest.raises(ValueError, match=option):
        m.AdaptiveFeatureGenerator(argparse.Namespace(**{**DEFAULTS, option: value}))


def test_flip_rule_is_the_references_and_takes_one_draw():
    from e4s2024_amd import ops
    for seed in range(40):
        np.random.seed(seed)
        flipped = ops.flip_choice(None)
        after = np.random.rand()
        np.random.seed(seed)
        draw = np.random.rand()
        assert flipped == (not draw < 0.5)                                                   # referencer.py:32: below 0.5 the target is taken as it is
        assert after == np.random.rand()                                                     # exactly one draw was consumed
    np.random.seed(3)
    state = np.random.get_state()[1].copy()
    assert ops.flip_choice(True) is True and ops.flip_choice(False) is False
    assert np.array_equal(state, np.random.get_state()[1])                                   # a decided flip draws nothing
    with pytest.raises(TypeError):
        ops.flip_choice(1)


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops
    net = ops.SmallFPN().eval()
    net.load_state_dict(FM.state_dict(True))
    good = T(FM.case_inputs("8x8.b2"))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):                           # CPU tensors are refused once everything else is in order
        ops.blender_fpn(good, net)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_fpn(good, FM.state_dict(True))                                            # a mapping serves as weights too
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_fpn(good, {"referencer.FPN." + k: v for k, v in FM.state_dict(True).items()})
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_fpn(good, {"FPN." + k: v for k, v in FM.state_dict(True).items()})
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_fpn(good.transpose(2, 3), net)                                            # non-contiguous input is accepted as far as the checks go
    with pytest.raises(TypeError):
        ops.blender_fpn(good.numpy(), net)
    with pytest.raises(TypeError):
        ops.blender_fpn(good, None)
    with pytest.raises(KeyError, match="layer1.0.weight_orig"):
        ops.blender_fpn(good, {"conv.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="conv2.bias"):
        ops.blender_fpn(good, {k: v for k, v in FM.state_dict(True).items() if k != "conv2.bias"})
    with pytest.raises(ValueError, match="conv1.weight"):
        ops.blender_fpn(good, {**FM.state_dict(True), "conv1.weight": torch.zeros(256, 3, 3, 3)})
    with pytest.raises(ValueError, match="float32"):
        ops.blender_fpn(good.double(), net)
    with pytest.raises(ValueError, match="float32"):
        ops.blender_fpn(good[0], net)                                                         # rank
    with pytest.raises(ValueError, match=r"\[bs, 3, H, W\]"):
        ops.blender_fpn(torch.zeros(1, 4, 8, 8), net)
    with pytest.raises(ValueError, match="at least 2 x 2"):
        ops.blender_fpn(torch.zeros(1, 3, 4, 8), net)                                         # 4 -> 2 -> 1
    with pytest.raises(ValueError, match="at least 2 x 2"):
        ops.blender_fpn(torch.zeros(1, 3, 8, 0), net)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.blender_fpn(good, ops.SmallFPN())
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.blender_fpn(good, ops.SmallFPN().eval().to("meta"))
    # blender_features
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_features(good, good, net, True)
    with pytest.raises(TypeError, match="flip_target"):
        ops.blender_features(good, good, net, 1)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.blender_features(good, good[:1], net)
    with pytest.raises(ValueError, match="float32"):
        ops.blender_features(good, good.double(), net)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.blender_features(good, good, ops.SmallFPN())
    # blender_forward
    whole = ops.BlenderNet(small_FPN=True).eval()
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_forward(good, good, lab, lab, whole, True)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_forward(good, good, lab, lab, whole.state_dict(), False)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.blender_forward(good, good, lab, lab, ops.BlenderNet(small_FPN=True))
    with pytest.raises(TypeError, match="referencer.FPN"):
        ops.blender_forward(good, good, lab, lab, net)                                        # a bare feature network is not the whole model
    with pytest.raises(KeyError, match="trainable_tao"):
        ops.blender_forward(good, good, lab, lab, FM.state_dict(True))
    with pytest.raises(TypeError):
        ops.blender_forward(good, good, lab, lab, None)
    with pytest.raises(TypeError, match="flip_target"):
        ops.blender_forward(good, good, lab, lab, whole, "yes")
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.blender_forward(torch.zeros(1, 3, 12, 12), torch.zeros(1, 3, 12, 12), lab[:1], lab[:1], whole)
    with pytest.raises(ValueError, match="uint8"):
        ops.blender_forward(good, good, lab.float(), lab, whole)
    with pytest.raises(ValueError, match="float32"):
        ops.blender_forward(good, good.half(), lab, lab, whole)
