"""Row f18 (face-vid2vid's dense-motion network) without a GPU: the reference's stored outputs against the float64 restatement ``vid2vid_motion_model``, the
conditions that keep a pass from being empty, the bars of the GPU tests pinned from the other side by single-change mutants, the mirror module's keys against
the reference's, the mirror on stock PyTorch, the seeded weights, the drop-in and the argument errors that must raise before any launch.

The bar of a case and output is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64 — never the code under test."""
import numpy as np
import pytest
import torch

import vid2vid_motion_model as M
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_conv3d_k7_prep_weights_sb3": 8, "e4s_conv3d_k7_sb3": 15, "e4s_conv3d_sb3_strided": 19, "e4s_avgpool2x2_strided": 8,
                "e4s_v2v_motion_input": 14, "e4s_v2v_motion_combine": 13}
TAGS = list(M.CASES)


@pytest.fixture(scope="module")
def golden():
    return load_golden("g29_vid2vid_motion")


def _stored(golden, tag):
    return {k: golden[f"{tag}.{k}"] for k in M.OUTPUTS if f"{tag}.{k}" in golden.files}


@pytest.mark.parametrize("tag", TAGS)
def test_reference_outputs_lie_within_the_bound_of_the_model(tag, golden):
    c = M.case(tag)
    for k in ("kp_d", "kp_s", "jac_d", "jac_s"):                                              # the same seeded inputs as when the fixture was made
        assert (c[k] is None and f"{tag}.{k}" not in golden.files) or np.array_equal(golden[f"{tag}.{k}"], c[k])
    ref = _stored(golden, tag)
    assert set(ref) == {k for k in M.OUTPUTS if k in c["out64"]}
    assert ("occlusion_map" in ref) == M.CASES[tag][0]["estimate_occlusion_map"]
    for k, got in ref.items():
        want = c["out64"][k]
        assert got.dtype == np.float32 and got.shape == want.shape
        e = M.max_err(got, want)
        print(f"{tag}.{k}: the reference against the model {e:.3e} = {e / c['e32'][k]:.2f} e32, std {want.std():.3f}")
        assert e <= M.bound(c["e32"][k], want)
    assert not any(f.endswith((".feature", ".weight")) for f in golden.files)                 # neither weights nor volumes are stored


def test_shapes_of_the_cases():
    want = {"D-A": ((2, 6, 4, 16, 16), 30, 38), "D-B": ((1, 4, 3, 8, 24), 12, 18), "D-C": ((1, 6, 3, 12, 20), 30, 38), "D-D": ((1, 21, 4, 8, 20), 63, 67)}
    for tag, (mask, infe, outf) in want.items():
        c = M.case(tag)
        bs, _, d, h, w = mask
        assert c["out64"]["mask"].shape == mask and c["out64"]["deformation"].shape == (bs, d, h, w, 3)
        assert c["out64"]["input"].shape[1] == infe and c["out64"]["prediction"].shape[1] == outf
        if "occlusion_map" in c["out64"]:
            assert c["out64"]["occlusion_map"].shape == (bs, 1, h, w)
    assert M.case("D-D")["sd"]["mask.weight"].shape == (21, 67, 7, 7, 7)                      # the ragged 32-channel form of the 7-tap kernel


@pytest.mark.parametrize("tag", TAGS)
def test_conditions_that_keep_a_pass_from_being_empty(tag, golden):
    """On the model's outputs and on the reference's stored ones: 5 % .. 50 % of the sparse-motion sample points outside the volume, the mask neither one-hot
    nor uniform, the occlusion map over at least 0.2 .. 0.8, well-conditioned Jacobians, and every output well conditioned (e32 <= 1e-4 of its deviation)."""
    print(tag, M.check_conditions(tag, M.case(tag)["out64"]), M.check_conditions(tag, _stored(golden, tag)))


def test_every_mutant_is_a_hundred_bars_from_the_fixture_on_its_case(golden):
    assert set(M.MUTANTS) == {"align_corners_true", "border_padding", "grid_zyx", "kp_variance_01", "heatmap_source_minus_driving", "background_heatmap_nonzero",
                              "feature_then_heatmap", "jac_d_inv_s", "jacobian_after_kp_s", "softmax_over_depth", "deformation_without_background",
                              "pool_before_relu", "skip_in_front", "depth_pool_and_up", "bn_eps_1e3", "sigmoid_missing", "k7_pad_2"}
    assert M.MUTANT_MARGIN == 100.0
    for m, (tag, name) in M.MUTANTS.items():
        c = M.case(tag)
        bars = M.max_err(M.mutant_output(m), golden[f"{tag}.{name}"]) / M.bound(c["e32"][name], c["out64"][name])
        print(f"mutant {m} on {tag}.{name}: {bars:.0f} bars from the fixture")
        assert bars >= M.MUTANT_MARGIN, m


def _want_keys(golden):
    lines = str(golden["keys.dm"]).split("\n")
    return [(ln.split("|")[0], tuple(int(d) for d in ln.split("|")[1].split("x") if d)) for ln in lines]


def test_mirror_has_the_reference_keys_in_order(golden):
    from e4s2024_amd import ops, ops_reenact
    want = _want_keys(golden)
    with torch.device("meta"):
        sd = ops.DenseMotionNetwork().state_dict()
    assert len(want) == 88 and [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert list(ops.dense_motion_state_dict_shapes().items()) == want                         # what a mapping's keys are checked against
    assert sum(int(np.prod(s)) for k, s in want if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))) == 43545549
    assert all(v.dtype == (torch.long if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    assert dict(want)["mask.weight"] == (16, 112, 7, 7, 7) and dict(want)["occlusion.weight"] == (1, 1792, 7, 7)
    assert "occlusion.weight" not in ops.dense_motion_state_dict_shapes(estimate_occlusion_map=False)
    for tag in TAGS:                                                                          # at the cases' configurations, and read off a mapping
        net = M.make_module(tag)
        assert list(ops.dense_motion_structure_shapes(net.structure).items()) == [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert ops_reenact._dm_structure_of_keys("t", M.state_dict(tag)) == net.structure


def test_seeded_weights():
    from e4s2024_amd import seeded
    assert "seeded_dense_motion_state_dict" in seeded.__all__
    with torch.device("meta"):
        template = M.make_module("D-A").state_dict()
    a, b = seeded.seeded_dense_motion_state_dict(template, 5), seeded.seeded_dense_motion_state_dict(template, 5)
    assert list(a) == list(template) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["mask.weight"], seeded.seeded_dense_motion_state_dict(template, 6)["mask.weight"])
    scales = [v for k, v in a.items() if k.split(".")[-2] == "norm" and k.endswith(".weight")]
    assert len(scales) == 8 and all(int((v == 0).sum()) == 1 and float(v.abs().max()) <= 1.5 for v in scales)      # one exact zero per layer, within +-1.5
    assert all(float(v.min()) >= 0.5 for k, v in a.items() if k.endswith("running_var"))
    assert all(float(v.abs().max()) > 0.05 for k, v in a.items() if k.endswith(("running_mean", ".bias")))
    assert all(v.dtype == torch.long for k, v in a.items() if k.endswith("num_batches_tracked"))
    assert seeded.V2V_MASK_HEAD_GAIN > 1.0 and seeded.V2V_OCCLUSION_GAIN > 1.0                 # chosen for the mask and occlusion conditions, not the He gain


@pytest.mark.parametrize("tag", TAGS)
def test_mirror_on_the_cpu_against_the_model(tag):
    c = M.case(tag)
    net = M.make_module(tag)
    net.load_state_dict(c["sd"], strict=True)
    kd, ks = M.kp_dicts(tag)
    out = net(T(c["feature"]), kd, ks)
    assert list(out) == [k for k in M.OUTPUTS if k in c["out64"]]
    for k, got in out.items():
        assert got.dtype == torch.float32 and M.max_err(got.numpy(), c["out64"][k]) <= M.bound(c["e32"][k], c["out64"][k]), k
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(c["feature"]), kd, ks)


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_reenact, pipeline
    for name in ("DenseMotionNetwork", "PreparedDenseMotion", "dense_motion_state_dict_shapes", "dense_motion_forward", "conv3d_k7", "prep_conv3d_k7",
                 "motion_input", "motion_combine"):
        assert name in ops_reenact.__all__ and getattr(ops, name) is getattr(ops_reenact, name)
    assert callable(pipeline.reenact_dense_motion)
    assert e4s2024_amd.REENACT_MOTION_OVERRIDES == {
        "swap_face_fine.face_vid2vid.modules.dense_motion": "swap_face_fine/face_vid2vid/modules/dense_motion.py"}
    assert set(e4s2024_amd.REENACT_MOTION_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert "REENACT_MOTION_OVERRIDES" in e4s2024_amd.install.__doc__
    assert not any(m.endswith(("sync_batchnorm", "modules.util", "modules.generator")) for m in e4s2024_amd._redirected())


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert {n: len(_lib._PROTOS[n]) for n in ENTRY_POINTS} == ENTRY_POINTS
    assert "f18" in src and _lib.ABI_VERSION == 1
    cdll = _lib.lib().cdll
    assert all(hasattr(cdll, name) for name in ENTRY_POINTS)


def test_dropin_resolves_and_is_built_as_the_generator_builds_it():
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    from swap_face_fine.face_vid2vid.modules import dense_motion as dm
    assert dm.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    assert not any(m.startswith("swap_face_fine.face_vid2vid.sync_batchnorm") or m == "swap_face_fine.face_vid2vid.modules.util" for m in sys.modules)
    from e4s2024_amd import ops
    cfg = M.config("D-A")
    # modules/generator.py hands num_kp, feature_channel and estimate_occlusion_map over by name and the rest as **dense_motion_params
    params = {k: cfg[k] for k in ("block_expansion", "max_features", "num_blocks", "reshape_depth", "compress")}
    net = dm.DenseMotionNetwork(num_kp=cfg["num_kp"], feature_channel=cfg["feature_channel"], estimate_occlusion_map=True, **params)
    assert isinstance(net, ops.DenseMotionNetwork) and list(net.state_dict()) == list(M.case("D-A")["sd"])
    net.load_state_dict(M.case("D-A")["sd"], strict=True)
    assert dm.DenseMotionNetwork(8, 3, 32, 5, 8, 4, 4).occlusion is None                      # the reference's positional order, no occlusion head by default
    kd, ks = M.kp_dicts("D-A")
    x = T(M.case("D-A")["feature"])
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(x, kd, ks)
    with pytest.raises(RuntimeError, match="CUDA"):                                           # eval: the native forward, which refuses a CPU tensor
        net.eval()(x, kd, ks)
    with pytest.raises(TypeError):
        dm.DenseMotionNetwork()                                                               # the reference's signature has no defaults for the widths
    with pytest.raises(ValueError, match="num_kp"):
        dm.DenseMotionNetwork(8, 3, 32, 32, 8, 4, 4)


def test_refusals_by_name_before_any_launch():
    from e4s2024_amd import ops, pipeline
    c = M.case("D-B")
    net = M.make_module("D-B")
    x = T(c["feature"])
    kd, ks = M.kp_dicts("D-B")
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.dense_motion_forward(x, kd, ks, net)
    net.load_state_dict(c["sd"], strict=True)
    before = [{k: v.clone() for k, v in kp.items()} for kp in (kd, ks)]
    gen = {"dense_motion_network." + k: v for k, v in c["sd"].items()}
    for call in (lambda: ops.dense_motion_forward(x, kd, ks, net), lambda: ops.dense_motion_forward(x, kd, ks, c["sd"]),
                 lambda: ops.dense_motion_forward(x, kd, ks, gen), lambda: ops.dense_motion_forward(x, kd, ks, {"generator": gen}),
                 lambda: pipeline.reenact_dense_motion(net, x, kd, ks), lambda: ops.motion_input(T(c["out64"]["compressed"].astype(np.float32)), kd, ks),
                 lambda: ops.motion_combine(T(c["out64"]["logits"].astype(np.float32)), kd, ks)):
        with pytest.raises(RuntimeError, match="CUDA"):                                       # a CPU tensor: the last refusal
            call()
    fwd = lambda x=x, kd=kd, ks=ks, w=net: ops.dense_motion_forward(x, kd, ks, w)      # noqa: E731
    with pytest.raises(ValueError, match="multiples of 2"):                                   # (3, 10, 20) with two blocks: the reference's own torch.cat fails
        fwd(x=torch.zeros(1, 5, 3, 10, 20))
    with pytest.raises(ValueError, match="multiples of 2"):
        fwd(x=torch.zeros(1, 5, 3, 8, 22))
    with pytest.raises(ValueError, match="at least 2"):
        fwd(x=torch.zeros(1, 5, 1, 8, 24))
    with pytest.raises(ValueError, match="reshape_depth"):
        fwd(x=torch.zeros(1, 5, 4, 8, 24))
    with pytest.raises(ValueError, match="feature_channel"):
        fwd(x=torch.zeros(1, 6, 3, 8, 24))
    with pytest.raises(ValueError, match="float32"):
        fwd(x=x.double())
    with pytest.raises(ValueError, match="float32"):
        fwd(kd=dict(kd, value=kd["value"].double()))
    with pytest.raises(ValueError, match="float32"):
        fwd(ks=dict(ks, jacobian=ks["jacobian"].half()))
    with pytest.raises(ValueError, match="do not fit"):
        fwd(kd=dict(kd, value=kd["value"][:, :2]))
    with pytest.raises(ValueError, match="do not fit"):
        fwd(ks=dict(ks, value=torch.cat((ks["value"], ks["value"]))))
    with pytest.raises(ValueError, match="do not fit"):
        fwd(kd=dict(kd, jacobian=kd["jacobian"][:, :, :2]))
    with pytest.raises(ValueError, match="only one"):
        fwd(ks={"value": ks["value"]})
    with pytest.raises(ValueError, match="only one"):
        fwd(kd={"value": kd["value"], "jacobian": None})
    with pytest.raises(TypeError, match="keypoint dict"):
        fwd(kd=kd["value"])
    with pytest.raises(RuntimeError, match="training mode"):
        fwd(w=net.train())
    net.eval()
    with pytest.raises(TypeError, match="mapping"):
        fwd(w=3)
    with pytest.raises(KeyError, match="mask.weight"):
        fwd(w={"conv.weight": x})
    sd = dict(c["sd"])
    del sd["hourglass.decoder.norm.running_var"]
    with pytest.raises(KeyError, match="running_var"):
        fwd(w=sd)
    sd = dict(c["sd"])
    sd["compress.bias"] = sd["compress.bias"].double()
    with pytest.raises(ValueError, match="compress.bias"):
        fwd(w=sd)
    with pytest.raises(ValueError, match="num_kp"):
        ops.DenseMotionNetwork(num_kp=32)
    with pytest.raises(ValueError, match="num_kp"):
        ops.motion_combine(torch.zeros(1, 34, 2, 2, 2), {"value": torch.zeros(1, 33, 3)}, {"value": torch.zeros(1, 33, 3)})
    with pytest.raises(ValueError, match="7, 7"):
        ops.prep_conv3d_k7(torch.zeros(4, 4, 5, 5))
    assert all(torch.equal(v, was[k]) and v.shape == was[k].shape for kp, was in zip((kd, ks), before) for k, v in kp.items())      # the caller's dicts
    assert list(kd) == ["value", "jacobian"] and list(ks) == ["value", "jacobian"]
