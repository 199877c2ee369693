"""Row f17 (face-vid2vid's keypoint detector, head-pose estimator and keypoint transformation) without a GPU: the reference's stored outputs against the float64
restatement ``vid2vid_kp_model``, the conditions that keep a pass from being empty, the bars of the GPU tests pinned from the other side by single-change
mutants, the mirror modules' keys against the reference's, the mirrors on stock PyTorch, the seeded weights, the drop-in and the argument errors that must raise
before any launch.

The bar of a case and output is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64 — never the code under test."""
import numpy as np
import pytest
import torch

import vid2vid_kp_model as M
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_conv3d_prep_weights_sb3": 14, "e4s_conv3d_sb3": 16, "e4s_v2v_antialias_down": 9, "e4s_avgpool2x2": 6, "e4s_v2v_heatmap_kp": 12,
                "e4s_v2v_kp_transform": 17}
NETS = list(M.KP_CASES) + list(M.HE_CASES)


@pytest.fixture(scope="module")
def golden():
    return load_golden("g28_vid2vid_kp")


def _outputs(tag):
    return M.KP_OUTPUTS if tag in M.KP_CASES else M.HE_OUTPUTS


def _stored(golden, tag):
    return {k: golden[f"{tag}.{k}"] for k in _outputs(tag) if f"{tag}.{k}" in golden.files}


@pytest.mark.parametrize("tag", NETS)
def test_reference_outputs_lie_within_the_bound_of_the_model(tag, golden):
    c = M.case(tag)
    assert np.array_equal(golden[f"{tag}.img"], c["img"])                                      # the same seeded input as when the fixture was made
    ref = _stored(golden, tag)
    assert set(ref) == {k for k in _outputs(tag) if c["out64"][k] is not None}
    for k, got in ref.items():
        want = c["out64"][k]
        assert got.dtype == np.float32 and got.shape == want.shape
        e = M.max_err(got, want)
        print(f"{tag}.{k}: the reference against the model {e:.3e} = {e / c['e32'][k]:.2f} e32, std {want.std():.3f}")
        assert e <= M.bound(c["e32"][k], want)
    if tag == M.STORED_VOLUME:
        for k in ("prediction", "heatmap"):
            assert M.max_err(golden[f"{tag}.{k}"], c["out64"][k]) <= M.bound(c["e32"][k], c["out64"][k])
    assert not any(f"{t}.{k}" in golden.files for t in M.KP_CASES if t != M.STORED_VOLUME for k in ("prediction", "heatmap"))


def test_volumes_of_the_cases():
    from e4s2024_amd import ops
    want = {"K-A": (4, 16, 16), "K-B": (3, 24, 40), "K-C": (2, 12, 8)}
    for tag, vol in want.items():
        assert M.case(tag)["out64"]["prediction"].shape[2:] == vol
        assert ops.kp_volume_size(M.make_module(tag).structure, *M.KP_CASES[tag][1][1:]) == vol
    assert M.case("K-B")["sd"]["predictor.up_blocks.up0.conv.weight"].shape[1] == 48 and M.case("K-B")["sd"]["kp.weight"].shape[1] == 12


@pytest.mark.parametrize("tag", list(M.CASES))
def test_conditions_that_keep_a_pass_from_being_empty(tag, golden):
    """On the model's outputs and, for the networks, on the reference's stored ones: heatmaps neither one-hot nor uniform, pose softmaxes over at least three
    bins, degrees spread over at least 20, and every output well conditioned (e32 <= 1e-4 of its standard deviation)."""
    c = M.case(tag)
    info = M.check_conditions(tag, c["out64"], c["out64"].get("heatmap"))
    if tag in M.HE_CASES:
        info = M.check_conditions(tag, _stored(golden, tag))
    if tag == M.STORED_VOLUME:
        info = M.check_conditions(tag, _stored(golden, tag), golden[f"{tag}.heatmap"])
    print(tag, info)
    if tag == "T-hand":
        deg = c["out64"]["deg"]
        assert deg.min() <= -55 and deg.max() >= 55
    if tag == "T-free":
        assert np.array_equal(c["out64"]["deg"][:, :2], np.array([[20.0, -35.0]] * 2)) and c["out64"]["deg"][:, 2].std() > 0


@pytest.mark.parametrize("tag", [t for t in M.T_CASES if M.T_CASES[t][0] != "hand"])
def test_transformation_of_the_model_on_the_stored_head_outputs(tag, golden):
    """What the GPU test is held to: the float64 transformation of the reference's stored head outputs and keypoints, well conditioned and near the model's own."""
    c = M.case(tag)
    he_tag, kp_tag, _ = M.T_CASES[tag]
    n = c["kp"].shape[0]
    t = M.transform_outputs(c, he={k: golden[f"{he_tag}.{k}"] for k in M.HE_OUTPUTS}, kp=golden[f"{kp_tag}.value"][:n],
                            jac=None if c["jac"] is None else golden[f"{kp_tag}.jacobian"][:n])
    for k, e in t["e32"].items():
        assert e <= 1e-4 * t["out64"][k].std()
        assert M.max_err(t["out64"][k], c["out64"][k]) <= 1e-3 * c["out64"][k].std()          # the float32 inputs moved the result by little


def test_every_mutant_is_a_hundred_bars_from_the_fixture_on_its_case(golden):
    assert set(M.MUTANTS) >= {"heads_uncrossed", "pi", "roll_pitch_yaw", "minus_96", "temperature_dropped", "softmax_per_slice", "grid_half_pixel", "grid_zyx",
                              "trilinear_up", "depth_up", "maxpool_down", "aa_no_zero_pad", "aa_sigma_2", "aa_from_2", "bn_eps_1e3", "relu_after_add_dropped",
                              "skip_norm4_dropped", "exp_before_rotation", "jacobian_from_the_right"}
    assert M.MUTANT_MARGIN == 100.0
    for m, (tag, name) in M.MUTANTS.items():
        c = M.case(tag)
        want = c["out64"][name] if tag in M.T_CASES else golden[f"{tag}.{name}"]               # (the transformation has no stored reference: its inputs are)
        bars = M.max_err(M.mutant_output(m), want) / M.bound(c["e32"][name], c["out64"][name])
        print(f"mutant {m} on {tag}.{name}: {bars:.0f} bars from the fixture")
        assert bars >= M.MUTANT_MARGIN, m


def _want_keys(golden, which):
    lines = str(golden[which]).split("\n")
    return [(ln.split("|")[0], tuple(int(d) for d in ln.split("|")[1].split("x") if d)) for ln in lines]


def test_mirrors_have_the_reference_keys_in_order(golden):
    from e4s2024_amd import ops
    buffers = ("running_mean", "running_var", "num_batches_tracked", "down.weight")
    for which, cls, shapes, count, params in (("keys.kp", ops.KPDetector, ops.kp_detector_state_dict_shapes, 75, 41940047),
                                              ("keys.he", ops.HEEstimator, ops.he_estimator_state_dict_shapes, 402, 30254838)):
        want = _want_keys(golden, which)
        with torch.device("meta"):
            sd = cls().state_dict()
        assert len(want) == count and [(k, tuple(v.shape)) for k, v in sd.items()] == want
        assert list(shapes().items()) == want                                                  # what a mapping's keys are checked against
        assert sum(int(np.prod(s)) for k, s in want if not k.endswith(buffers)) == params
        assert all(v.dtype == (torch.long if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    assert dict(_want_keys(golden, "keys.kp"))["down.weight"] == (3, 1, 13, 13)
    for tag in NETS:                                                                           # and at the cases' configurations, through the structure
        net = M.make_module(tag)
        fn = ops.kp_detector_structure_shapes if tag in M.KP_CASES else ops.he_estimator_structure_shapes
        assert list(fn(net.structure).items()) == [(k, tuple(v.shape)) for k, v in net.state_dict().items()]


def test_structure_read_off_a_mapping():
    from e4s2024_amd import ops_reenact
    for tag in NETS:
        net = M.make_module(tag)
        fn = ops_reenact._kp_structure_of_keys if tag in M.KP_CASES else ops_reenact._he_structure_of_keys
        assert fn("t", M.state_dict(tag)) == net.structure
        assert fn("t", net.state_dict()) == net.structure


def test_antialias_buffer_is_the_modules_gaussian():
    from e4s2024_amd import ops
    k = ops.antialias_kernel(0.25)
    assert k.shape == (13, 13) and k.dtype == torch.float32 and abs(float(k.sum()) - 1) < 1e-6
    want = np.exp(-(np.arange(13) - 6.0) ** 2 / (2 * 1.5 ** 2))
    want = np.outer(want, want) / np.outer(want, want).sum()
    assert np.abs(k.numpy() - want).max() < 1e-7                                               # sigma 1.5, 13 x 13, normalised
    assert torch.equal(M.state_dict("K-A")["down.weight"], k.view(1, 1, 13, 13).repeat(3, 1, 1, 1))
    assert torch.equal(ops.KPDetector().down.weight[1, 0], k) and ops.antialias_kernel(0.5).shape == (5, 5)
    assert "down.weight" not in M.state_dict("K-B")                                            # scale_factor 1: no buffer


def test_seeded_weights():
    from e4s2024_amd import seeded
    assert {"seeded_kp_detector_state_dict", "seeded_he_estimator_state_dict"} <= set(seeded.__all__)
    for tag, fn, probe in (("K-A", seeded.seeded_kp_detector_state_dict, "predictor.up_blocks.up1.conv.weight"),
                           ("H-B", seeded.seeded_he_estimator_state_dict, "block4.conv2.weight")):
        with torch.device("meta"):
            template = M.make_module(tag).state_dict()
        a, b = fn(template, 5), fn(template, 5)
        assert list(a) == list(template) and all(torch.equal(a[k], b[k]) for k in a)
        assert not torch.equal(a[probe], fn(template, 6)[probe])
        scales = [v for k, v in a.items() if k.split(".")[-2].startswith("norm") and k.endswith(".weight")]
        assert scales and all(int((v == 0).sum()) == 1 and float(v.abs().max()) <= 1.5 for v in scales)      # one exact zero per layer, within +-1.5
        assert 0.4 <= float(torch.cat(scales).lt(0).float().mean()) <= 0.6                                   # both signs
        assert all(float(v.min()) >= 0.5 for k, v in a.items() if k.endswith("running_var"))
        assert all(float(v.abs().max()) > 0.05 for k, v in a.items() if k.endswith(("running_mean", ".bias")))
        assert all(v.dtype == torch.long for k, v in a.items() if k.endswith("num_batches_tracked"))
    assert seeded.V2V_KP_HEAD_GAIN > 1.0                                                       # chosen for the heatmap condition, not the He gain


@pytest.mark.parametrize("tag", NETS)
def test_mirror_on_the_cpu_against_the_model(tag):
    c = M.case(tag)
    net = M.make_module(tag)
    net.load_state_dict(c["sd"], strict=True)
    out = net(T(c["x"]))
    assert set(out) == {k for k in _outputs(tag) if c["out64"][k] is not None}
    for k, got in out.items():
        assert got.dtype == torch.float32 and M.max_err(got.numpy(), c["out64"][k]) <= M.bound(c["e32"][k], c["out64"][k]), k
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(c["x"]))


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_reenact, pipeline
    for name in ("KPDetector", "HEEstimator", "PreparedKPDetector", "PreparedHEEstimator", "kp_detector_forward", "he_estimator_forward", "headpose_degrees",
                 "rotation_matrix", "keypoint_transformation", "reenact_keypoints", "conv3d_sb3", "prep_conv3d", "heatmap_keypoints", "antialias_down",
                 "avgpool2x2", "kp_detector_state_dict_shapes", "he_estimator_state_dict_shapes"):
        assert name in ops_reenact.__all__ and getattr(ops, name) is getattr(ops_reenact, name)
    assert callable(pipeline.reenact_keypoints)
    assert e4s2024_amd.REENACT_KP_OVERRIDES == {
        "swap_face_fine.face_vid2vid.modules.keypoint_detector": "swap_face_fine/face_vid2vid/modules/keypoint_detector.py"}
    assert set(e4s2024_amd.REENACT_KP_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert "REENACT_KP_OVERRIDES" in e4s2024_amd.install.__doc__
    assert not any(m.endswith(("sync_batchnorm", "modules.util")) for m in e4s2024_amd._redirected())


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert {n: len(_lib._PROTOS[n]) for n in ENTRY_POINTS} == ENTRY_POINTS
    assert "f17" in src
    cdll = _lib.lib().cdll
    assert all(hasattr(cdll, name) for name in ENTRY_POINTS)


def test_dropin_resolves_and_imports_without_sync_batchnorm():
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    from swap_face_fine.face_vid2vid.modules import keypoint_detector as kd
    assert kd.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    assert not any(m.startswith("swap_face_fine.face_vid2vid.sync_batchnorm") or m == "swap_face_fine.face_vid2vid.modules.util" for m in sys.modules)
    from e4s2024_amd import ops
    cfg = M.kp_config("K-A")
    net = kd.KPDetector(cfg["block_expansion"], 32, cfg["num_kp"], 3, cfg["max_features"], cfg["reshape_channel"], cfg["reshape_depth"], cfg["num_blocks"], 0.1,
                        estimate_jacobian=True, scale_factor=0.25)
    assert isinstance(net, ops.KPDetector) and list(net.state_dict()) == list(M.case("K-A")["sd"])
    net.load_state_dict(M.case("K-A")["sd"], strict=True)
    he = kd.HEEstimator(64, 32, 5, 3, 2048)
    assert isinstance(he, ops.HEEstimator) and list(he.state_dict()) == list(M.case("H-B")["sd"])
    he.load_state_dict(M.case("H-B")["sd"], strict=True)
    for mod, tag in ((net, "K-A"), (he, "H-B")):
        x = T(M.case(tag)["x"])
        with pytest.raises(NotImplementedError, match="eval"):
            mod.train()(x)
        with pytest.raises(RuntimeError, match="CUDA"):                                       # eval: the native forward, which refuses a CPU tensor
            mod.eval()(x)
    with pytest.raises(TypeError):
        kd.KPDetector()                                                                       # the reference's signature has no defaults for the widths
    with pytest.raises(ValueError, match="single_jacobian_map"):
        kd.KPDetector(8, 32, 5, 3, 32, 128, 4, 3, 0.1, estimate_jacobian=True, single_jacobian_map=True)


def test_configurations_refused_by_name():
    from e4s2024_amd import ops
    ok = M.kp_config("K-A")
    for change, why in ((dict(single_jacobian_map=True), "single_jacobian_map"), (dict(scale_factor=0.3), "scale_factor"), (dict(scale_factor=2), "scale_factor"),
                        (dict(reshape_channel=96), "reshape_channel"), (dict(reshape_depth=1, reshape_channel=32), "reshape_depth"),
                        (dict(image_channel=1), "image_channel"), (dict(temperature=0), "temperature")):
        with pytest.raises(ValueError, match=why):
            ops.KPDetector(**{**ok, **change})
    with pytest.raises(ValueError, match="image_channel"):
        ops.HEEstimator(image_channel=4)
    assert ops.KPDetector(**{**ok, "scale_factor": 0.5}).down.weight.shape == (3, 1, 5, 5)


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops, pipeline
    ck, ch = M.case("K-A"), M.case("H-B")
    kp, he = M.make_module("K-A"), M.make_module("H-B")
    xk, xh = T(ck["x"]), T(ch["x"])
    for call in (lambda: ops.kp_detector_forward(xk, kp), lambda: ops.he_estimator_forward(xh, he)):
        with pytest.raises(RuntimeError, match="never loaded"):
            call()
    kp.load_state_dict(ck["sd"], strict=True), he.load_state_dict(ch["sd"], strict=True)
    out_k = {k: T(v.astype(np.float32)) for k, v in ck["out64"].items() if k in M.KP_OUTPUTS}
    out_h = {k: T(v.astype(np.float32)) for k, v in ch["out64"].items()}
    for call in (lambda: ops.kp_detector_forward(xk, kp), lambda: ops.he_estimator_forward(xh, he), lambda: ops.kp_detector_forward(xk, ck["sd"]),
                 lambda: ops.he_estimator_forward(xh, {"he_estimator": ch["sd"]}), lambda: ops.keypoint_transformation({k: v[:1] for k, v in out_k.items()}, out_h),
                 lambda: ops.headpose_degrees(out_h), lambda: ops.rotation_matrix(out_h), lambda: ops.reenact_keypoints(xk[:1], xk, kp, he),
                 lambda: pipeline.reenact_keypoints(kp, he, xk[:1], xk)):
        with pytest.raises(RuntimeError, match="CUDA"):                                       # a CPU tensor
            call()
    for fn, x, net in ((ops.kp_detector_forward, xk, kp), (ops.he_estimator_forward, xh, he)):
        with pytest.raises(ValueError, match="float32"):
            fn(x.double(), net)
        with pytest.raises(ValueError, match="three colour"):
            fn(x[:, :2], net)
        with pytest.raises(RuntimeError, match="training mode"):
            fn(x, net.train())
        net.eval()
        with pytest.raises(TypeError, match="mapping"):
            fn(x, 3)
    with pytest.raises(ValueError, match="at least 2"):
        ops.kp_detector_forward(xk[:, :, :, :8], kp)                                          # 8 -> 2 -> 1 -> 0: no volume left
    with pytest.raises(ValueError, match="at least 2"):
        ops.kp_detector_forward(xk[:, :, :4, :], kp)                                          # 4 -> 1 -> 0
    with pytest.raises(KeyError, match="predictor"):
        ops.kp_detector_forward(xk, {"conv.weight": xk})
    with pytest.raises(KeyError, match="conv1.weight"):
        ops.he_estimator_forward(xh, {"conv.weight": xh})
    sd = dict(ck["sd"])
    del sd["predictor.up_blocks.up1.norm.running_var"]
    with pytest.raises(KeyError, match="running_var"):
        ops.kp_detector_forward(xk, sd)
    sd = dict(ch["sd"])
    sd["block2.skip.bias"] = sd["block2.skip.bias"].double()
    with pytest.raises(ValueError, match="block2.skip.bias"):
        ops.he_estimator_forward(xh, sd)
    with pytest.raises(ValueError, match="temperature"):
        ops.kp_detector_forward(xk, kp, temperature=-1.0)
    bad = dict(out_h, yaw=out_h["yaw"][:, :60])
    with pytest.raises(ValueError, match="66"):
        ops.keypoint_transformation({k: v[:1] for k, v in out_k.items()}, bad)
    with pytest.raises(ValueError, match="jacobian"):
        ops.keypoint_transformation({"value": out_k["value"][:1], "jacobian": out_k["jacobian"][:1, :, :2]}, out_h)
    with pytest.raises(ValueError, match=r"\[1, 3, H, W\]"):
        ops.reenact_keypoints(xk, xk, kp, he)
    t_before = out_h["t"].shape
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.keypoint_transformation({k: v[:1] for k, v in out_k.items()}, out_h)
    assert out_h["t"].shape == t_before                                                       # he['t'] is never reshaped in place
