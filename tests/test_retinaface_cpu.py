"""Row f14 (GPEN's RetinaFace detector) without a GPU: the reference's stored outputs against the float64 restatement ``retinaface_model``, the mirror module's
keys against the reference's, the mirror on stock PyTorch, the restated priors and NMS against the reference's bit for bit, the admission conditions of the
cases, the bars of the GPU tests pinned from the other side by single-change mutants, the drop-ins and the argument errors that must raise before any launch.

The bar of a case and output is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64 — never the code under test."""
import os

import numpy as np
import pytest
import torch

import retinaface_model as RM
from conftest import GOLDEN, load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_retina_input", "e4s_retina_up_add", "e4s_retina_cat_relu", "e4s_retina_priors", "e4s_retina_decode", "e4s_retina_compact", "e4s_retina_nms"}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g25_retinaface")


def _stored_detect(golden, tag, b):
    return golden[f"{tag}.{b}.dets"], golden[f"{tag}.{b}.landms"]


def test_fixture_is_small_and_holds_no_weights(golden):
    assert os.path.getsize(os.path.join(GOLDEN, "g25_retinaface.npz")) < 750_000
    assert not any("weight" in k or "running" in k for k in golden.files if k != "keys.default")


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_reference_outputs_lie_within_the_bound_of_the_model(tag, golden):
    c = RM.case(tag)
    bs, H, W, _ = RM.CASES[tag]
    assert np.array_equal(golden[f"{tag}.img"], c["img"])                                      # the same seeded input as when the fixture was made
    for name in ("loc", "conf", "landms"):
        ref, want = golden[f"{tag}.{name}"], c[name + "64"]
        err = RM.max_err(ref, want)
        print(f"{tag}.{name}: the reference against the model {err:.3e} = {err / c['e32_' + name]:.2f} e32, bar {c['bar_' + name]:.3e}")
        assert ref.dtype == np.float32 and ref.shape == want.shape and err <= c["bar_" + name]
    assert c["e32_loc"] <= 1e-4 * c["loc64"].std()                                            # the case is well conditioned
    for b in range(bs):
        want = c["det"][b]
        dist = RM.detect_distance(_stored_detect(golden, tag, b), (want["dets"], want["landms"]), c["bar_xy"], c["bar_conf"])
        print(f"{tag}.{b}: {len(want['dets'])} detections of {len(want['cand'])} candidates, the reference {dist:.2f} bars from the model")
        assert dist <= 1.0
        assert np.all(np.diff(golden[f"{tag}.{b}.dets"][:, 4]) < 0)                            # score descending


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_cases_meet_the_admission_conditions(tag):
    c = RM.case(tag)
    bs, H, W, _ = RM.CASES[tag]
    sizes = {"A": [(8, 8), (4, 4), (2, 2)], "B": [(9, 13), (5, 7), (3, 4)], "C": [(7, 12), (4, 6), (2, 3)], "D": [(5, 5), (3, 3), (2, 2)],
             "E": [(13, 5), (7, 3), (4, 2)]}[tag]
    assert RM.level_sizes(H, W) == sizes and c["N"] == 2 * sum(h * w for h, w in sizes)
    for b in range(bs):
        assert RM.admission(c["loc64"][b], c["conf64"][b], c["landms64"][b], H, W) == []
        d = c["det"][b]
        assert 0.05 * c["N"] <= len(d["cand"]) <= 0.4 * c["N"] and 3 <= len(d["keep"]) <= 0.8 * len(d["cand"])


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_restated_priors_equal_the_reference_bit_for_bit(tag, golden):
    _, H, W, _ = RM.CASES[tag]
    pr = RM.priors(H, W)
    assert pr.dtype == np.float32 and np.array_equal(pr, golden[f"{tag}.priors"])
    # a correctly rounded float32 division of the exact float32 numerator gives the same values: what the kernel computes
    sizes = RM.level_sizes(H, W)
    rows = []
    for (h, w), step, ms in zip(sizes, RM.STEPS, RM.MIN_SIZES):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        cx = (xx + np.float32(0.5)) * np.float32(step) / np.float32(W)
        cy = (yy + np.float32(0.5)) * np.float32(step) / np.float32(H)
        rows.append(np.stack([np.stack([cx, cy, np.full_like(cx, np.float32(m) / np.float32(W)), np.full_like(cx, np.float32(m) / np.float32(H))], -1)
                              for m in ms], 2).reshape(-1, 4))
    assert np.array_equal(np.concatenate(rows), pr)


def test_restated_nms_equals_the_stored_keep_lists(golden):
    for name, (n, thresh) in RM.NMS_SETS.items():
        boxes, scores = RM.nms_box_set(name)
        assert np.array_equal(boxes, golden[name + ".boxes"]) and np.array_equal(scores, golden[name + ".scores"])
        assert np.all(np.diff(scores) < 0)
        keep = golden[name + ".keep"].tolist()
        assert RM.nms(boxes.astype(np.float64), thresh) == keep and RM.nms(boxes, np.float32(thresh)) == keep
        assert 0.2 * len(boxes) <= len(keep) < len(boxes)
        if name != "nms.tie":
            b64 = boxes.astype(np.float64)
            assert min(np.abs(RM.iou_row(b64[i], b64[i + 1:]) - thresh).min() for i in range(len(b64) - 1)) >= 1e-4


def test_every_mutant_is_caught(golden):
    for m, tag in RM.NET_MUTANTS.items():
        c = RM.case(tag)
        x = RM.to_input(c["img"], mutant=m) if m == "mean_rgb" else c["x"]
        got = [t.numpy() for t in RM.network(c["sd"], x, mutant=None if m == "mean_rgb" else m)]
        bars = max(RM.max_err(g, golden[f"{tag}.{n}"]) / c["bar_" + n] for g, n in zip(got, ("loc", "conf", "landms")))
        print(f"mutant {m} on {tag}: {bars:.0f} bars from the fixture")
        assert bars >= RM.MUTANT_MARGIN, m
    for m, tag in RM.DETECT_MUTANTS.items():
        c = RM.case(tag)
        d = RM.detect(c["loc64"][0], c["conf64"][0], c["landms64"][0], c["H"], c["W"], mutant=m)
        bars = RM.detect_distance((d["dets"], d["landms"]), _stored_detect(golden, tag, 0), c["bar_xy"], c["bar_conf"])
        print(f"mutant {m} on {tag}: {bars:.0f} bars from the fixture")
        assert bars >= RM.MUTANT_MARGIN, m
    # the NMS mutants change a stored keep list
    b0, _ = RM.nms_box_set("nms.1")
    assert RM.nms(b0.astype(np.float64), RM.NMS_T, "iou_no_plus1") != golden["nms.1.keep"].tolist()
    bt, _ = RM.nms_box_set("nms.tie")
    assert RM.nms(bt.astype(np.float64), 0.5, "ovr_lt") != golden["nms.tie.keep"].tolist()
    assert RM.nms(bt.astype(np.float64), 0.5) == golden["nms.tie.keep"].tolist() == [0, 1, 2, 3, 4]


def test_mirror_has_the_reference_keys_in_order(golden):
    from e4s2024_amd import ops, seeded
    lines = str(golden["keys.default"]).split("\n")
    want = [(ln.split("|")[0], tuple(int(d) for d in ln.split("|")[1].split("x") if d)) for ln in lines]
    sd = ops.RetinaFace().state_dict()
    assert len(want) == 456 and [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert list(ops.retinaface_state_dict_shapes().items()) == want
    assert sd["body.bn1.num_batches_tracked"].dtype == torch.long
    assert not any(k.startswith(("body.fc", "body.avgpool")) for k, _ in want)
    assert "seeded_retinaface_state_dict" in seeded.__all__
    seeded_sd = seeded.seeded_retinaface_state_dict(3)
    assert list(seeded_sd) == [k for k, _ in want]
    ops.RetinaFace().load_state_dict(seeded_sd, strict=True)
    small = ops.RetinaFace(dict(ops.RETINAFACE_CFG_RE50, out_channel=64))
    small.load_state_dict(seeded.seeded_retinaface_state_dict(3, 64), strict=True)
    assert small.fpn.output1[2].negative_slope == 0.1 and ops.RetinaFace().fpn.output1[2].negative_slope == 0
    # the seeded statistics keep every channel and every residual branch alive, and are away from the identity
    gam = torch.cat([v for k, v in seeded_sd.items() if k.endswith("bn3.weight")])
    assert float(gam.abs().min()) >= 0.25 and 0.4 <= float(gam.lt(0).float().mean()) <= 0.6
    assert all(float(v.min()) >= 0.5 for k, v in seeded_sd.items() if k.endswith("running_var"))
    assert all(float(v.abs().max()) > 0.05 for k, v in seeded_sd.items() if k.endswith(("running_mean", ".bias")))


def test_constructor_errors():
    from e4s2024_amd import ops
    with pytest.raises(ValueError, match="mobilenet0.25"):
        ops.RetinaFace(dict(ops.RETINAFACE_CFG_RE50, name="mobilenet0.25"))
    with pytest.raises(ValueError, match="'train'"):
        ops.RetinaFace(None, "train")
    with pytest.raises(ValueError, match="out_channel"):
        ops.RetinaFace(dict(ops.RETINAFACE_CFG_RE50, out_channel=30))


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_mirror_on_the_cpu_against_the_model_and_the_fixture(tag, golden):
    c = RM.case(tag)
    net = RM.make_module(tag)
    net.load_state_dict(c["sd"], strict=True)
    got = [t.numpy() for t in net(T(c["x"]))]
    for g, n in zip(got, ("loc", "conf", "landms")):
        assert g.shape == c[n + "64"].shape and RM.max_err(g, c[n + "64"]) <= c["bar_" + n]
        assert RM.max_err(g, golden[f"{tag}.{n}"]) <= c["bar_" + n]
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(c["x"]))


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_retinaface, pipeline
    for name in ("RetinaFace", "PreparedRetinaFace", "retinaface_state_dict_shapes", "retinaface_weight_tensors", "retinaface_forward", "retinaface_detect",
                 "retinaface_detect_padded", "retinaface_priors", "retinaface_detection_tail"):
        assert name in ops_retinaface.__all__ and getattr(ops, name) is getattr(ops_retinaface, name)
    assert ops_retinaface.ARITH == "sb3" and ops.RETINAFACE_MAX_SIDE == 1500
    assert callable(pipeline.gpen_detect_faces)
    assert e4s2024_amd.GPEN_DETECT_OVERRIDES == {
        "swap_face_fine.gpen.face_detect.facemodels.retinaface": "swap_face_fine/gpen/face_detect/facemodels/retinaface.py",
        "swap_face_fine.gpen.face_detect.retinaface_detection": "swap_face_fine/gpen/face_detect/retinaface_detection.py"}
    assert set(e4s2024_amd.GPEN_DETECT_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert "GPEN_DETECT_OVERRIDES" in e4s2024_amd.install.__doc__
    assert all(os.path.exists(os.path.join(e4s2024_amd.DROPIN_DIR, rel)) for rel in e4s2024_amd.GPEN_DETECT_OVERRIDES.values())


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert [len(_lib._PROTOS[n]) for n in sorted(ENTRY_POINTS)] == [10, 8, 13, 7, 15, 4, 9]


def test_dropins_resolve_and_import_without_cv2_and_torchvision(tmp_path):
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    from e4s2024_amd import ops
    install_dropin()
    from swap_face_fine.gpen.face_detect.facemodels import retinaface
    from swap_face_fine.gpen.face_detect import retinaface_detection
    assert retinaface.__file__.startswith(e4s2024_amd.DROPIN_DIR) and retinaface_detection.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    assert "cv2" not in sys.modules and "torchvision" not in sys.modules
    assert "swap_face_fine.gpen.face_detect.facemodels.net" not in sys.modules
    c = RM.case("D")
    net = retinaface.RetinaFace(cfg=dict(retinaface_detection.cfg_re50, out_channel=64), phase="test")
    assert isinstance(net, ops.RetinaFace) and list(net.state_dict()) == list(c["sd"])
    net.load_state_dict(c["sd"], strict=True)
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(c["x"]))
    with pytest.raises(RuntimeError, match="CUDA"):                                           # eval: the native forward, which refuses a CPU tensor
        net.eval()(T(c["x"]))
    with pytest.raises(ValueError, match="'train'"):
        retinaface.RetinaFace(cfg=retinaface_detection.cfg_re50)                              # the reference's default phase is not implemented
    # the detector class with the reference's constructor: base_dir/weights/<network>.pth, a 'module.' prefix stripped
    from e4s2024_amd import seeded
    os.makedirs(tmp_path / "weights")
    torch.save({"module." + k: v for k, v in seeded.seeded_retinaface_state_dict(1).items()}, tmp_path / "weights" / "RetinaFace-R50.pth")
    det = retinaface_detection.RetinaFaceDetection(str(tmp_path), device="cpu")
    assert isinstance(det.net, ops.RetinaFace) and not det.net.training and det.net._loaded
    with pytest.raises(NotImplementedError, match="detect_tensor"):
        det.detect_tensor(T(c["x"]))
    with pytest.raises(ValueError, match="resize"):
        det.detect(c["img"][0], resize=2)
    with pytest.raises(TypeError, match="uint8"):                                             # a float frame is refused, not quantised
        det.detect(c["img"][0].astype(np.float32) + 0.25)
    with pytest.raises(RuntimeError, match="CUDA"):
        det.detect(c["img"][0])
    with pytest.raises(ValueError, match="1500"):
        det.detect(np.zeros((8, 1501, 3), dtype=np.uint8))


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops, pipeline
    c = RM.case("D")
    net = RM.make_module("D")
    x, img = T(c["x"]), T(c["img"])
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.retinaface_forward(x, net)
    net.load_state_dict(c["sd"], strict=True)
    for call in (lambda: ops.retinaface_forward(x, net), lambda: ops.retinaface_detect(img, net), lambda: pipeline.gpen_detect_faces(net, img),
                 lambda: ops.retinaface_forward(x, c["sd"])):
        with pytest.raises(RuntimeError, match="CUDA"):                                       # a CPU tensor
            call()
    with pytest.raises(ValueError, match="float32"):
        ops.retinaface_forward(x.double(), net)
    with pytest.raises(ValueError, match="uint8"):
        ops.retinaface_detect(x, net)
    with pytest.raises(ValueError, match="three colour"):
        ops.retinaface_forward(x[:, :2], net)
    with pytest.raises(ValueError, match="limited to 1500"):
        ops.retinaface_detect(torch.zeros((1, 1501, 8, 3), dtype=torch.uint8), net)
    with pytest.raises(ValueError, match="limited to 1500"):
        ops.retinaface_forward(torch.zeros((1, 3, 8, 1501)), net)
    with pytest.raises(ValueError, match="top_k"):
        ops.retinaface_detect_padded(img, net, top_k=0)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.retinaface_forward(x, net.train())
    with pytest.raises(KeyError, match="fpn.output1.0.weight"):
        ops.retinaface_forward(x, {"conv.weight": x})
    sd = dict(c["sd"])
    del sd["body.layer2.0.downsample.1.running_var"]
    with pytest.raises(KeyError, match="running_var"):
        ops.retinaface_forward(x, sd)
