"""Row f11 (the Real-ESRGAN step and ct_mode 'blender') without a GPU: the mirror module's keys, the float64 restatement ``rrdb_model`` against the mirror on
stock PyTorch, the bar of the GPU tests pinned from the other side by single-change mutants, the conditioning of the seeded cases, the drop-in, the rules
of ``swap_images`` and the argument errors that must raise before any launch.

basicsr is not installed and its architecture file is not part of the reference tree, so this row has no reference-made fixture: ``rrdb_model`` is the pin.
The bound of a case is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64.  Every mutant of the model moves the float64
output by at least ten bounds on some case, so a kernel inside the bound has none of these mistakes."""
import numpy as np
import pytest
import torch

import rrdb_model as RM

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_esr_input", "e4s_esr_scale_add", "e4s_esr_up2", "e4s_esr_tail"}


def test_mirror_has_the_keys_of_the_checkpoint():
    from e4s2024_amd import ops
    for nb, n in ((23, 702), (2, 72)):
        sd = ops.RRDBNet(nb).state_dict()
        assert len(sd) == n and list(ops.rrdbnet_state_dict_shapes(nb).items()) == [(k, tuple(v.shape)) for k, v in sd.items()]
    sd = ops.RRDBNet().state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    want = {"conv_first": (64, 3), "conv_body": (64, 64), "conv_up1": (64, 64), "conv_up2": (64, 64), "conv_hr": (64, 64), "conv_last": (3, 64)}
    for i in range(23):
        for r in (1, 2, 3):
            for k in range(1, 6):
                want[f"body.{i}.rdb{r}.conv{k}"] = (32 if k < 5 else 64, 64 + 32 * (k - 1))
    assert shapes == {f"{p}.{s}": ((co, ci, 3, 3) if s == "weight" else (co,)) for p, (co, ci) in want.items() for s in ("weight", "bias")}
    ops.RRDBNet(2).load_state_dict(RM.base_state_dict(2), strict=True)
    with pytest.raises(ValueError, match="num_block"):
        ops.RRDBNet(0)


@pytest.mark.parametrize("nb", [1, 2])
def test_mirror_is_the_gpen_sr_mirror_at_width_64_and_scale_4(nb):
    """Rows f11 and f16 run one network: the same keys and shapes in the same order, and one module's weights load into the other."""
    from e4s2024_amd import ops
    assert list(ops.rrdbnet_state_dict_shapes(nb).items()) == list(ops.gpen_sr_state_dict_shapes(nb, 64, 4).items())
    if nb == 1:
        ops.GpenSRNet(1, 64, 4).load_state_dict(ops.RRDBNet(1).state_dict(), strict=True)


def test_seeded_weights_depend_on_the_seed_alone():
    from e4s2024_amd import seeded
    assert "seeded_rrdbnet_state_dict" in seeded.__all__
    a, b = seeded.seeded_rrdbnet_state_dict(5, 1), seeded.seeded_rrdbnet_state_dict(5, 1)
    assert all(torch.equal(a[k], b[k]) for k in a) and len(a) == 2 * (15 + 6)
    assert not torch.equal(a["conv_hr.weight"], seeded.seeded_rrdbnet_state_dict(6, 1)["conv_hr.weight"])
    w = a["body.0.rdb2.conv3.weight"].double()
    assert abs(float(w.std()) * np.sqrt(128 * 9) - seeded.RRDB_GAIN) < 0.02 and float(a["conv_hr.bias"].abs().max()) <= 0.1


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_mirror_on_the_cpu_against_the_model(tag):
    from e4s2024_amd import ops
    c = RM.case(tag)
    net = ops.RRDBNet(RM.CASES[tag][0]).eval()
    net.load_state_dict(c["sd"], strict=True)
    with torch.no_grad():
        got = net(T(c["x"])).numpy()
    nb, h, w, bs = RM.CASES[tag]
    assert got.shape == (bs, 3, 4 * h, 4 * w) == c["want"].shape
    err = RM.max_err(got, c["want"])
    print(f"{tag}: the mirror in float32 against the model {err:.3e} = {err / c['e32']:.2f} e32, e32 {c['e32']:.3e}, max|want| {np.abs(c['want']).max():.2f}")
    assert err <= RM.bound(c["e32"], c["want"])
    assert c["e32"] <= 1e-4 * c["want"].std()                                                 # the case is well conditioned
    assert abs(c["want"].mean() - RM.OUT_MEAN) < 1e-3 and abs(c["want"].std() - RM.OUT_STD) < 1e-3


@pytest.mark.parametrize("tag", list(RM.IMAGE_CASES) + [RM.REAL_CASE[0]])
def test_image_cases_are_well_conditioned(tag):
    """What the GPU tests assert of every image case, on the model alone: the uint8 rule leaves at least 99 % of the pixels strict, fewer than 10 % are
    clamped, and the image spreads over more than 30 grey levels."""
    if tag == RM.REAL_CASE[0]:
        c = RM.real_case()
        u = np.concatenate([p.reshape(-1) for _, p in c["parts"]])
    else:
        c = RM.image_case(tag)
        u = c["u"]
    strict, clamped, std = RM.strict_pixels(u, c["e32"]).mean(), ((u <= 0) | (u >= 255)).mean(), RM.expected_u8(u).astype(np.float64).std()
    print(f"{tag}: e32 {c['e32']:.3e}, strict {100 * strict:.2f} %, clamped {100 * clamped:.2f} %, std {std:.1f} grey levels")
    assert strict >= 0.99 and clamped < 0.10 and std > 30


def test_every_mutant_is_ten_bounds_away_on_some_case():
    worst = {}
    for mutant in RM.MUTANTS:
        if mutant in ("align_corners_false", "uint8_rounds"):
            for tag in RM.IMAGE_CASES:
                c = RM.image_case(tag)
                b = RM.bound(c["e32"], c["want"])
                r = RM.image_network_output(c["sd"], c["img"], c["in_size"], c["out_size"], mutant=mutant)
                if mutant == "uint8_rounds":                                                  # a grey level is 1 / 255 of the network's output
                    moved = RM.max_err(RM.to_u8(r, mutant)[1], RM.expected_u8(c["u"])) / 255
                else:
                    moved = RM.max_err(r.numpy(), c["want"])
                worst[mutant] = max(worst.get(mutant, 0.0), moved / b)
        else:
            for tag in RM.CASES:
                c = RM.case(tag)
                moved = RM.max_err(RM.network(c["sd"], c["x"], mutant=mutant).numpy(), c["want"])
                worst[mutant] = max(worst.get(mutant, 0.0), moved / RM.bound(c["e32"], c["want"]))
        print(f"{mutant} lies {worst[mutant]:.0f} bounds from the model")
    assert set(worst) == set(RM.MUTANTS) and all(v >= RM.MUTANT_MARGIN for v in worst.values()), worst


def test_uint8_rule():
    """The rule at its edges, and on an image case of the seeded network: the expected image passes, one grey level off on a strict pixel does not."""
    u = np.array([-3.0, -1e-9, 0.5, 0.9999999, 1.0000001, 7.5, 254.9999999, 255.0000001, 255.5, 300.0])
    strict = RM.strict_pixels(u, 1e-6)
    assert strict.tolist() == [True, True, True, False, False, True, False, False, True, True]
    assert RM.expected_u8(u).tolist() == [0, 0, 0, 0, 1, 7, 254, 255, 255, 255]
    RM.check_u8(np.array([0, 0, 0, 1, 0, 7, 255, 254, 255, 255], dtype=np.uint8), u, 1e-6)
    with pytest.raises(AssertionError, match="strict"):
        RM.check_u8(np.array([0, 0, 0, 1, 0, 8, 255, 254, 255, 255], dtype=np.uint8), u, 1e-6)
    with pytest.raises(AssertionError, match="differs by"):
        RM.check_u8(np.array([0, 0, 0, 2, 0, 7, 255, 254, 255, 255], dtype=np.uint8), u, 1e-6)
    c = RM.image_case("img.40x36")
    want = RM.expected_u8(c["u"])
    RM.check_u8(want, c["u"], c["e32"])
    inner = np.argwhere(RM.strict_pixels(c["u"], c["e32"]) & (want > 0) & (want < 255))[0]
    off = want.copy()
    off[tuple(inner)] += 1
    with pytest.raises(AssertionError, match="1 strict pixels differ"):
        RM.check_u8(off, c["u"], c["e32"])


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_recolor, pipeline
    for name in ("RRDBNet", "PreparedRRDBNet", "rrdbnet_state_dict_shapes", "rrdbnet_weight_tensors", "realesr_forward", "realesr_input", "realesr_image"):
        assert name in ops_recolor.__all__ and getattr(ops, name) is getattr(ops_recolor, name)
    assert e4s2024_amd.ENHANCE_OVERRIDES == {"swap_face_fine.realesr.image_infer": "swap_face_fine/realesr/image_infer.py"}
    assert set(e4s2024_amd.ENHANCE_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert "ENHANCE_OVERRIDES" in e4s2024_amd.install.__doc__
    assert (pipeline.ESR_IN, pipeline.ESR_OUT) == (256, 1024) and ops.CT_MODES == ("lct", "mkl")
    for name in ("realesr_infer_batch", "realesr_infer_image", "color_transfer_blender"):
        assert callable(getattr(pipeline, name))
    # why realesr_infer_image leaves the reference's second resize out: at equal sizes align_corners=True picks single pixels
    x = torch.rand(1, 3, pipeline.ESR_OUT // 32, pipeline.ESR_OUT // 32)
    assert torch.equal(torch.nn.functional.interpolate(x, size=tuple(x.shape[2:]), mode="bilinear", align_corners=True), x)


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)


def test_dropin_resolves_and_imports_without_basicsr():
    import importlib.util
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    assert importlib.util.find_spec("basicsr") is None and "basicsr" not in sys.modules
    from swap_face_fine.realesr import image_infer
    assert image_infer.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    assert "basicsr" not in sys.modules and "cv2" not in sys.modules
    cls = image_infer.RealESRBatchInfer
    assert callable(cls.infer_batch) and callable(cls.infer_image)


def fake_reference_tree(root, monkeypatch):
    """``root/e4s/swap_face_fine`` as the first ``swap_face_fine`` on ``sys.path`` (what using the engine inside the reference tree looks like); returns where
    the reference's ``image_infer.py``, three directories below ``root``, looks for its checkpoint."""
    import importlib
    import sys
    pkg = root / "e4s" / "swap_face_fine"
    (pkg / "realesr").mkdir(parents=True)
    (pkg / "__init__.py").write_text("")
    monkeypatch.syspath_prepend(str(root / "e4s"))
    for name in [m for m in sys.modules if m == "swap_face_fine"]:
        monkeypatch.delitem(sys.modules, name)                                                # (put back when the test ends)
    importlib.invalidate_caches()
    return root / "ReliableSwap" / "pretrained" / "third_party" / "RealESRGAN" / "RealESRGAN_x4plus.pth"


def test_dropin_looks_for_the_checkpoint_where_the_reference_does(tmp_path, monkeypatch):
    import os
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    from swap_face_fine.realesr import image_infer
    # on its own the drop-in starts from its own package: <engine>/ReliableSwap/..., three directories above dropin/swap_face_fine/realesr
    alone = image_infer.checkpoint_path()
    assert alone == os.path.join(os.path.dirname(e4s2024_amd.DROPIN_DIR), image_infer.CHECKPOINT)
    # inside a reference tree: the reference's own expression, make_abs_path("../../../ReliableSwap/...") from <tree>/swap_face_fine/realesr/
    want = fake_reference_tree(tmp_path, monkeypatch)
    theirs = os.path.join(str(tmp_path / "e4s" / "swap_face_fine" / "realesr"), "../../../ReliableSwap/pretrained/third_party/RealESRGAN/RealESRGAN_x4plus.pth")
    assert image_infer.checkpoint_path() == os.path.normpath(theirs) == str(want)
    with pytest.raises(FileNotFoundError, match="RealESRGAN_x4plus.pth"):                      # the constructor goes there, and nowhere else
        image_infer.RealESRBatchInfer()
    want.parent.mkdir(parents=True)
    torch.save({"something": 1}, str(want))
    with pytest.raises(KeyError, match="params_ema"):
        image_infer.RealESRBatchInfer()


def test_invalidate_weight_caches_reaches_the_caches_of_netweights():
    """``netweights.prepare`` keeps a module's prepared weights beside the module, not on it; ``invalidate_weight_caches`` empties those of every module under
    its argument, once each, and leaves other modules' alone."""
    import weakref
    from e4s2024_amd import netweights, ops
    esr, other = ops.RRDBNet(1), ops.RRDBNet(1)
    holder = torch.nn.Sequential(torch.nn.Identity(), torch.nn.Sequential(esr))
    per_module = netweights._CACHES.setdefault(ops.PreparedRRDBNet, weakref.WeakKeyDictionary())
    caches = {}
    for m in (esr, other):
        caches[m] = per_module[m] = ops.PreparedRRDBNet()
        caches[m]._state = (("stale",), None, None, None, frozenset())
    assert netweights.caches_of(holder) == [caches[esr]] and netweights.caches_of(torch.nn.Identity()) == []
    assert ops.invalidate_weight_caches(holder) == 1
    assert caches[esr].key is None and caches[other].key == ("stale",)
    assert ops.invalidate_weight_caches(other) == 1 and caches[other].key is None


def test_swap_images_rules_for_the_blender_mode():
    from e4s2024_amd import ops, pipeline
    fr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    nets = (ops.BlenderNet(small_FPN=True).eval(), ops.RRDBNet(1).eval())
    with pytest.raises(ValueError, match=r"recolor_nets.*\['lct', 'mkl'\]"):
        pipeline.swap_images(None, None, None, fr, None, ct_mode="blender")
    with pytest.raises(ValueError, match=r"\['lct', 'mkl'\]"):
        pipeline.color_transfer(fr, fr, lab, lab, "blender")
    with pytest.raises(ValueError, match=r"\['lct', 'mkl'\]"):
        ops.skin_color_transfer(fr, fr, lab[:, None].float(), lab[:, None].float(), "blender")
    for mode in ("lct", "mkl", None, "rct"):
        with pytest.raises(TypeError, match="recolor_nets goes with ct_mode='blender'"):
            pipeline.swap_images(None, None, None, fr, None, ct_mode=mode, recolor_nets=nets)
    with pytest.raises(TypeError, match="recolor_nets and recolor_fn"):
        pipeline.swap_images(None, None, None, fr, None, recolor_fn=lambda s, c: s, recolor_nets=nets)
    with pytest.raises(TypeError, match="ct_mode and recolor_fn"):
        pipeline.swap_images(None, None, None, fr, None, recolor_fn=lambda s, c: s, ct_mode="blender", recolor_nets=nets)
    with pytest.raises(TypeError, match=r"pair \(blender, esr\)"):
        pipeline.swap_images(None, None, None, fr, None, ct_mode="blender", recolor_nets=nets[0])
    # a wrong pair fails before anything is launched (the frames here are CPU tensors and the other arguments None)
    with pytest.raises(TypeError, match="referencer.FPN"):
        pipeline.swap_images(None, None, None, fr, None, ct_mode="blender", recolor_nets=(nets[1], nets[1]))
    with pytest.raises(KeyError, match="conv_first.weight"):
        pipeline.swap_images(None, None, None, fr, None, ct_mode="blender", recolor_nets=(nets[0], nets[0]))
    with pytest.raises(RuntimeError, match="training mode"):
        pipeline.swap_images(None, None, None, fr, None, ct_mode="blender", recolor_nets=(ops.BlenderNet(small_FPN=True), nets[1]))
    with pytest.raises(TypeError, match="comp_indices is fixed"):
        pipeline.swap_images(None, None, None, fr, None, ct_mode="blender", recolor_nets=nets, comp_indices=(1,))


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops, pipeline
    net = ops.RRDBNet(1).eval()
    sd = RM.base_state_dict(1)
    net.load_state_dict(sd)
    good = torch.rand(2, 3, 5, 4)
    for weights in (net, sd, {"params_ema." + k: v for k, v in sd.items()}, {"params": sd}, {"params_ema": sd, "params": {}}):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):                       # CPU tensors are refused once everything else is in order
            ops.realesr_forward(good, weights)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.realesr_forward(good.transpose(2, 3), net)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.realesr_forward(torch.zeros(0, 3, 1, 1), net)
    with pytest.raises(TypeError):
        ops.realesr_forward(good.numpy(), net)
    with pytest.raises(TypeError):
        ops.realesr_forward(good, None)
    with pytest.raises(KeyError, match="conv_first.weight"):
        ops.realesr_forward(good, {"conv.weight": torch.zeros(1)})
    with pytest.raises(KeyError, match="body.0.rdb1.conv1.weight"):
        ops.realesr_forward(good, {"conv_first.weight": sd["conv_first.weight"]})
    with pytest.raises(KeyError, match="conv_hr.bias"):
        ops.realesr_forward(good, {k: v for k, v in sd.items() if k != "conv_hr.bias"})
    with pytest.raises(ValueError, match="body.0.rdb2.conv5.weight"):
        ops.realesr_forward(good, {**sd, "body.0.rdb2.conv5.weight": torch.zeros(64, 192, 1, 1)})
    with pytest.raises(ValueError, match="float32"):
        ops.realesr_forward(good, {**sd, "conv_up1.bias": sd["conv_up1.bias"].double()})
    with pytest.raises(ValueError, match="float32"):
        ops.realesr_forward(good.double(), net)
    with pytest.raises(ValueError, match="float32"):
        ops.realesr_forward(good[0], net)                                                     # rank
    with pytest.raises(ValueError, match=r"\[bs, 3, h, w\]"):
        ops.realesr_forward(torch.zeros(1, 4, 8, 8), net)
    with pytest.raises(ValueError, match="h, w >= 1"):
        ops.realesr_forward(torch.zeros(1, 3, 0, 8), net)
    with pytest.raises(ValueError, match="16384"):
        ops.realesr_forward(torch.zeros(1, 3, 1, 4097), net)
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.realesr_forward(good, ops.RRDBNet(1).to("meta"))
    # the wrappers
    img = torch.zeros(1, 6, 5, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        pipeline.realesr_infer_image(net, img)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        pipeline.realesr_infer_image(net, img, in_size=8, out_size=20)
    with pytest.raises(ValueError, match="uint8"):
        pipeline.realesr_infer_image(net, img.float())
    with pytest.raises(ValueError, match="uint8"):
        pipeline.realesr_infer_image(net, img[..., :2])
    with pytest.raises(ValueError, match="in_size"):
        pipeline.realesr_infer_image(net, img, in_size=0)
    with pytest.raises(ValueError, match="out_size"):
        pipeline.realesr_infer_image(net, img, out_size=2.5)
    with pytest.raises(KeyError, match="conv_first.weight"):
        pipeline.realesr_infer_image({}, img)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        pipeline.realesr_infer_batch(net, good)
    with pytest.raises(ValueError, match="float32"):
        pipeline.realesr_infer_batch(net, good.double())
    with pytest.raises(ValueError, match="out_hw"):
        pipeline.realesr_infer_batch(net, good, out_hw=(4, 4, 4))
    with pytest.raises(KeyError, match="conv_first.weight"):
        pipeline.realesr_infer_batch({}, good)
    # color_transfer_blender
    blender = ops.BlenderNet(small_FPN=True).eval()
    fr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        pipeline.color_transfer_blender(fr, fr, None, blender, net)
    with pytest.raises(ValueError, match="uint8"):
        pipeline.color_transfer_blender(fr.float(), fr, None, blender, net)
    with pytest.raises(ValueError, match="one shape"):
        pipeline.color_transfer_blender(fr, fr[:, :4], None, blender, net)
