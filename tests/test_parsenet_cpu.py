"""Row f13 (GPEN's ParseNet face mask) without a GPU: the reference's stored outputs against the float64 restatement ``parsenet_model``, the mirror module's
keys against the reference's, the mirror on stock PyTorch, the bars of the GPU tests pinned from the other side by single-change mutants, the uint8 table, the
strictness cap on the reference's own float32 output, the drop-in and the argument errors that must raise before any launch.

The bar of a case and output is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64 — never the code under test."""
import numpy as np
import pytest
import torch

import parsenet_model as PM
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_parsenet_stem", "e4s_parsenet_pad"}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g24_parsenet")


@pytest.mark.parametrize("tag", list(PM.CASES))
def test_reference_outputs_lie_within_the_bound_of_the_model(tag, golden):
    c = PM.case(tag)
    n = PM.STORED[tag]
    assert np.array_equal(golden[f"{tag}.img"], c["img"])                                      # the same seeded input as when the fixture was made
    ref_mask, ref_img = golden[f"{tag}.out_mask"], golden[f"{tag}.out_img"]
    assert ref_mask.dtype == np.float32 and ref_mask.shape == (n,) + c["mask64"].shape[1:] and ref_img.shape == (n,) + c["img64"].shape[1:]
    e_mask, e_img = PM.max_err(ref_mask, c["mask64"][:n]), PM.max_err(ref_img, c["img64"][:n])
    print(f"{tag}: the reference against the model {e_mask:.3e} = {e_mask / c['e32_mask']:.2f} e32 (logits), {e_img:.3e} = {e_img / c['e32_img']:.2f} e32 (image); "
          f"logits std {ref_mask.std():.2f}")
    assert e_mask <= PM.bound(c["e32_mask"], c["mask64"]) and e_img <= PM.bound(c["e32_img"], c["img64"])
    assert 1.0 <= ref_mask.std() <= 10.0                                                      # logits of order 1 to 10: the bars stay narrow
    assert c["e32_mask"] <= 1e-4 * c["mask64"].std()                                          # the case is well conditioned


def test_output_sizes_of_the_cases():
    want = {"A": (16, 16), "B": (64, 64), "C": (32, 32), "D": (48, 48), "E": (20, 12)}
    from e4s2024_amd import ops
    for tag, hw in want.items():
        assert PM.case(tag)["mask64"].shape[2:] == hw
        assert ops.parsenet_output_size(PM.make_module(tag).structure, *PM.CASES[tag][1][1:]) == hw
    assert ops.parsenet_output_size(PM.make_module("A").structure, 16, 4) is None             # 4 -> 2 -> 1: a map below 2 x 2


@pytest.mark.parametrize("tag", list(PM.CASES))
def test_strictness_cap_holds_for_the_reference(tag, golden):
    """The cap cannot hide a failure: at most 1 % of a case's pixels are non-strict, and the reference's own float32 labels and masks pass the rule."""
    c = PM.case(tag)
    n = PM.STORED[tag]
    part = {k: c[k][:n] for k in ("labels", "strict", "mask")}
    share = PM.check_labels(golden[f"{tag}.out_mask"].argmax(1), part)
    PM.check_mask(PM.mask_of(golden[f"{tag}.out_mask"].argmax(1)), part)
    full = 1.0 - float(c["strict"].mean())
    print(f"{tag}: non-strict share {full:.5f} (stored samples {share:.5f}), margin {2 * PM.bound(c['e32_mask'], c['mask64']):.2e}")
    assert full <= PM.NONSTRICT_CAP
    bad = c["labels"].copy()                                                                  # and the rule bites: one strict pixel off fails
    i = tuple(np.argwhere(c["strict"])[0])
    bad[i] = (bad[i] + 1) % PM.PARSING_CH
    with pytest.raises(AssertionError, match="strict pixels"):
        PM.check_labels(bad, c)


def test_every_mutant_is_a_hundred_bars_from_the_fixture_on_its_case(golden):
    assert set(PM.MUTANTS) >= {"zero_pad", "symmetric_pad", "bilinear_up", "stride_from_1", "stride_on_conv1", "shortcut_from_conv1", "slope_001",
                               "act_after_conv2", "bn_eps_1e3", "feat_dropped", "flip_dropped"}
    for m, tag in PM.MUTANTS.items():
        c = PM.case(tag)
        x = PM.img2tensor(c["img"], bgr=False) if m == "flip_dropped" else c["x"]
        got = PM.network(c["sd"], x, mutant=None if m == "flip_dropped" else m)[0].numpy()[:PM.STORED[tag]]
        bars = PM.max_err(got, golden[f"{tag}.out_mask"]) / PM.bound(c["e32_mask"], c["mask64"])
        print(f"mutant {m} on {tag}: {bars:.0f} bars from the fixture")
        assert bars >= PM.MUTANT_MARGIN, m
    # the two table mutants leave the logits alone and move the mask on strict pixels
    for m, tag in (("class14_255", "B"), ("class18_255", "D")):
        c = PM.case(tag)
        moved = (PM.mask_of(c["labels"], PM.table(m)) != c["mask"]) & c["strict"]
        print(f"mutant {m} on {tag}: {int(moved.sum())} strict pixels change")
        assert moved.sum() >= 100, m
        with pytest.raises(AssertionError, match="strict pixels"):
            PM.check_mask(PM.mask_of(c["labels"], PM.table(m)), c)


def test_mirror_has_the_reference_keys_in_order(golden):
    from e4s2024_amd import ops
    lines = str(golden["keys.default"]).split("\n")
    want = [(ln.split("|")[0], tuple(int(d) for d in ln.split("|")[1].split("x") if d)) for ln in lines]
    sd = ops.ParseNet().state_dict()
    assert len(want) == 238 and [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert list(ops.parsenet_state_dict_shapes().items()) == want
    assert list(ops.parsenet_structure_shapes(ops.ParseNet().structure).items()) == want      # what a mapping's keys are checked against
    assert sum(int(np.prod(s)) for k, s in want if not k.endswith("num_batches_tracked")) == 21319894                # 21.3 M parameters
    assert sum(k.endswith("conv2d.weight") for k, _ in want) == 47
    assert sd["body.0.conv1.norm.norm.num_batches_tracked"].dtype == torch.long
    for kwargs, why in ((dict(norm_type="in"), "'in'"), (dict(relu_type="prelu"), "'prelu'"), (dict(norm_type="none"), "'none'")):
        with pytest.raises(ValueError, match=why):
            ops.ParseNet(**kwargs)
    # a block that keeps its size and changes its width has a shortcut convolution too; a mapping's structure is read off its keys
    assert ops.parsenet_structure_shapes((8, (("body", "none", 8, 16),), 16, 19))["body.0.shortcut_func.conv2d.weight"] == (16, 8, 3, 3)


def test_structure_read_off_a_mapping():
    from e4s2024_amd import ops_parsenet
    for tag in ("A", "B", "C", "D"):
        net = PM.make_module(tag)
        assert ops_parsenet._structure_of_keys("t", net.state_dict()) == net.structure
        assert [tuple(t.shape) for t in ops_parsenet.parsenet_weight_tensors(PM.state_dict(tag))] == \
            [tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")]


def test_seeded_weights():
    from e4s2024_amd import seeded
    assert "seeded_parsenet_state_dict" in seeded.__all__
    with torch.device("meta"):
        template = PM.make_module("D").state_dict()
    a, b = seeded.seeded_parsenet_state_dict(template, 5), seeded.seeded_parsenet_state_dict(template, 5)
    assert list(a) == list(template) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["body.0.conv1.conv2d.weight"], seeded.seeded_parsenet_state_dict(template, 6)["body.0.conv1.conv2d.weight"])
    scales = [v for k, v in a.items() if k.endswith("norm.norm.weight")]
    assert all(int((v == 0).sum()) == 1 and float(v.abs().max()) <= 1.5 for v in scales)     # one exact zero per layer, within +-1.5
    neg = float(torch.cat(scales).lt(0).float().mean())
    assert 0.4 <= neg <= 0.6
    assert all(float(v.min()) >= 0.5 for k, v in a.items() if k.endswith("running_var"))
    assert all(float(v.abs().max()) > 0.05 for k, v in a.items() if k.endswith(("running_mean", ".bias")))
    assert all(v.dtype == torch.long for k, v in a.items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("tag", list(PM.CASES))
def test_mirror_on_the_cpu_against_the_model(tag):
    c = PM.case(tag)
    net = PM.make_module(tag)
    net.load_state_dict(c["sd"], strict=True)
    mask, img = net(T(c["x"]))
    assert PM.max_err(mask.numpy(), c["mask64"]) <= PM.bound(c["e32_mask"], c["mask64"])
    assert PM.max_err(img.numpy(), c["img64"]) <= PM.bound(c["e32_img"], c["img64"])
    PM.check_labels(mask.argmax(1).numpy(), c)
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(c["x"]))


def test_uint8_table_is_numpys_expression_on_all_levels():
    from e4s2024_amd import ops
    table = ops.img2tensor_table()
    levels = np.arange(256, dtype=np.uint8)
    assert table.dtype == np.float32 and table.shape == (256,)
    assert np.array_equal(table, (levels / 255. * 2 - 1).astype(np.float32))                   # float64, rounded once
    assert table[0] == -1 and table[255] == 1
    # FaceParse.img2tensor itself, through torch as the reference runs it, flip included
    img = levels.repeat(3).reshape(16, 16, 3).copy()
    img[..., 1] = img[::-1, :, 1]
    img[..., 2] = img[:, ::-1, 2]
    ref = torch.from_numpy((img[..., ::-1] / 255. * 2 - 1).transpose(2, 0, 1)).unsqueeze(0).float().numpy()
    assert np.array_equal(ref, table[img[None, ..., ::-1]].transpose(0, 3, 1, 2)) and np.array_equal(ref, PM.img2tensor(img[None]))
    # rounding each operation in float32 instead differs on some level: the table is not that
    f32 = (levels.astype(np.float32) / np.float32(255.) * np.float32(2) - np.float32(1))
    assert (f32 != table).any()
    assert ops.MASK_COLORMAP == PM.MASK_COLORMAP and len(ops.MASK_COLORMAP) == 19


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_parsenet, pipeline
    for name in ("ParseNet", "PreparedParseNet", "parsenet_state_dict_shapes", "parsenet_weight_tensors", "parsenet_forward", "parsenet_mask",
                 "parsenet_mask_from_tensor"):
        assert name in ops_parsenet.__all__ and getattr(ops, name) is getattr(ops_parsenet, name)
    assert callable(pipeline.gpen_face_mask)
    assert e4s2024_amd.GPEN_PARSE_OVERRIDES == {"swap_face_fine.gpen.face_parse.parse_model": "swap_face_fine/gpen/face_parse/parse_model.py"}
    assert set(e4s2024_amd.GPEN_PARSE_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert "GPEN_PARSE_OVERRIDES" in e4s2024_amd.install.__doc__
    assert len(e4s2024_amd.GPEN_OVERRIDES) == 1
    assert not any(m.endswith("face_parse.blocks") for m in e4s2024_amd._redirected())


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert [len(_lib._PROTOS[n]) for n in sorted(ENTRY_POINTS)] == [8, 12]
    assert "argmax + table" in src                                                             # the equal-size use of e4s_bilinear_argmax is stated


def test_dropin_resolves_and_imports_without_cv2():
    import sys
    from conftest import install_dropin
    import e4s2024_amd
    install_dropin()
    from swap_face_fine.gpen.face_parse import parse_model
    assert parse_model.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    assert "cv2" not in sys.modules and "swap_face_fine.gpen.face_parse.blocks" not in sys.modules
    from e4s2024_amd import ops
    cfg = PM.config("A")
    net = parse_model.ParseNet(cfg["in_size"], cfg["out_size"], cfg["min_feat_size"], cfg["base_ch"], 19, cfg["res_depth"], norm_type="bn",
                               relu_type="LeakyReLU", ch_range=list(cfg["ch_range"]))
    assert isinstance(net, ops.ParseNet) and list(net.state_dict()) == list(PM.case("A")["sd"])
    net.load_state_dict(PM.case("A")["sd"], strict=True)
    with pytest.raises(NotImplementedError, match="eval"):
        net.train()(T(PM.case("A")["x"]))
    with pytest.raises(RuntimeError, match="CUDA"):                                           # eval: the native forward, which refuses a CPU tensor
        net.eval()(T(PM.case("A")["x"]))
    with pytest.raises(ValueError, match="'prelu'"):
        parse_model.ParseNet()                                                                # the reference's default relu_type is not implemented
    p = parse_model.define_P(16, 16, 4)
    assert isinstance(p, parse_model.ParseNet) and not p.training and p.in_size == 16 and p.structure[0] == 64
    assert list(parse_model.define_P().state_dict()) == list(ops.ParseNet().state_dict())
    with pytest.raises(ValueError, match="'relu'"):
        parse_model.define_P(relu_type="relu")


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops, pipeline
    c = PM.case("A")
    net = PM.make_module("A")
    x, img = T(c["x"]), T(c["img"])
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.parsenet_forward(x, net)
    net.load_state_dict(c["sd"], strict=True)
    for call in (lambda: ops.parsenet_forward(x, net), lambda: ops.parsenet_mask(img, net), lambda: ops.parsenet_mask_from_tensor(x, net),
                 lambda: pipeline.gpen_face_mask(net, img), lambda: ops.parsenet_forward(x, c["sd"])):
        with pytest.raises(RuntimeError, match="CUDA"):                                       # a CPU tensor
            call()
    with pytest.raises(ValueError, match="float32"):
        ops.parsenet_forward(x.double(), net)
    with pytest.raises(ValueError, match="uint8"):
        ops.parsenet_mask(x, net)
    with pytest.raises(ValueError, match="in_size is 16"):
        ops.parsenet_mask(img[:, :8], net)
    with pytest.raises(ValueError, match="in_size is 16"):
        ops.parsenet_mask_from_tensor(x[:, :, :, :8], net)
    with pytest.raises(ValueError, match="2 x 2"):
        ops.parsenet_forward(x[:, :, :, :4], net)
    with pytest.raises(ValueError, match="three colour"):
        ops.parsenet_forward(x[:, :2], net)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.parsenet_forward(x, net.train())
    with pytest.raises(KeyError, match="encoder.0.conv2d.weight"):
        ops.parsenet_forward(x, {"conv.weight": x})
    sd = dict(c["sd"])
    del sd["body.1.conv2.norm.norm.running_var"]
    with pytest.raises(KeyError, match="running_var"):
        ops.parsenet_forward(x, sd)
    sd = dict(c["sd"])
    sd["decoder.0.shortcut_func.conv2d.bias"] = sd["decoder.0.shortcut_func.conv2d.bias"].double()
    with pytest.raises(ValueError, match="shortcut_func.conv2d.bias"):
        ops.parsenet_forward(x, sd)
    sd["decoder.0.shortcut_func.conv2d.bias"] = torch.zeros(3)
    with pytest.raises(ValueError, match="shortcut_func.conv2d.bias"):
        ops.parsenet_forward(x, sd)
