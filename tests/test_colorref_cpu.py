"""Row f8 (Blender recolouring, stage 1) without a GPU: the float64 restatement ``colorref_model`` against the reference's own ``get_color_refer`` and
``Referencer.forward`` (``g20_color_refer.npz``), the per-sample rule, the package's names and argument errors that must raise before any launch.

The bound of the model against the fixture is four times ``ref_err``, the reference's float32 output against the float64 model measured when the fixture
was made (5.2e-7 .. 2.5e-6 over the cases), with a floor of 2e-7 (three float32 ulps at 1.0): a model that restates the reference cannot be further from it
than float32 arithmetic puts the reference from the exact value; four covers a different summation order.  Outputs of one-pixel parts are left out, as in
``ref_err`` (``colorref_model.one_pixel_outputs``: the reference divides 0 by 0 there)."""
import numpy as np
import pytest
import torch

import colorref_model as RM
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
OVERRIDES_BEFORE = {"models.networks", "models.stylegan2.model", "models.stylegan2.op", "models.stylegan2.op.fused_act", "models.stylegan2.op.upfirdn2d",
                    "models.stylegan2.op.conv2d_gradfix", "models.encoders.psp_encoders", "swap_face_fine.face_parsing.model",
                    "swap_face_fine.face_parsing.resnet", "swap_face_fine.face_parsing.face_parsing_demo"}


def _keys(present_row):
    return [n for i, n in enumerate(RM.PARTS) if present_row[i]]


@pytest.mark.parametrize("tag", [t for t in RM.FIXTURE_REFER_CASES if t not in ("forward", "two_class")])
def test_model_against_the_reference_get_color_refer(tag):
    g = load_golden("g20_color_refer")
    img_t, fa, ft, pa, pt, tau = RM.reference_inputs(tag)
    assert RM.crc(img_t, fa, ft, pa, pt) == int(g[tag.split(".tau")[0] + ".crc"]), "the seeded inputs are not the ones the fixture was made from"
    refs, present, inv, inv_target = RM.reference_outputs(tag)
    assert _keys(present[0]) == str(g[f"{tag}.keys"]).split(",")
    ru, iu = RM.one_pixel_outputs(pa, pt, *fa.shape[-2:])
    ru, iu = np.broadcast_to(ru, refs[0].shape), np.broadcast_to(iu, inv[0].shape)
    assert bool(ru.any()) == tag.startswith("hand") and not g[f"{tag}.refs"][ru].any() and not g[f"{tag}.inv"][iu].any()
    err = RM.max_err((np.where(ru, 0, refs[0]), np.where(iu, 0, inv[0]), inv_target[0]),
                     (np.where(ru, 0, g[f"{tag}.refs"]), np.where(iu, 0, g[f"{tag}.inv"]), g[f"{tag}.inv_target"]))
    ref_err = float(g[f"{tag}.ref_err"])
    print(f"{tag}: model against the reference {err:.3e}, ref_err {ref_err:.3e}, bound {RM.bound(ref_err):.3e}")
    assert err <= RM.bound(ref_err)


def test_hand_case_holds_what_it_is_for():
    """Absent in A only, absent in T only, one pixel, 63 / 64 / 65 / 130 pixels, and a part whose keys are all zero keys: the plain mean of their RGB."""
    img_t, fa, ft, pa, pt = RM.case_hand()
    na, nt = pa[0].reshape(9, -1).sum(1) // 16, pt[0].reshape(9, -1).sum(1) // 16
    assert na.tolist() == [130, 63, 64, 65, 1, 0, 20, 20, 40] and nt.tolist() == [130, 64, 65, 63, 3, 10, 0, 1, 60]
    refs, present, _, _ = RM.reference_outputs("hand.tau12")
    assert _keys(present[0]) == list(RM.HAND_PRESENT)
    rgb = RM.nearest_pick(RM.denorm(img_t[0]), 12, 20).reshape(3, -1).double().numpy()
    hair = refs[0, 1].reshape(3, -1)
    assert np.allclose(hair[:, :63], rgb[:, 100:164].mean(1, keepdims=True), rtol=0, atol=1e-14) and not hair[:, 63:].any()


@pytest.mark.parametrize("tag,maker", [("forward", RM.case_forward), ("two_class", RM.case_two_class)])
def test_model_against_the_reference_forward(tag, maker):
    g = load_golden("g20_color_refer")
    c = maker()
    assert RM.crc(*c[:6]) == int(g[f"{tag}.crc"]), "the seeded inputs are not the ones the fixture was made from"
    pack, (inv, inv_target), present = RM.packages(*c)
    assert _keys(present[0]) == str(g[f"{tag}.keys"]).split(",")
    assert np.array_equal(pack[0, 6:].astype(np.float32), g[f"{tag}.packages"][6:])            # masks, grey, background: exact
    err = RM.max_err((pack[0, :6], inv[0], inv_target[0], inv[0], inv_target[0]),
                     (g[f"{tag}.packages"][:6], g[f"{tag}.inv"], g[f"{tag}.inv_target"], g[f"{tag}.inv_cro"], g[f"{tag}.inv_target_cro"]))
    ref_err = float(g[f"{tag}.ref_err"])
    print(f"{tag}: model against the reference {err:.3e}, ref_err {ref_err:.3e}, bound {RM.bound(ref_err):.3e}")
    assert err <= RM.bound(ref_err)
    if tag == "two_class":                                                                     # two parts are enough: the zero rule sits below two
        assert _keys(present[0]) == ["skin", "inpainting"] and np.abs(pack[0, :6]).max() > 0.1


def test_fewer_than_two_parts_give_zero_references():
    img_a, img_t, la, lt, fa, ft, tau = RM.case_two_class()
    la = la.copy()
    la[:] = 1                                                                                  # head_A everywhere: no inpainting pixels in A
    pack, _, present = RM.packages(img_a, img_t, la, lt, fa, ft, tau)
    assert _keys(present[0]) == ["skin"] and not pack[0, :6].any() and pack[0, 6].all()


def test_model_processes_every_sample_on_its_own():
    img_a, img_t, la, lt, fa, ft, tau = RM.case_batch3()
    pa, pt, _, _, _ = RM.part_masks(la[:, ::4, ::4], lt[:, ::4, ::4])                           # 64 x 64 maps: the rule, not the size, is what is checked
    img = img_t[:, :, ::4, ::4]
    whole = RM.color_reference(img, fa, ft, pa, pt, tau)
    for b in range(3):
        one = RM.color_reference(img[b:b + 1], fa[b:b + 1], ft[b:b + 1], pa[b:b + 1], pt[b:b + 1], tau)
        assert all(np.array_equal(w[b:b + 1], o) for w, o in zip(whole, one))


def test_batch3_case_lacks_one_part_per_sample():
    pa, pt, _, _, _ = RM.part_masks(*RM.case_batch3()[2:4])
    na = RM.nearest_pick(T(pa), 64, 64).flatten(2).sum(2).numpy()
    nt = RM.nearest_pick(T(pt), 64, 64).flatten(2).sum(2).numpy()
    got = (na > 0) & (nt > 0)
    for b, name in enumerate(RM.BATCH3_ABSENT):
        assert _keys(got[b]) == [n for n in RM.PARTS if n != name], (b, _keys(got[b]))


# ------------------------------------------------------------------------------------------------ the package
def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_recolor
    for name in ("blender_part_masks", "color_reference", "blender_packages", "BLENDER_PARTS", "BLENDER_PART_IDS"):
        assert name in ops_recolor.__all__ and getattr(ops, name) is getattr(ops_recolor, name)
    assert ops.BLENDER_PARTS == RM.PARTS and {k: tuple(v) for k, v in ops.BLENDER_PART_IDS.items()} == RM.NAME_TO_IDS
    assert e4s2024_amd.RECOLOR_OVERRIDES == {"swap_face_fine.Blender.model_center.semantic_tools": "swap_face_fine/Blender/model_center/semantic_tools.py"}
    assert set(e4s2024_amd.OVERRIDES) == OVERRIDES_BEFORE
    assert set(e4s2024_amd.RECOLOR_OVERRIDES) <= set(e4s2024_amd._redirected())


def test_entry_points_are_declared_and_bound():
    from e4s2024_amd import _lib
    want = {"e4s_colorref_scratch_bytes", "e4s_colorref_lists", "e4s_colorref_rows", "e4s_colorref_attend", "e4s_colorref_sum_parts", "e4s_colorref_package"}
    assert want <= set(_lib.declared_symbols()) and want <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in want)


def _dropin():
    from conftest import install_dropin
    install_dropin()
    import e4s2024_amd
    from swap_face_fine.Blender.model_center import semantic_tools as st
    assert st.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    return st


def test_dropin_exports_the_reference_names():
    st = _dropin()
    for name in ("get_color_refer", "get_part_dict", "get_greyscale_head", "get_dilated_mask", "name_to_ids", "chunk_cosine_similarity"):
        assert hasattr(st, name)
    assert {k: tuple(v) for k, v in st.name_to_ids.items()} == RM.NAME_TO_IDS and list(st.name_to_ids) == list(RM.PARTS[:-1])
    lab = T(RM.blocky_labels(3, 2, 16, 16, 4))
    d = st.get_part_dict(lab)
    pa, _, head, _, _ = RM.part_masks(lab.numpy(), lab.numpy())
    assert list(d) == list(RM.PARTS[:-1]) + ["head"] and all(v.dtype == torch.int64 for v in d.values())
    assert all(np.array_equal(d[n].numpy(), pa[:, i]) for i, n in enumerate(RM.PARTS[:-1])) and np.array_equal(d["head"].numpy(), head[:, 0])
    img = T(RM.image(4, 2, 16, 16))
    a01 = torch.stack([RM.denorm(i) for i in img])
    grey = (a01[:, 0] * 0.299 + a01[:, 1] * 0.587 + a01[:, 2] * 0.114).clamp(0, 1) * d["head"]
    assert torch.equal(st.get_greyscale_head(img, d["head"]), grey)


def _good():
    """CPU tensors of valid shapes and dtypes: img_a, img_t, labels_a, labels_t, feats_a, feats_t, parts_a, parts_t."""
    lab = T(RM.blocky_labels(1, 2, 32, 32, 8))
    pa, pt, _, _, _ = RM.part_masks(lab.numpy(), lab.flip(-1).numpy())
    return (T(RM.image(1, 2, 32, 32)), T(RM.image(2, 2, 32, 32)), lab, lab.flip(-1).contiguous(), T(RM.features(3, 2, 8, 8)), T(RM.features(4, 2, 8, 8)),
            T(pa), T(pt))


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops
    img_a, img_t, la, lt, fa, ft, pa, pt = _good()
    # CPU tensors are refused once everything else is in order
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_part_masks(la, lt)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.color_reference(img_t, fa, ft, pa, pt, 7.0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_packages(img_a, img_t, la, lt, fa, ft, 7.0)
    with pytest.raises(RuntimeError, match="tau must be a CUDA tensor"):
        ops.color_reference(img_t, fa, ft, pa, pt, torch.tensor(7.0))
    # types
    with pytest.raises(TypeError):
        ops.blender_part_masks(la.numpy(), lt)
    with pytest.raises(TypeError):
        ops.color_reference(img_t, fa, ft, pa, pt, "7")
    with pytest.raises(TypeError):
        ops.color_reference(img_t, fa.numpy(), ft, pa, pt, 7.0)
    with pytest.raises(TypeError):
        ops.blender_packages(img_a, img_t, la, lt, fa, None, 7.0)
    # dtypes
    with pytest.raises(ValueError, match="uint8"):
        ops.blender_part_masks(la.long(), lt)
    with pytest.raises(ValueError, match="float32"):
        ops.color_reference(img_t.double(), fa, ft, pa, pt, 7.0)
    with pytest.raises(ValueError, match="float32"):
        ops.color_reference(img_t, fa.half(), ft, pa, pt, 7.0)
    with pytest.raises(ValueError, match="uint8"):
        ops.color_reference(img_t, fa, ft, pa.float(), pt, 7.0)
    with pytest.raises(ValueError, match="one float32 element"):
        ops.color_reference(img_t, fa, ft, pa, pt, torch.tensor([7.0, 8.0]))
    with pytest.raises(ValueError, match="uint8"):
        ops.blender_packages(img_a, img_t, la.int(), lt, fa, ft, 7.0)
    # shapes
    with pytest.raises(ValueError, match="differ in shape"):
        ops.blender_part_masks(la, lt[:, :16])
    with pytest.raises(ValueError):
        ops.blender_part_masks(la[0], lt[0])
    with pytest.raises(ValueError, match="must agree"):
        ops.color_reference(img_t, fa, ft[:, :, :4], pa, pt, 7.0)
    with pytest.raises(ValueError, match="part masks"):
        ops.color_reference(img_t, fa, ft, pa[:, :8], pt, 7.0)
    with pytest.raises(ValueError, match="part masks"):
        ops.color_reference(img_t, fa, ft, pa, pt[:, :, :16], 7.0)
    with pytest.raises(ValueError):
        ops.color_reference(img_t[:, :2], fa, ft, pa, pt, 7.0)
    with pytest.raises(ValueError):
        ops.blender_packages(img_a[:1], img_t, la, lt, fa, ft, 7.0)
    # D != 256, h * w > 4096
    with pytest.raises(ValueError, match="128 feature channels"):
        ops.color_reference(img_t, fa[:, :128], ft[:, :128], pa, pt, 7.0)
    with pytest.raises(ValueError, match="128 feature channels"):
        ops.blender_packages(img_a, img_t, la, lt, fa[:, :128], ft[:, :128], 7.0)
    big = torch.zeros(2, 256, 64, 65)
    with pytest.raises(ValueError, match=r"h \* w must be in 1..4096"):
        ops.color_reference(img_t, big, big, pa, pt, 7.0)
    with pytest.raises(ValueError, match=r"h \* w must be in 1..4096"):
        ops.blender_packages(img_a, img_t, la, lt, big, big, 7.0)
    # the dilation radius: int(W * 0.1 / 2) = 17 at W = 340
    wide = torch.zeros(1, 8, 340, dtype=torch.uint8)
    with pytest.raises(ValueError, match="radius of 17"):
        ops.blender_part_masks(wide, wide)


def test_dropin_argument_errors_before_any_launch():
    st = _dropin()
    _, img_t, la, lt, fa, ft, pa, pt = _good()
    da, dt = RM.part_dicts(pa, pt)
    with pytest.raises(NotImplementedError, match="light=True"):
        st.get_color_refer(img_t, fa, ft, da, dt, torch.tensor(1.0), True, True)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        st.get_color_refer(img_t, fa, ft, da, dt, torch.tensor(1.0))
    with pytest.raises(KeyError, match="inpainting"):
        st.get_color_refer(img_t, fa, ft, {k: v for k, v in da.items() if k != "inpainting"}, dt, torch.tensor(1.0))
    with pytest.raises(ValueError, match="128 feature channels"):
        st.get_color_refer(img_t, fa[:, :128], ft[:, :128], da, dt, 1.0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        st.get_dilated_mask(da["head"])
