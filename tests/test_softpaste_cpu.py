"""The two-image caller's paste-back (row f6) without a GPU: the CPU restatement ``softpaste_model`` against outputs of the reference's own
``SoftErosion`` / ``Trick`` / ``utils.morphology`` (``g18_soft_paste.npz``), the C ABI's new entry points, the image-mode style mix, and argument
errors that must raise before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import softpaste_model as SP
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
SE_INPUTS = ("face_96x80", "blocky_128", "resized_90x75")
SOFT_TOL = 1e-6          # the same float32 ATen arithmetic as the fixture's: only the library version differs


def _configs(g):
    return [(int(k), float(t), int(i)) for k, t, i in g["configs"]]


@pytest.mark.parametrize("name", SE_INPUTS)
@pytest.mark.parametrize("ci", [0, 1, 2])
def test_soft_erosion_restatement_reproduces_the_reference(name, ci):
    g = load_golden("g18_soft_paste")
    assert _configs(g) == [(15, 0.6, 1), (17, 0.9, 7), (5, 0.5, 2)]
    k, thr, it = _configs(g)[ci]
    soft, hard = SP.soft_erosion(g[f"se.{name}.x"].astype(np.float32), k, thr, it)
    assert np.array_equal(hard, g[f"se.{name}.c{ci}.hard"])
    d = np.abs(soft - g[f"se.{name}.c{ci}.soft"]).max()
    print(f"soft_erosion{(k, thr, it)} on {name}: max-abs {d:.3e}")
    assert d <= SOFT_TOL and not np.isnan(soft).any()


@pytest.mark.parametrize("radius", [2, 10])
def test_expansion_masks_restatement_reproduces_the_reference(radius):
    g = load_golden("g18_soft_paste")
    got = SP.soft_paste_masks(g["exp.labels"][None], g["exp.hole"][None], radius)
    for name, m in zip(("content", "border", "full"), got):
        d = np.abs(m - g[f"exp.r{radius}.{name}"]).max()
        print(f"expansion r{radius} {name}: max-abs {d:.3e}")
        assert m.shape == g[f"exp.r{radius}.{name}"].shape and d <= SOFT_TOL


def test_facial_mask_restatement_reproduces_the_reference():
    g = load_golden("g18_soft_paste")
    got = SP.facial_mask12(g["facial.labels"][None], tuple(int(v) for v in g["facial.size"]))
    assert got.shape == g["facial.out"].shape == (1, 1, 100, 90)
    assert np.abs(got - g["facial.out"]).max() <= SOFT_TOL


@pytest.mark.parametrize("ratio", [1.0, 0.75])
def test_blend_restatement_reproduces_the_reference(ratio):
    g = load_golden("g18_soft_paste")
    assert np.isnan(g["blend.mask"]).any()
    for ch in (1, 3):
        mask = np.repeat(g["blend.mask"][None, None], ch, axis=1)
        got = SP.blend_with_mask(g["blend.bottom"][None], g["blend.up"][None], mask, ratio)
        assert np.array_equal(got[0], g[f"blend.out_{int(ratio * 100)}"])
    if ratio == 1.0:          # the crop paste np.uint8(swapped * content + T * (1 - content)) of _past_back:216-217 is the same bits
        m = np.nan_to_num(g["blend.mask"], nan=0.0)[:, :, None]
        assert np.array_equal(np.uint8(g["blend.up"] * m + g["blend.bottom"] * (1 - m)), g["blend.out_100"])


def test_documented_departures_of_the_restatement():
    """All-pass plane -> ones; all-zero plane -> zeros, no NaN; each plane normalised by its own maximum."""
    x = np.zeros((1, 3, 12, 12), np.float32)
    x[0, 0] = 4.0                      # every convolution value >= 0.6, even in the corners
    x[0, 2, 3:9, 3:9] = 1.0
    soft, hard = SP.soft_erosion(x)
    assert hard[0, 0].all() and (soft[0, 0] == 1).all()
    assert not hard[0, 1].any() and (soft[0, 1] == 0).all()
    alone, _ = SP.soft_erosion(x[:, 2:3])
    assert np.array_equal(soft[0, 2], alone[0, 0]) and not np.isnan(soft).any()


# ------------------------------------------------------------------------------------------------ library and host logic
NEW_SYMBOLS = ("e4s_soft_erosion", "e4s_soft_erosion_scratch_bytes", "e4s_blend_u8")


def test_library_exports_the_soft_paste_entry_points():
    from e4s2024_amd import _lib
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/e4s_hip.h"
        assert name in _lib._PROTOS and hasattr(L.cdll, name), f"{name} is not exported by {L.path}"


def test_soft_paste_argument_errors_without_a_launch():
    from e4s2024_amd import ops
    from e4s2024_amd._lib import lib
    c = lib().cdll
    one = ctypes.c_void_p(16)          # non-null dummy pointers: validation fails before they are touched
    for k, it in ((14, 1), (35, 1), (1, 1), (15, 0)):
        assert c.e4s_soft_erosion(one, one, one, one, one, 1, 8, 8, k, 0.6, it, None) == -1, (k, it)
    assert b"kernel_size" in c.e4s_last_error() or b"iterations" in c.e4s_last_error()
    assert c.e4s_soft_erosion(one, one, one, one, one, -1, 8, 8, 15, 0.6, 1, None) == -1
    assert c.e4s_soft_erosion(one, None, one, None, one, 1, 8, 8, 15, 0.6, 1, None) == -1          # no weights
    assert c.e4s_soft_erosion(None, None, None, None, None, 0, 8, 8, 15, 0.6, 1, None) == 0        # no planes: nothing to do
    assert c.e4s_blend_u8(one, one, one, one, 1.0, 1, 8, 8, 2, None) == -1
    assert b"mask_channels" in c.e4s_last_error()
    assert c.e4s_blend_u8(one, one, one, one, 1.5, 1, 8, 8, 1, None) == -1
    assert c.e4s_blend_u8(one, one, one, None, 1.0, 1, 8, 8, 1, None) == -1
    nbytes = ctypes.c_int64(-1)
    assert c.e4s_soft_erosion_scratch_bytes(3, 512, 512, 1, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * 3 * 8 * 16
    assert c.e4s_soft_erosion_scratch_bytes(3, 512, 512, 7, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * (3 * 8 * 16 + 2 * 3 * 512 * 512)
    assert c.e4s_soft_erosion_scratch_bytes(3, 512, 512, 0, ctypes.byref(nbytes)) == -1
    # the Python layer: checks come before any launch, so they work on CPU tensors too
    x = torch.zeros(1, 1, 8, 8)
    for bad in (14, 35, 1, 15.0):
        with pytest.raises(ValueError, match="kernel_size"):
            ops.soft_erosion(x, kernel_size=bad)
    with pytest.raises(ValueError, match="iterations"):
        ops.soft_erosion(x, iterations=0)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.soft_erosion(x)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.soft_paste_masks(lab)
    with pytest.raises(ValueError, match="kernel_size"):
        ops.soft_paste_masks(lab, kernel_size=4)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.facial_mask12(lab)
    with pytest.raises(TypeError, match="unexpected"):
        ops.facial_mask12(lab, radius=3)
    fr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.blend_with_mask(fr, fr, torch.zeros(1, 1, 8, 8))
    for name in ("soft_erosion", "soft_paste_masks", "facial_mask12", "blend_with_mask"):
        assert name in ops.__dict__ and name in __import__("e4s2024_amd.ops_post", fromlist=["__all__"]).__all__


def test_image_mode_style_mix_and_component_sets():
    """``mix_style_vectors(..., ear_interpolation=False)`` == ``_swap_comp_style_vector`` (Face_swap_with_two_imgs.py:416-453); the default keeps the
    video caller's ear average."""
    from e4s2024_amd import pipeline
    assert pipeline.IMAGE_COMP_INDICES == SP.IMAGE_COMP_INDICES == (1, 2, 3, 5, 6, 7, 8, 9)
    assert pipeline.IMAGE_COMP_INDICES_CT == SP.IMAGE_COMP_INDICES_CT == (1, 2, 3, 5, 6, 9)
    rs = np.random.RandomState(3)
    t, s = T(rs.randn(3, 12, 32).astype(np.float32)), T(rs.randn(3, 12, 32).astype(np.float32))
    s[1, 9] = 0                        # a driven face without teeth
    for idx in (pipeline.IMAGE_COMP_INDICES, pipeline.IMAGE_COMP_INDICES_CT):
        for below in (False, True):
            got = pipeline.mix_style_vectors(t, s, idx, below, ear_interpolation=False)
            assert torch.equal(got, SP.mix_style_vectors_image(t, s, idx, below)), (idx, below)
    with_ears = pipeline.mix_style_vectors(t, s, pipeline.IMAGE_COMP_INDICES)
    assert torch.equal(with_ears[:, 7], (t[:, 7] + s[:, 7]) / 2) and torch.equal(with_ears, pipeline.mix_style_vectors(t, s, pipeline.IMAGE_COMP_INDICES, False, True))
    assert torch.equal(pipeline.mix_style_vectors(t, s, pipeline.IMAGE_COMP_INDICES, ear_interpolation=False)[:, 7], s[:, 7])
    assert torch.equal(pipeline.mix_style_vectors(t, s, pipeline.IMAGE_COMP_INDICES_CT, ear_interpolation=False)[:, 7], t[:, 7])
