"""The image caller's skin colour transfer (row f7) without a GPU: the CPU restatement ``colortransfer_model`` against outputs of the reference's own
``utils.morphology`` and ``swap_face_fine.color_transfer`` (``g19_color_transfer.npz``), the C ABI's new entry points, and argument errors that must
raise before anything is launched.

The byte bound on the lct / mkl restatement is a condition on the fixture, not a tuned number: the reference takes its means (lct: and covariances) in
float32, the model in float64, so a value that lands within about 1e-5 grey levels of an integer may truncate to the neighbouring level.  No byte may
differ by more than one level and at most 1e-3 of them may differ at all (measured on these inputs: 1.8e-5 .. 1.4e-4)."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import colortransfer_model as CM
from conftest import load_golden
from oracle import e4s_oracle as O

MAX_SHARE = 1e-3
LAMBDA_MIN = 4e-3


def _crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


@pytest.mark.parametrize("shape,radii", CM.MORPH_SHAPES, ids=lambda v: "x".join(str(i) for i in v))
def test_flat_morphology_restatement_equals_the_reference(shape, radii):
    g = load_golden("g19_color_transfer")
    x = CM.morph_input(shape)
    tag = "x".join(str(v) for v in shape)
    assert _crc(x) == int(g[f"morph.{tag}.crc"]), "the seeded input is not the one the fixture was made from"
    assert (x == 0).any() and (x == 1).any() and ((x > 0) & (x < 1)).any()
    for r in radii:
        for name, fn, op in (("dilate", CM.grey_dilate, np.maximum), ("erode", CM.grey_erode, np.minimum)):
            got = fn(x, r)
            assert got.dtype == np.float32 and np.array_equal(got, g[f"morph.{tag}.r{r}.{name}"]), (tag, r, name)
            assert np.array_equal(got, O._flat_morph(x, r, op))              # the separable form is the oracle's (2r+1)^2 form
        if r == 0:
            assert np.array_equal(CM.grey_dilate(x, 0), x)


@pytest.mark.parametrize("pair", range(CM.CT_PAIRS))
@pytest.mark.parametrize("mode", CM.MODES)
def test_transfer_restatement_against_the_reference(pair, mode):
    g = load_golden("g19_color_transfer")
    d, t, md, mt = CM.ct_pair(pair)
    assert _crc(d, t, md, mt) == int(g[f"ct.p{pair}.crc"]), "the seeded pair is not the one the fixture was made from"
    assert g["ct.eigenvalues"].shape == (CM.CT_PAIRS, 2, 3) and g["ct.eigenvalues"].min() >= LAMBDA_MIN
    lam = np.linalg.eigvalsh(np.cov(CM.inner(d, md).reshape(-1, 3).astype(np.float64).T))
    assert np.allclose(lam, g["ct.eigenvalues"][pair, 0], rtol=1e-9)
    composed, q = CM.skin_color_transfer(d, t, md, mt, mode)
    ref = g[f"ct.p{pair}.{mode}.q"]
    diff = np.abs(q.astype(np.int32) - ref.astype(np.int32))
    share = float((diff > 0).mean())
    print(f"pair {pair} {mode}: max {diff.max()} level, share of differing bytes {share:.2e}")
    assert q.shape == ref.shape == (CM.CT_SIZE, CM.CT_SIZE, 3) and diff.max() <= 1 and share <= MAX_SHARE, (diff.max(), share)
    assert (q != d).mean() > 0.2                                            # the transfer does something
    assert composed.dtype == np.float32 and np.array_equal(composed[md[..., 0] == 0], d[md[..., 0] == 0].astype(np.float32))


def test_masks_of_the_pairs_are_what_the_fixture_asks_for():
    """Pair 0 under binary ellipses, pair 1 under bilinear-softened masks (exact 0 and 1 and values between), pair 2 one of each."""
    kinds = []
    for i in range(CM.CT_PAIRS):
        _, _, md, mt = CM.ct_pair(i)
        kinds.append(tuple(bool(((m > 0) & (m < 1)).any()) for m in (md, mt)))
        assert all((m == 0).any() and (m == 1).any() and m.dtype == np.float32 for m in (md, mt))
    assert kinds == [(False, False), (True, True), (True, False)]


def test_empty_masks_give_finite_coefficients_in_the_model():
    d, t, md, mt = CM.ct_pair(0, 32)
    zero = np.zeros_like(md)
    for mode in CM.MODES:
        for ms, mtt in ((zero, mt), (md, zero), (zero, zero)):
            a, mu0, mu1 = CM.coefficients(CM.inner(d, ms), CM.inner(t, mtt), mode)
            assert np.isfinite(a).all() and np.isfinite(mu0).all() and np.isfinite(mu1).all(), mode
            composed, q = CM.skin_color_transfer(d, t, ms, mtt, mode)
            assert np.isfinite(composed).all()


# ------------------------------------------------------------------------------------------------ library and host logic
NEW_SYMBOLS = ("e4s_grey_morph", "e4s_ct_moments_scratch_bytes", "e4s_ct_moments", "e4s_ct_solve", "e4s_ct_apply")


def test_library_exports_the_colour_transfer_entry_points():
    from e4s2024_amd import _lib
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/e4s_hip.h"
        assert name in _lib._PROTOS and hasattr(L.cdll, name), f"{name} is not exported by {L.path}"


def test_colour_transfer_argument_errors_without_a_launch():
    from e4s2024_amd import ops
    from e4s2024_amd._lib import lib
    c = lib().cdll
    one = ctypes.c_void_p(16)          # non-null dummy pointers: validation fails before they are touched
    two = ctypes.c_void_p(32)
    assert c.e4s_grey_morph(one, two, 1, 8, 8, -1, 0, None) == -1 and b"radius" in c.e4s_last_error()
    assert c.e4s_grey_morph(one, two, 1, 8, 8, 17, 0, None) == -1
    assert c.e4s_grey_morph(one, two, 1, 8, 8, 2, 2, None) == -1 and b"op" in c.e4s_last_error()
    assert c.e4s_grey_morph(one, two, 1, 0, 8, 2, 0, None) == -1
    assert c.e4s_grey_morph(one, one, 1, 8, 8, 2, 0, None) == -1          # in place
    assert c.e4s_grey_morph(one, None, 1, 8, 8, 2, 0, None) == -1
    assert c.e4s_grey_morph(None, None, 0, 8, 8, 2, 0, None) == 0         # no planes: nothing to do
    nbytes = ctypes.c_int64(-1)
    assert c.e4s_ct_moments_scratch_bytes(3, 1024, 1024, ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * 9 * 3 * 256
    assert c.e4s_ct_moments_scratch_bytes(2, 37, 53, ctypes.byref(nbytes)) == 0 and nbytes.value == 8 * 9 * 2 * 1
    assert c.e4s_ct_moments_scratch_bytes(2, 0, 53, ctypes.byref(nbytes)) == -1
    assert c.e4s_ct_moments_scratch_bytes(2, 8, 8, None) == -1
    assert c.e4s_ct_moments(one, one, None, 1, 8, 8, None) == -1
    assert c.e4s_ct_moments(None, None, None, 0, 8, 8, None) == 0
    assert c.e4s_ct_solve(one, one, one, 1, 8, 8, 2, None) == -1 and b"mode" in c.e4s_last_error()
    assert c.e4s_ct_solve(one, None, one, 1, 8, 8, 0, None) == -1
    assert c.e4s_ct_apply(one, None, one, one, None, 1, 8, 8, None) == -1
    assert c.e4s_ct_apply(None, None, None, None, None, 0, 8, 8, None) == 0
    # the Python layer: checks come before any launch, so they work on CPU tensors too
    x = torch.zeros(1, 1, 8, 8)
    for fn in (ops.grey_dilate, ops.grey_erode):
        for bad in (-1, 17, 2.0, True):
            with pytest.raises(ValueError, match="radius"):
                fn(x, bad)
        with pytest.raises(ValueError, match="float32"):
            fn(x.double(), 2)
        with pytest.raises(ValueError, match="float32"):
            fn(x.to(torch.uint8), 2)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(x, 2)
    with pytest.raises(ValueError, match="radius"):
        ops.soft_expansion_masks(x, -1)
    with pytest.raises(ValueError, match="kernel_size"):
        ops.soft_expansion_masks(x, 2, kernel_size=4)
    with pytest.raises(ValueError, match=r"float32 \[bs, 1, H, W\]"):
        ops.soft_expansion_masks(torch.zeros(1, 2, 8, 8), 2)
    with pytest.raises(ValueError, match=r"float32 \[bs, 1, H, W\]"):
        ops.soft_expansion_masks(torch.zeros(1, 1, 8, 8, dtype=torch.uint8), 2)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.soft_expansion_masks(x, 2)
    fr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for bad in ("rct", "mix", "sot", "idt", "adaptive", "blender", "LCT", None, 0):
        with pytest.raises(ValueError, match=r"\['lct', 'mkl'\]"):
            ops.skin_color_transfer(fr, fr, x, x, bad)
    with pytest.raises(ValueError, match="cv2"):
        ops.skin_color_transfer(fr, fr, x, x, "rct")
    with pytest.raises(ValueError, match="uint8"):
        ops.skin_color_transfer(fr.float(), fr, x, x, "lct")
    with pytest.raises(ValueError, match="differ in shape"):
        ops.skin_color_transfer(fr, fr[:, :4], x, x, "lct")
    with pytest.raises(ValueError, match="float32"):
        ops.skin_color_transfer(fr, fr, x.double(), x, "lct")
    with pytest.raises(ValueError, match="trg_mask"):
        ops.skin_color_transfer(fr, fr, x, x[:, :, :4], "mkl")
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.skin_color_transfer(fr, fr, x, x, "mkl")
    for name in ("grey_dilate", "grey_erode", "soft_expansion_masks", "skin_color_transfer", "CT_MODES"):
        assert name in ops.__dict__ and name in __import__("e4s2024_amd.ops_post", fromlist=["__all__"]).__all__
    assert ops.CT_MODES == CM.MODES


def test_pipeline_argument_errors_without_a_launch():
    from e4s2024_amd import pipeline
    assert pipeline.CT_FACE_CLASSES == CM.CT_FACE_CLASSES and pipeline.CT_BORDER_RADIUS == 10
    fr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(TypeError, match="ct_mode and recolor_fn"):
        pipeline.swap_images(None, None, None, fr, None, recolor_fn=lambda s, c: s, ct_mode="lct")
    for bad in ("rct", "blender", "pca"):
        with pytest.raises(ValueError, match=r"\['lct', 'mkl'\]"):
            pipeline.swap_images(None, None, None, fr, None, ct_mode=bad)
        with pytest.raises(ValueError, match=r"\['lct', 'mkl'\]"):
            pipeline.color_transfer(fr, fr, lab, lab, bad)
    with pytest.raises(ValueError, match="uint8"):
        pipeline.color_transfer(fr.float(), fr, lab, lab)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        pipeline.color_transfer(fr, fr, lab, lab)
