"""Row f15 without a GPU: tests/gpen_paste_model.py (the numpy restatement of what ``FaceEnhancement.process`` does between its networks, which
csrc/gpen_paste.hip follows) against g26_gpen_paste.npz — the reference's own reference points, its own ``(tfm, tfm_inv)`` on 24 landmark sets, and its own
``process`` run over the model's functions as its cv2 on cases A - E — single-change mutants of the model, the host-side argument checks, and the names."""
import contextlib
import os

import numpy as np
import pytest
import torch

import gpen_paste_model as PM
from conftest import GOLDEN

ENTRY_POINTS = {"e4s_gpen_face_transforms", "e4s_gpen_warp_crop_u8", "e4s_gpen_smooth3_u8", "e4s_gpen_mask_feather_scratch_bytes", "e4s_gpen_mask_feather",
                "e4s_gpen_paste_u8"}
# sets.deviation: the reference's float32 path (warp_and_crop_face casts to float32) against its own _umeyama run on the same points in float64, relative to the
# matrix's largest entry, the largest over the fixture's landmark sets (make_golden_gpen_paste.py measures and stores it: 8.7e-7).  The closed form is held to 4 x that
DEVIATION_FACTOR = 4


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "g26_gpen_paste.npz")) as z:
        return {k: z[k] for k in z.files}


@contextlib.contextmanager
def mutant(name):
    assert name in PM.MUTANTS and not PM.MUT
    PM.MUT.add(name)
    try:
        yield
    finally:
        PM.MUT.clear()


def test_reference_points(golden):
    from e4s2024_amd import ops
    for S in (512, 32, 48):
        assert np.abs(PM.reference_points(S) - golden[f"ref.{S}"]).max() <= 1e-12
        assert np.abs(ops.gpen_reference_points(S) - golden[f"ref.{S}"]).max() <= 1e-12
    assert np.allclose(ops.gpen_reference_points(512)[0], (202.04068428, 242.88396346), atol=1e-8, rtol=0)
    with pytest.raises(ValueError, match="size.*0"):
        ops.gpen_reference_points(0)


def test_closed_form_against_the_reference_transforms(golden):
    sets, tfm, inv = golden["sets.landms"], golden["sets.tfm"], golden["sets.tfm_inv"]
    assert len(sets) == 24
    dev = []
    for l, a, b in zip(sets, tfm, inv):
        m, mi, ok = PM.similarity_pair(l, golden["ref.512"])
        assert ok
        dev.append(max(np.abs(m - a).max() / np.abs(a).max(), np.abs(mi - b).max() / np.abs(b).max()))
        full, full_inv = np.vstack([m, [0, 0, 1]]), np.vstack([mi, [0, 0, 1]])
        assert np.abs(full_inv @ full - np.eye(3))[:2, :2].max() <= 1e-5
        assert np.abs((full_inv @ full - np.eye(3))[:2, 2]).max() <= 1e-5 * max(1.0, np.abs(mi[:, 2]).max())
        # and it is the least-squares similarity: the forward matrix carries the landmarks' centroid to the reference points'
        src = l.reshape(2, 5).astype(np.float64)
        assert np.abs(m[:, :2] @ src.mean(1) + m[:, 2] - golden["ref.512"].astype(np.float32).astype(np.float64).mean(0)).max() <= 1e-9
    own = float(golden["sets.deviation"])
    print(f"closed form against the reference's float32 path: worst {max(dev):.3e}; that path against the reference's own float64 _umeyama: {own:.3e}")
    assert 1e-8 < own < 1e-5 and max(dev) <= DEVIATION_FACTOR * own
    # the mirrored set has det(A) < 0: the closed form still gives a proper rotation, as _umeyama's d = (1, -1) does
    assert np.linalg.det(tfm[22][:, :2]) > 0 and np.linalg.det(PM.similarity_pair(sets[22], golden["ref.512"])[0][:, :2]) > 0


def test_degenerate_landmarks_are_skipped():
    ref = PM.reference_points(32)
    T, flags = PM.transforms(np.array([[0, 0, 50, 50, 0.99]] * 3, np.float32),
                             np.array([[5] * 10, [1, 2, 3, 4, np.nan, 1, 2, 3, 4, 5], [1, 9, 4, 2, 7, 3, 3, 8, 1, 6]], np.float32), ref, 0.9, 100)
    assert flags.tolist() == [3, 3, 2] and not T[:2].any() and T[2].any()


@pytest.mark.parametrize("tag", PM.CASE_TAGS)
def test_model_against_the_recorded_process(tag, golden):
    """The reference's ``process`` ran over the model's functions: with its recorded matrices the model's own loop gives its images exactly."""
    rec = PM.load_case(golden, tag)
    out, orig, fm, pre, flags, faces, masks = PM.model_outputs(rec)
    assert np.array_equal(out, rec["out"]) and np.array_equal(orig, rec["orig"])
    S, H, W, k, sigma, thres, small = PM.config(rec)
    assert out.shape == (H, W, 3) and orig.shape == (int((flags & 1 == 0).sum()), S, S, 3)
    # with its own float64 transforms the model lands within a grey level or two of it (the matrices differ by 1e-6)
    if len(flags):
        T, flags2 = PM.transforms(rec["dets"], rec["landms"], golden[f"ref.{S}"], 0.9, small)
        assert np.array_equal(flags, flags2)
        own = PM.model_outputs(rec, T)[0]
        assert (own != rec["out"]).mean() < 0.02
        # and the model's own loop over callables, FaceEnhancement.process as a whole, is that composition
        kept = np.flatnonzero(flags & PM.FACE_SKIP == 0)
        faces_in, masks_in = iter(rec["ef"][kept]), iter(rec["pm"][kept])
        whole = PM.process(rec["frame"], rec["dets"], rec["landms"], lambda of: next(faces_in), lambda ef: next(masks_in), S, k, sigma, thres, 0.9, small,
                           rec.get("base"))
        assert np.array_equal(whole[0], own) and len(whole[1]) == len(kept) and np.array_equal(whole[5], T)
    if tag == "D":
        assert np.array_equal(out, rec["frame"])
    if tag == "C":
        assert not np.array_equal(out, PM.load_case(golden, "A")["out"])


def test_cases_are_what_they_claim(golden):
    fl = {t: PM.flags_of(golden[f"{t}.dets"], 0.9, PM.config(PM.load_case(golden, t))[6]).tolist() for t in PM.CASE_TAGS}
    assert fl == {"A": [2, 2, 2], "B": [0, 3, 2], "C": [2, 2, 2], "D": [], "E": [2, 2]}
    assert golden["B.frame"].shape == (70, 53, 3) and golden["A.frame"].shape == (80, 96, 3) and "C.base" in golden and "A.base" not in golden
    for tag in ("A", "B", "C", "D"):                     # the strictness the GPU test asserts holds for the model alone
        rec = PM.load_case(golden, tag)
        out, orig, fm, pre, flags, faces, masks = PM.model_outputs(rec)
        strict = PM.strict_pixels(rec["base"] if "base" in rec else rec["frame"], faces, masks, rec["T"], flags)
        assert strict.mean() >= 0.99, tag
    a = PM.load_case(golden, "A")
    fm = PM.model_outputs(a)[2]
    assert (fm[:, -1] > 0.05).any() and (fm > 0.9).any()            # a face hangs over the frame's edge; the masks reach 1


MUTANT_CASES = {"blur_once": "A", "border_kept": "A", "reflect": "A", "no_round_offset": "A", "truncate": "A", "ge": "E", "reverse": "E", "small_max": "B",
                "not_inverted": "A"}


@pytest.mark.parametrize("name", PM.MUTANTS)
def test_every_mutant_moves_a_stored_output(name, golden):
    if name == "half_up":
        args = (golden["half.base"], [golden["half.mask"]], [golden["half.img"]])
        assert np.array_equal(PM.compose(*args)[0], golden["half.out"])
        with mutant(name):
            assert not np.array_equal(PM.compose(*args)[0], golden["half.out"])
        return
    rec = PM.load_case(golden, MUTANT_CASES[name])
    with mutant(name):
        out, orig = PM.model_outputs(rec)[:2]
    moved = int((out != rec["out"]).sum()) + int((orig != rec["orig"]).sum())
    print(f"mutant {name} on {MUTANT_CASES[name]}: {moved} bytes moved")
    assert moved > 0


def test_uint8_weights_are_the_tables():
    """OpenCV's 15-bit bilinear table entries are 32 times (32 - ax)(32 - ay) ...: they sum to 32768 without its correction step, so
    (sum v w32 + 16384) >> 15 is (sum v w + 512) >> 10."""
    a = np.arange(32)
    w = np.stack([np.outer(32 - a, 32 - a), np.outer(32 - a, a), np.outer(a, 32 - a), np.outer(a, a)])
    assert (w.sum(0) == 1024).all() and ((32 * w).sum(0) == 32768).all()
    rng = np.random.default_rng(0)
    v = rng.integers(0, 256, (4, 32, 32))
    assert np.array_equal(((v * 32 * w).sum(0) + 16384) >> 15, ((v * w).sum(0) + 512) >> 10)


def test_blur_is_exact_where_it_must_be():
    ones = PM.gaussian_blur(np.ones((12, 12)), 9, 1.5)
    assert np.abs(ones - 1).max() <= 4e-16 and PM.gaussian_blur(np.zeros((12, 12)), 9, 1.5).max() == 0
    assert abs(PM.gaussian_taps(101, 11).sum() - 1) <= 1e-15 and PM.gaussian_taps(101, 11).argmax() == 50
    with pytest.raises(ValueError, match="ksize 9"):
        PM.gaussian_blur(np.zeros((4, 4)), 9, 1.5)
    s = np.arange(25).reshape(5, 5).astype(np.uint8)
    sm = PM.filter2d_smooth(np.stack([s] * 3, -1))
    assert sm[2, 2, 0] == 12 and sm[0, 0, 0] == 3               # (4*0 + 2*(1+5+1+5) ... reflect-101 of the corner: (0*4 + 2*1*2 + 2*5*2 + 6*4) / 16 = 3
    assert PM.convert_scale_abs(np.array([0.5, 1.5, 2.5, 300, -3.2], np.float32)).tolist() == [0, 2, 2, 255, 3]


def test_host_checks_refuse_by_name():
    from e4s2024_amd import ops
    u8 = torch.uint8
    with pytest.raises(ValueError, match=r"dets \[n, 5\].*\(2, 4\)"):
        ops.gpen_face_transforms(torch.zeros(2, 4), torch.zeros(2, 10), PM.reference_points(32))
    with pytest.raises(RuntimeError, match="dets must be a CUDA tensor"):
        ops.gpen_face_transforms(torch.zeros(2, 5), torch.zeros(2, 10), PM.reference_points(32))
    with pytest.raises(ValueError, match="threshold.*nan"):
        ops.gpen_face_transforms(torch.zeros(2, 5), torch.zeros(2, 10), PM.reference_points(32), threshold=float("nan"))
    with pytest.raises(ValueError, match="ksize 10"):
        ops.gpen_mask_feather(torch.zeros(1, 32, 32, dtype=u8), 10, 1.5, 3)
    with pytest.raises(ValueError, match="ksize 101 on 32 x 32"):
        ops.gpen_mask_feather(torch.zeros(1, 32, 32, dtype=u8))
    with pytest.raises(ValueError, match="ksize.*131"):
        ops.gpen_mask_feather(torch.zeros(1, 512, 512, dtype=u8), 131, 11., 20)
    with pytest.raises(ValueError, match="sigma.*0"):
        ops.gpen_mask_feather(torch.zeros(1, 32, 32, dtype=u8), 9, 0, 3)
    with pytest.raises(ValueError, match="thres.*0"):
        ops.gpen_mask_feather(torch.zeros(1, 32, 32, dtype=u8), 9, 1.5, 0)
    with pytest.raises(ValueError, match=r"masks_u8.*\(1, 32, 30\)"):
        ops.gpen_mask_feather(torch.zeros(1, 32, 30, dtype=u8), 9, 1.5, 3)
    with pytest.raises(ValueError, match=r"faces_u8.*torch.float32"):
        ops.gpen_smooth_small(torch.zeros(1, 8, 8, 3), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"flags \(2,\) for 1 faces"):
        ops.gpen_smooth_small(torch.zeros(1, 8, 8, 3, dtype=u8), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"transforms.*\(1, 2, 3\)"):
        ops.gpen_warp_crop(torch.zeros(1, 8, 8, 3, dtype=u8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 3, dtype=torch.float64), 8)
    with pytest.raises(ValueError, match="size.*5000"):
        ops.gpen_warp_crop(torch.zeros(1, 8, 8, 3, dtype=u8), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 2, 3, dtype=torch.float64), 5000)
    args = (torch.zeros(1, 8, 8, 3, dtype=u8), torch.zeros(2, 4, 4, 3, dtype=u8), torch.zeros(2, 4, 4), torch.zeros(2, 2, 2, 3, dtype=torch.float64),
            torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"face_begin.*\[2\].*\(3,\)"):
        ops.gpen_paste(*args, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"masks.*\(2, 4, 5\)"):
        ops.gpen_paste(args[0], args[1], torch.zeros(2, 4, 5), *args[3:], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="base_u8 must be a CUDA tensor"):
        ops.gpen_paste(*args, torch.zeros(2, dtype=torch.int32))
    assert ops.GPEN_PASTE_DEFAULTS == {"ksize": 101, "sigma": 11, "thres": 20, "threshold": 0.9, "small_face": 100}


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_gpen_paste, pipeline
    for name in ("gpen_reference_points", "gpen_face_transforms", "gpen_warp_crop", "gpen_smooth_small", "gpen_mask_feather", "gpen_paste", "GPEN_PASTE_DEFAULTS"):
        assert name in ops_gpen_paste.__all__ and getattr(ops, name) is getattr(ops_gpen_paste, name)
    assert (ops.GPEN_FACE_SKIP, ops.GPEN_FACE_SMALL) == (PM.FACE_SKIP, PM.FACE_SMALL)
    assert callable(pipeline.gpen_enhance_frames)
    assert e4s2024_amd.GPEN_ALIGN_OVERRIDES == {"swap_face_fine.gpen.align_faces": "swap_face_fine/gpen/align_faces.py"}
    assert set(e4s2024_amd.GPEN_ALIGN_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert "GPEN_ALIGN_OVERRIDES" in e4s2024_amd.install.__doc__
    path = os.path.join(e4s2024_amd.DROPIN_DIR, e4s2024_amd.GPEN_ALIGN_OVERRIDES["swap_face_fine.gpen.align_faces"])
    text = open(path).read()
    assert "import cv2" not in text and "import skimage" not in text and "from skimage" not in text
    for doc in (pipeline.gpen_enhance.__doc__, pipeline.gpen_face_mask.__doc__, pipeline.gpen_detect_faces.__doc__):
        assert "stay" in doc.split(".")[-2]                       # the earlier stages' functions and their docstrings are as they were


def test_dropin_reference_points_and_refusals(golden):
    import e4s2024_amd
    e4s2024_amd.install()
    try:
        from swap_face_fine.gpen import align_faces as AF
        assert AF.__file__.startswith(e4s2024_amd.DROPIN_DIR)
        for S in (512, 32, 48):
            assert np.abs(AF.get_reference_facial_points((S, S), 0.25, (0, 0), True) - golden[f"ref.{S}"]).max() <= 1e-12
        assert np.array_equal(AF.get_reference_facial_points(), np.array(AF.REFERENCE_FACIAL_POINTS))
        with pytest.raises(AF.FaceWarpException):
            AF.get_reference_facial_points((100, 100))
        with pytest.raises(NotImplementedError, match="'affine'"):
            AF.warp_and_crop_face(np.zeros((4, 4, 3), np.uint8), np.zeros((2, 5)), crop_size=(32, 32), align_type="affine")
        with pytest.raises(AF.FaceWarpException, match="same shape"):
            AF.warp_and_crop_face(np.zeros((4, 4, 3), np.uint8), np.zeros((2, 4)), reference_pts=golden["ref.32"], crop_size=(32, 32))
        with pytest.raises(TypeError, match="float32"):
            AF.warp_and_crop_face(np.zeros((4, 4, 3), np.float32), np.zeros((2, 5)), reference_pts=golden["ref.32"], crop_size=(32, 32))
    finally:
        e4s2024_amd.uninstall()


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert [len(_lib._PROTOS[n]) for n in sorted(ENTRY_POINTS)] == [9, 9, 3, 14, 6, 10]
    assert "double" not in " ".join(l for l in src.splitlines() if "e4s_gpen_" in l and "E4S_API" in l)
    assert _lib.ABI_VERSION == 1
