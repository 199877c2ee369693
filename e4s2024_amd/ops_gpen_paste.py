"""Row f15: GPEN face enhancement, stage 4 — what ``FaceEnhancement.process(aligned=False)`` (swap_face_fine/gpen/face_enhancement.py:68-108) does between its
three networks, on the device (csrc/gpen_paste.hip), in OpenCV's arithmetic as tests/gpen_paste_model.py restates it:

    gpen_reference_points   get_reference_facial_points((S, S), 0.25, (0, 0), True) (align_faces.py:102-184), float64 on the host
    gpen_face_transforms    the 5-point similarity pair of warp_and_crop_face (:210-266, _umeyama :25-93) per face in float64 closed form, and the face flags
    gpen_warp_crop          cv2.warpAffine(frame, tfm, (S, S), flags=3) per face
    gpen_smooth_small       cv2.filter2D(ef, -1, kernel) of the faces whose small flag is set
    gpen_mask_feather       mask_postprocess(mask / 255.): the zeroed border and the two Gaussian blurs, float64 inside
    gpen_paste              the two cv2.warpAffine back to the frame, the "largest mask wins" composition over the faces and cv2.convertScaleAbs of the blend,
                            one pass over the frame

Transforms travel as float64 ``[n, 2, 2, 3]`` (forward, inverse), flags as int32 ``[n]`` (``GPEN_FACE_SKIP``, ``GPEN_FACE_SMALL``).  No host synchronisation
anywhere; the same inputs give the same bits; every call captures in a graph.  Every argument is checked before any launch."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._lib import lib
from .ops import _p, _stream
from .netweights import _cuda_checked, _tensor_checked

GPEN_PASTE_DEFAULTS = {"ksize": 101, "sigma": 11, "thres": 20, "threshold": 0.9, "small_face": 100}        # face_enhancement.py:24, 44-48, 75, 93
GPEN_FACE_SKIP, GPEN_FACE_SMALL = 1, 2
GPEN_FEATHER_MAX_KSIZE = 129
GPEN_MAX_FACE_SIZE = 4096
_REFERENCE_FACIAL_POINTS = ((30.29459953, 51.69630051), (65.53179932, 51.50139999), (48.02519989, 71.73660278), (33.54930115, 92.3655014),
                            (62.72990036, 92.20410156))                      # align_faces.py:14-20, on its 96 x 112 crop


def _size_checked(name, nm, v, lo=1, hi=GPEN_MAX_FACE_SIZE):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name}: {nm} must be an integer in {lo} .. {hi}, got {v!r}")
    return int(v)


def gpen_reference_points(size: int) -> np.ndarray:
    """``get_reference_facial_points((size, size), 0.25, (0, 0), True)``: float64 ``[5, 2]`` (x, y) on the host — the 96 x 112 points made square (x + 8),
    padded by a quarter (+ 28, a 168 crop) and resized by ``size / 168``.  (202.04068428, 242.88396346) is the first at 512."""
    size = _size_checked("gpen_reference_points", "size", size)
    pts = np.array(_REFERENCE_FACIAL_POINTS, np.float64)
    pts += np.array([16, 0]) / 2
    pts += np.array([112, 112]) * 0.25 * 2 / 2
    return pts * (np.float32(size) / np.int64(168))


def _float_checked(name, nm, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)):
        raise ValueError(f"{name}: {nm} must be a finite number, got {v!r}")
    return float(v)


def _transforms_checked(name, transforms, flags, n=None):
    _tensor_checked(name, "transforms", transforms, torch.float64, 4, "a float64 [n, 2, 2, 3] tensor (forward, inverse)")
    if tuple(transforms.shape[1:]) != (2, 2, 3) or (n is not None and transforms.shape[0] != n):
        raise ValueError(f"{name}: transforms: expected float64 [{'n' if n is None else n}, 2, 2, 3], got {tuple(transforms.shape)}")
    if flags is not None:
        _tensor_checked(name, "flags", flags, torch.int32, 1, "an int32 [n] tensor")
        if flags.shape[0] != transforms.shape[0]:
            raise ValueError(f"{name}: flags {tuple(flags.shape)} for {transforms.shape[0]} transforms")


def _same_device(name, first_nm, first, **others):
    _cuda_checked(name, **{first_nm: first}, **others)
    for nm, t in others.items():
        if t.device != first.device:
            raise RuntimeError(f"{name}: device mismatch: {first_nm} on {first.device}, {nm} on {t.device}")


def _faces_checked(name, nm, t):
    _tensor_checked(name, nm, t, torch.uint8, 4, "uint8 [n, S, S, 3] faces")
    if t.shape[3] != 3 or t.shape[1] != t.shape[2] or not 1 <= t.shape[1] <= GPEN_MAX_FACE_SIZE:
        raise ValueError(f"{name}: {nm}: expected uint8 [n, S, S, 3] faces with S in 1 .. {GPEN_MAX_FACE_SIZE}, got {tuple(t.shape)}")


def _frames_checked(name, nm, t):
    _tensor_checked(name, nm, t, torch.uint8, 4, "uint8 [bs, H, W, 3] frames")
    if t.shape[3] != 3 or t.shape[0] < 1 or min(t.shape[1:3]) < 1 or max(t.shape[1:3]) > 32768:
        raise ValueError(f"{name}: {nm}: expected uint8 [bs, H, W, 3] frames with bs >= 1 and sides in 1 .. 32768, got {tuple(t.shape)}")


def gpen_face_transforms(dets: torch.Tensor, landms: torch.Tensor, ref_points, threshold: float = GPEN_PASTE_DEFAULTS["threshold"],
                         small_face: float = GPEN_PASTE_DEFAULTS["small_face"]):
    """``(transforms float64 [n, 2, 2, 3], flags int32 [n])`` from the detector's ``dets [n, 5]`` and ``landms [n, 10]`` (x0..x4, y0..y4) on the device and the
    reference points (``gpen_reference_points``: anything ``[5, 2]`` numpy takes).  ``transforms[i, 0]`` is
    ``warp_and_crop_face``'s forward matrix, ``[i, 1]`` its ``tfm_inv``, the least-squares similarity pair in float64 closed form — the reference's SVD runs in
    float32 and lies about 1e-6 away.  Flags: ``GPEN_FACE_SKIP`` for ``score < threshold`` (face_enhancement.py:75), and for landmarks that are not finite or
    all coincide (the reference raises there); ``GPEN_FACE_SMALL`` for ``min(h, w) < small_face`` (:93)."""
    name = "gpen_face_transforms"
    _tensor_checked(name, "dets", dets, torch.float32, 2, "a float32 [n, 5] tensor")
    _tensor_checked(name, "landms", landms, torch.float32, 2, "a float32 [n, 10] tensor")
    if dets.shape[1] != 5 or landms.shape[1] != 10 or dets.shape[0] != landms.shape[0]:
        raise ValueError(f"{name}: expected dets [n, 5] and landms [n, 10], got {tuple(dets.shape)} and {tuple(landms.shape)}")
    threshold, small_face = _float_checked(name, "threshold", threshold), _float_checked(name, "small_face", small_face)
    _same_device(name, "dets", dets, landms=landms)
    ref = np.asarray(ref_points, np.float64)
    if ref.shape != (5, 2) or not np.isfinite(ref).all():
        raise ValueError(f"{name}: ref_points: expected five finite (x, y) points, got shape {ref.shape}")
    ref = torch.from_numpy(np.ascontiguousarray(ref)).to(dets.device)
    n = dets.shape[0]
    T = torch.empty((n, 2, 2, 3), dtype=torch.float64, device=dets.device)
    flags = torch.empty((n,), dtype=torch.int32, device=dets.device)
    lib().call("e4s_gpen_face_transforms", _p(T), _p(flags), _p(dets.contiguous()), _p(landms.contiguous()), _p(ref), threshold, small_face, n, _stream())
    return T, flags


def gpen_warp_crop(frames_u8: torch.Tensor, frame_of_face: torch.Tensor, transforms: torch.Tensor, size: int) -> torch.Tensor:
    """``cv2.warpAffine(frame, tfm, (size, size), flags=3)`` per face (align_faces.py:264): uint8 ``[bs, H, W, 3]`` frames, ``frame_of_face`` int32 ``[n]``
    (the frame each face is cut from; an index outside the batch gives a zero crop) and ``transforms [n, 2, 2, 3]`` (the forward matrices are read) to the uint8
    crops ``[n, size, size, 3]``, bit for bit OpenCV's fixed-point bilinear."""
    name = "gpen_warp_crop"
    _frames_checked(name, "frames_u8", frames_u8)
    _tensor_checked(name, "frame_of_face", frame_of_face, torch.int32, 1, "an int32 [n] tensor")
    _transforms_checked(name, transforms, None, frame_of_face.shape[0])
    size = _size_checked(name, "size", size)
    _same_device(name, "frames_u8", frames_u8, frame_of_face=frame_of_face, transforms=transforms)
    n, (bs, H, W, _) = frame_of_face.shape[0], frames_u8.shape
    out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=frames_u8.device)
    lib().call("e4s_gpen_warp_crop_u8", _p(out), _p(frames_u8.contiguous()), _p(frame_of_face.contiguous()), _p(transforms.contiguous()), n, bs, H, W, size,
               _stream())
    return out


def gpen_smooth_small(faces_u8: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """``cv2.filter2D(ef, -1, kernel)`` with the 3 x 3 binomial kernel (face_enhancement.py:32-35, 93-94) of the faces whose ``GPEN_FACE_SMALL`` flag is set, a
    copy of the others: uint8 ``[n, S, S, 3]`` to the same.  The flag is read on the device."""
    name = "gpen_smooth_small"
    _faces_checked(name, "faces_u8", faces_u8)
    _tensor_checked(name, "flags", flags, torch.int32, 1, "an int32 [n] tensor")
    if flags.shape[0] != faces_u8.shape[0]:
        raise ValueError(f"{name}: flags {tuple(flags.shape)} for {faces_u8.shape[0]} faces")
    _same_device(name, "faces_u8", faces_u8, flags=flags)
    out = torch.empty(tuple(faces_u8.shape), dtype=torch.uint8, device=faces_u8.device)
    lib().call("e4s_gpen_smooth3_u8", _p(out), _p(faces_u8.contiguous()), _p(flags.contiguous()), faces_u8.shape[0], faces_u8.shape[1], _stream())
    return out


def gpen_gaussian_taps(ksize: int, sigma: float) -> np.ndarray:
    """``cv2.getGaussianKernel(ksize, sigma)`` for ``sigma > 0`` in float64: ``exp(-0.5 x^2 / sigma^2)`` over its sum."""
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    t = np.exp(-0.5 * x * x / (float(sigma) * float(sigma)))
    return t / t.sum()


def gpen_mask_feather(masks_u8: torch.Tensor, ksize: int = GPEN_PASTE_DEFAULTS["ksize"], sigma: float = GPEN_PASTE_DEFAULTS["sigma"],
                      thres: int = GPEN_PASTE_DEFAULTS["thres"]) -> torch.Tensor:
    """``mask_postprocess(mask / 255.)`` (face_enhancement.py:44-49, 89): uint8 ``[n, S, S]`` parse masks to the float32 paste masks ``[n, S, S]`` — ``thres``
    rows and columns at each edge zeroed, ``cv2.GaussianBlur((ksize, ksize), sigma)`` twice in float64 (rows, then columns, BORDER_REFLECT_101), one rounding to
    float32 at the end.  ``ksize`` is odd, at most 129, and ``ksize // 2 < S`` (OpenCV's reflection needs it)."""
    name = "gpen_mask_feather"
    _tensor_checked(name, "masks_u8", masks_u8, torch.uint8, 3, "uint8 [n, S, S] masks")
    n, S = masks_u8.shape[0], masks_u8.shape[1]
    if masks_u8.shape[2] != S or not 1 <= S <= GPEN_MAX_FACE_SIZE:
        raise ValueError(f"{name}: masks_u8: expected uint8 [n, S, S] masks with S in 1 .. {GPEN_MAX_FACE_SIZE}, got {tuple(masks_u8.shape)}")
    ksize = _size_checked(name, "ksize", ksize, 1, GPEN_FEATHER_MAX_KSIZE)
    if ksize % 2 != 1 or ksize // 2 >= S:
        raise ValueError(f"{name}: ksize {ksize} on {S} x {S} masks: it must be odd with ksize // 2 < S")
    sigma = _float_checked(name, "sigma", sigma)
    if sigma <= 0:
        raise ValueError(f"{name}: sigma must be positive, got {sigma!r} (OpenCV derives a sigma <= 0 from ksize; that is not done here)")
    thres = _size_checked(name, "thres", thres, 1, 1 << 30)
    _cuda_checked(name, masks_u8=masks_u8)
    dev = masks_u8.device
    out = torch.empty((n, S, S), dtype=torch.float32, device=dev)
    nbytes = ctypes.c_int64()
    lib().call("e4s_gpen_mask_feather_scratch_bytes", n, S, ctypes.byref(nbytes))
    scratch = torch.empty((max(nbytes.value, 8) // 8,), dtype=torch.float64, device=dev)
    taps = torch.from_numpy(gpen_gaussian_taps(ksize, sigma)).to(dev)
    lib().call("e4s_gpen_mask_feather", _p(out), _p(masks_u8.contiguous()), _p(taps), _p(scratch), n, S, ksize, thres, _stream())
    return out


def gpen_paste(base_u8: torch.Tensor, faces_u8: torch.Tensor, masks: torch.Tensor, transforms: torch.Tensor, flags: torch.Tensor, face_begin: torch.Tensor,
               out: torch.Tensor = None, return_mask: bool = False):
    """The paste of ``FaceEnhancement.process`` (face_enhancement.py:91, 98-108) for a batch: per frame ``b`` the faces ``face_begin[b] .. face_begin[b + 1] - 1``
    (int32 ``[bs + 1]`` on the device) in order, those flagged ``GPEN_FACE_SKIP`` left out — the float32 ``warpAffine`` of the feathered mask ``masks [n, S, S]``
    and the uint8 one of ``faces_u8 [n, S, S, 3]`` by ``transforms[i, 1]``, ``full_mask`` / ``full_img`` taken where the mask exceeds the running maximum, and
    ``convertScaleAbs(base (1 - full_mask) + full_img full_mask)`` — in one pass over ``base_u8 [bs, H, W, 3]``.  Returns the uint8 frames, with ``return_mask``
    also ``full_mask`` float32 ``[bs, H, W]``.  ``out`` may be ``base_u8`` itself (in place: a lane reads its own pixels before it writes them) or a separate
    contiguous tensor; a partial overlap is refused."""
    name = "gpen_paste"
    _frames_checked(name, "base_u8", base_u8)
    _faces_checked(name, "faces_u8", faces_u8)
    n, S, (bs, H, W, _) = faces_u8.shape[0], faces_u8.shape[1], base_u8.shape
    _tensor_checked(name, "masks", masks, torch.float32, 3, "float32 [n, S, S] masks")
    if tuple(masks.shape) != (n, S, S):
        raise ValueError(f"{name}: masks: expected float32 [{n}, {S}, {S}] beside faces_u8 {tuple(faces_u8.shape)}, got {tuple(masks.shape)}")
    _transforms_checked(name, transforms, flags, n)
    _tensor_checked(name, "face_begin", face_begin, torch.int32, 1, f"an int32 [bs + 1] = [{bs + 1}] tensor")
    if face_begin.shape[0] != bs + 1:
        raise ValueError(f"{name}: face_begin: expected int32 [{bs + 1}] for {bs} frames, got {tuple(face_begin.shape)}")
    _same_device(name, "base_u8", base_u8, faces_u8=faces_u8, masks=masks, transforms=transforms, flags=flags, face_begin=face_begin)
    if out is None:
        base, out = base_u8.contiguous(), torch.empty((bs, H, W, 3), dtype=torch.uint8, device=base_u8.device)
    else:
        _frames_checked(name, "out", out)
        if out.shape != base_u8.shape or not out.is_contiguous() or out.device != base_u8.device:
            raise ValueError(f"{name}: out must be a contiguous uint8 {tuple(base_u8.shape)} tensor on {base_u8.device}, got {tuple(out.shape)}, "
                             f"contiguous: {out.is_contiguous()}, on {out.device}")
        in_place = out.data_ptr() == base_u8.data_ptr() and base_u8.is_contiguous()
        nbytes = bs * H * W * 3
        if not in_place and base_u8.is_contiguous() and out.data_ptr() < base_u8.data_ptr() + nbytes and base_u8.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError(f"{name}: out overlaps base_u8 without being it: pass base_u8 itself for an in-place paste")
        base = out if in_place else base_u8.contiguous()
    full_mask = torch.empty((bs, H, W), dtype=torch.float32, device=base_u8.device) if return_mask else None
    lib().call("e4s_gpen_paste_u8", _p(out), _p(full_mask), _p(base), _p(faces_u8.contiguous()), _p(masks.contiguous()), _p(transforms.contiguous()),
               _p(flags.contiguous()), _p(face_begin.contiguous()), n, bs, H, W, S, _stream())
    return (out, full_mask) if return_mask else out


__all__ = ["GPEN_PASTE_DEFAULTS", "GPEN_FACE_SKIP", "GPEN_FACE_SMALL", "GPEN_FEATHER_MAX_KSIZE", "gpen_reference_points", "gpen_gaussian_taps",
           "gpen_face_transforms", "gpen_warp_crop", "gpen_smooth_small", "gpen_mask_feather", "gpen_paste"]
