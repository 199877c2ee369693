"""Drop-in for the reference's ``swap_face_fine/gpen/align_faces.py``: ``REFERENCE_FACIAL_POINTS``, ``get_reference_facial_points``, ``warp_and_crop_face`` and
``FaceWarpException`` with the reference's signatures, the 5-point similarity transform and the ``cv2.warpAffine`` crop on the device
(``ops.gpen_face_transforms``, ``ops.gpen_warp_crop``).  It takes a numpy image and returns a numpy crop and ``tfm_inv``, as the reference does.  Neither ``cv2``
nor ``skimage`` is imported.

Departures, each stated: the transform is the float64 least-squares solution in closed form (the reference's SVD runs in float32 and lies about 1e-6 from it);
``align_type`` other than ``'smilarity'`` raises ``NotImplementedError`` (``'cv2_affine'`` and ``'affine'`` are never used by ``FaceEnhancement``); the image is
uint8 ``[H, W, 3]`` and there are exactly five points; landmarks that all coincide, or are not finite, raise ``FaceWarpException``."""
import numpy as np
import torch

from e4s2024_amd import ops

# reference facial points, a list of coordinates (x, y) on the default 96 x 112 crop
REFERENCE_FACIAL_POINTS = [
    [30.29459953, 51.69630051],
    [65.53179932, 51.50139999],
    [48.02519989, 71.73660278],
    [33.54930115, 92.3655014],
    [62.72990036, 92.20410156],
]

DEFAULT_CROP_SIZE = (96, 112)


class FaceWarpException(Exception):
    def __str__(self):
        return "In File {}:{}".format(__file__, super().__str__())


def get_reference_facial_points(output_size=None, inner_padding_factor=0.0, outer_padding=(0, 0), default_square=False):
    """The five reference points for a crop of ``output_size`` (w, h): the default points, optionally made square, padded inside by
    ``inner_padding_factor`` of the crop on every side, resized to ``output_size - 2 outer_padding`` and shifted by ``outer_padding``; float64 ``[5, 2]``."""
    pts = np.array(REFERENCE_FACIAL_POINTS)
    crop = np.array(DEFAULT_CROP_SIZE)
    if default_square:
        diff = max(crop) - crop
        pts += diff / 2
        crop += diff
    if output_size and output_size[0] == crop[0] and output_size[1] == crop[1]:
        return pts
    if inner_padding_factor == 0 and outer_padding == (0, 0):
        if output_size is None:
            return pts
        raise FaceWarpException("No paddings to do, output_size must be None or {}".format(crop))
    if not (0 <= inner_padding_factor <= 1.0):
        raise FaceWarpException("Not (0 <= inner_padding_factor <= 1.0)")
    if (inner_padding_factor > 0 or outer_padding[0] > 0 or outer_padding[1] > 0) and output_size is None:
        output_size = crop * (1 + inner_padding_factor * 2).astype(np.int32)
        output_size += np.array(outer_padding)
    if not (outer_padding[0] < output_size[0] and outer_padding[1] < output_size[1]):
        raise FaceWarpException("Not (outer_padding[0] < output_size[0] and outer_padding[1] < output_size[1])")
    if inner_padding_factor > 0:
        diff = crop * inner_padding_factor * 2
        pts += diff / 2
        crop += np.round(diff).astype(np.int32)
    inner = np.array(output_size) - np.array(outer_padding) * 2
    if inner[0] * crop[1] != inner[1] * crop[0]:
        raise FaceWarpException("Must have (output_size - outer_padding) = some_scale * (crop_size * (1.0 + inner_padding_factor)")
    pts = pts * (inner[0].astype(np.float32) / crop[0])
    return pts + np.array(outer_padding)


def _points(pts, what):
    pts = np.float32(pts)
    if pts.ndim != 2 or max(pts.shape) < 3 or min(pts.shape) != 2:
        raise FaceWarpException(what + ".shape must be (K,2) or (2,K) and K>2")
    return pts.T if pts.shape[0] == 2 else pts


def warp_and_crop_face(src_img, facial_pts, reference_pts=None, crop_size=(96, 112), align_type="smilarity"):
    """``(face_img uint8 [crop_size[1], crop_size[0], 3], tfm_inv float64 [2, 3])`` of a uint8 ``[H, W, 3]`` numpy image and its five landmarks, (2, 5) or (5, 2)."""
    if align_type != "smilarity":
        raise NotImplementedError(f"warp_and_crop_face: align_type {align_type!r} is not implemented: the native path is 'smilarity' (the 5-point similarity)")
    if reference_pts is None:
        if crop_size[0] == 96 and crop_size[1] == 112:
            reference_pts = REFERENCE_FACIAL_POINTS
        else:
            reference_pts = get_reference_facial_points(crop_size, 0, (0, 0), False)
    ref, src = _points(reference_pts, "reference_pts"), _points(facial_pts, "facial_pts")
    if src.shape != ref.shape:
        raise FaceWarpException("facial_pts and reference_pts must have the same shape")
    if src.shape != (5, 2):
        raise NotImplementedError(f"warp_and_crop_face: {src.shape[0]} points: the native path takes the detector's five")
    if int(crop_size[0]) != int(crop_size[1]):
        raise NotImplementedError(f"warp_and_crop_face: crop_size {tuple(crop_size)}: the native path cuts square crops")
    img = np.asarray(src_img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise TypeError(f"warp_and_crop_face: src_img must be a uint8 [H, W, 3] array, got {img.dtype} {img.shape}")
    device = "cuda"
    frames = torch.from_numpy(np.ascontiguousarray(img)).to(device)[None]
    landms = torch.from_numpy(np.ascontiguousarray(src.T).reshape(1, 10)).to(device)
    dets = torch.tensor([[0., 0., 0., 0., 1.]], dtype=torch.float32, device=device)
    T, flags = ops.gpen_face_transforms(dets, landms, ref.astype(np.float64), threshold=0., small_face=0.)
    face = ops.gpen_warp_crop(frames, torch.zeros(1, dtype=torch.int32, device=device), T, int(crop_size[0]))
    if int(flags[0]) & ops.GPEN_FACE_SKIP:
        raise FaceWarpException("facial_pts do not determine a similarity transform (they coincide or are not finite)")
    return face[0].cpu().numpy(), T[0, 1].cpu().numpy()
