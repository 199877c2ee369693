"""Host geometry of the video path's crop-and-align step and of its paste back into the frame (row f5 of the scope table):
from 68 landmarks per frame to one oriented square per face, smoothed over the clip, and from there to the launch plan of the two warp
kernels (``csrc/align.hip``, ``ops.crop_align`` / ``ops.paste_into_frames``).

Reference: ``compute_transform`` (utils/alignment.py:150-220, the active body after the docstring), the quad smoothing of ``crop_faces``
(:222-258), ``crop_image(..., enable_padding=False)`` (:101-147) and ``calc_alignment_coefficients`` (:275-285), called with the target-side
arguments by face_swap_video_pipeline.py:181-210.  Everything here is float64 numpy, in the order the reference and Pillow evaluate it, so
that the warps built from it agree with Pillow's byte for byte; torch is needed only to hand the plan to the device.

Landmark detection is not part of this module: ``lm`` comes from whatever detector the application runs (dlib / face_alignment's
68-point layout)."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np


# ------------------------------------------------------------------------------------------------ the oriented square per frame
def transform_from_landmarks(lm, scale: float = 1.0):
    """``lm`` float ``[n, 68, 2]`` (x, y) -> ``(c, x, y)``, each ``[n, 2]``: the centre and the two half-axes of the face square
    (the eye / mouth rule of ``compute_transform``)."""
    lm = np.asarray(lm, dtype=np.float64)
    if lm.ndim == 2:
        lm = lm[None]
    if lm.ndim != 3 or lm.shape[1:] != (68, 2):
        raise ValueError(f"transform_from_landmarks: landmarks [n, 68, 2], got {lm.shape}")
    n = lm.shape[0]
    c, xs, ys = np.empty((n, 2)), np.empty((n, 2)), np.empty((n, 2))
    for i in range(n):
        eye_left = np.mean(lm[i, 36:42], axis=0)
        eye_right = np.mean(lm[i, 42:48], axis=0)
        eye_avg = (eye_left + eye_right) * 0.5
        eye_to_eye = eye_right - eye_left
        mouth_avg = (lm[i, 48] + lm[i, 54]) * 0.5
        eye_to_mouth = mouth_avg - eye_avg
        x = eye_to_eye - np.flipud(eye_to_mouth) * [-1, 1]
        x /= np.hypot(*x)
        x *= max(np.hypot(*eye_to_eye) * 2.0, np.hypot(*eye_to_mouth) * 1.8)
        x *= scale
        xs[i] = x
        ys[i] = np.flipud(x) * [-1, 1]
        c[i] = eye_avg + eye_to_mouth * 0.1
    return c, xs, ys


def _reflect_index(i: np.ndarray, n: int) -> np.ndarray:
    """Half-sample symmetric extension (``d c b a | a b c d | d c b a``), repeated for any distance from the signal."""
    m = np.mod(i, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def gaussian_smooth(a, sigma: float, truncate: float = 4.0) -> np.ndarray:
    """Gaussian filter along axis 0 with the conventions of ``scipy.ndimage.gaussian_filter1d`` (mode ``'reflect'``, radius
    ``int(truncate * sigma + 0.5)``, the sampled kernel normalised to sum 1).  ``sigma == 0`` returns the input unchanged."""
    a = np.asarray(a, dtype=np.float64)
    if sigma == 0:
        return a.copy()
    if sigma < 0:
        raise ValueError("gaussian_smooth: sigma must be >= 0")
    radius = int(truncate * float(sigma) + 0.5)
    t = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * t.astype(np.float64) ** 2)
    w = w / w.sum()
    n = a.shape[0]
    idx = _reflect_index(np.arange(n)[:, None] + t[None, :], n)         # [n, 2r+1] source index of every tap
    return np.tensordot(a[idx], w, axes=([1], [0])) if a.ndim == 1 else np.einsum("ntk,t->nk", a[idx].reshape(n, 2 * radius + 1, -1), w).reshape(a.shape)


def smooth_transforms(c, x, y, center_sigma: float = 0.0, xy_sigma: float = 0.0):
    """Temporal smoothing of the per-frame squares over a clip (``crop_faces``): the centres with ``center_sigma``, both axes with
    ``xy_sigma``, frame axis 0.  A sigma of 0 leaves that input unchanged."""
    c, x, y = (np.asarray(v, dtype=np.float64) for v in (c, x, y))
    return gaussian_smooth(c, center_sigma), gaussian_smooth(x, xy_sigma), gaussian_smooth(y, xy_sigma)


def quads_from_transforms(c, x, y) -> np.ndarray:
    """``[n, 4, 2]`` corners in Pillow's QUAD order (NW, SW, SE, NE of the output square): ``c-x-y, c-x+y, c+x+y, c+x-y``."""
    c, x, y = (np.asarray(v, dtype=np.float64) for v in (c, x, y))
    return np.stack([c - x - y, c - x + y, c + x + y, c + x - y], axis=1)


# ------------------------------------------------------------------------------------------------ the launch plan
@dataclass
class CropPlan:
    """Per-frame geometry of ``ops.crop_align`` and ``ops.paste_into_frames`` for frames of ``frame_hw`` = (H, W).

    ``shrink`` int ``[n]`` (1 = none) and ``resized_wh`` int ``[n, 2]``: the frame is first resized to ``resized_wh`` (Lanczos) when its face quad
    is 4 output sizes or more across (its diagonal).  ``boxes`` int32 ``[n, 4]`` = (x0, y0, x1, y1): the source window of the crop in the (resized)
    frame.  ``paste_boxes`` int32 ``[n, 4]``: the frame pixels the paste can touch (the quad's bounding box plus one pixel).  Both box sets size
    the launches and are validated by the host, so they stay host tensors.  ``quad_coeffs`` float64 ``[n, 8]``: Pillow's QUAD data of the
    crop; ``inv_coeffs`` float64 ``[n, 8]``: the PERSPECTIVE data of the paste.  ``.to(device)`` moves the two coefficient tensors."""
    frame_hw: tuple
    output_size: int
    quads: np.ndarray
    shrink: np.ndarray
    resized_wh: np.ndarray
    boxes: "torch.Tensor"  # noqa: F821
    paste_boxes: "torch.Tensor"  # noqa: F821
    quad_coeffs: "torch.Tensor"  # noqa: F821
    inv_coeffs: "torch.Tensor"  # noqa: F821

    def __len__(self):
        return int(self.quads.shape[0])

    def to(self, device) -> "CropPlan":
        return replace(self, quad_coeffs=self.quad_coeffs.to(device), inv_coeffs=self.inv_coeffs.to(device))

    def __getitem__(self, sl) -> "CropPlan":
        """The plan of a contiguous block of frames (``plan[lo:hi]``), e.g. one batch of ``runner.run_clip_streamed``."""
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("CropPlan supports contiguous slices only")
        return replace(self, quads=self.quads[sl], shrink=self.shrink[sl], resized_wh=self.resized_wh[sl], boxes=self.boxes[sl],
                       paste_boxes=self.paste_boxes[sl], quad_coeffs=self.quad_coeffs[sl], inv_coeffs=self.inv_coeffs[sl])


def quad_coefficients(quad, size: int):
    """The 8 QUAD coefficients Pillow's ``Image.transform((size, size), QUAD, quad.flatten())`` derives from the corners (Python floats)."""
    q = [float(v) for v in np.asarray(quad, dtype=np.float64).reshape(8)]
    nw, sw, se, ne = q[0:2], q[2:4], q[4:6], q[6:8]
    x0, y0 = nw
    As = 1.0 / size
    At = 1.0 / size
    return (x0, (ne[0] - x0) * As, (sw[0] - x0) * At, (se[0] - sw[0] - ne[0] + x0) * As * At,
            y0, (ne[1] - y0) * As, (sw[1] - y0) * At, (se[1] - sw[1] - ne[1] + y0) * As * At)


def perspective_coefficients(src_pts, dst_pts) -> np.ndarray:
    """The 8 PERSPECTIVE coefficients that map ``src_pts`` onto ``dst_pts`` (Pillow's data maps output to input coordinates: an output whose
    points ``src_pts`` sample the input at ``dst_pts``): the normal-equation solve ``inv(A^T A) A^T b`` of ``calc_alignment_coefficients``, float64."""
    rows = []
    for (px, py), (qx, qy) in zip(np.asarray(src_pts, dtype=np.float64), np.asarray(dst_pts, dtype=np.float64)):
        rows.append([px, py, 1.0, 0.0, 0.0, 0.0, -qx * px, -qx * py])
        rows.append([0.0, 0.0, 0.0, px, py, 1.0, -qy * px, -qy * py])
    a = np.array(rows, dtype=np.float64)
    b = np.asarray(dst_pts, dtype=np.float64).reshape(8)
    return np.dot(np.linalg.inv(a.T @ a) @ a.T, b).reshape(8)


def crop_plan(quads, frame_hw, output_size: int = 1024) -> CropPlan:
    """``crop_image(frame, output_size, quad, enable_padding=False)`` for every frame, as a plan (see ``CropPlan``).  ``frame_hw`` = (H, W)."""
    import torch
    quads = np.asarray(quads, dtype=np.float64)
    if quads.ndim == 2:
        quads = quads[None]
    if quads.ndim != 3 or quads.shape[1:] != (4, 2) or quads.shape[0] < 1:
        raise ValueError(f"crop_plan: quads [n, 4, 2], got {quads.shape}")
    h, w = int(frame_hw[0]), int(frame_hw[1])
    size = int(output_size)
    if h < 1 or w < 1 or size < 1:
        raise ValueError(f"crop_plan: bad frame {frame_hw} or output size {output_size}")
    if not np.all(np.isfinite(quads)):
        raise ValueError("crop_plan: quads must be finite")
    n = quads.shape[0]
    shrinks, rwh, boxes, pboxes, qc, ic = [], [], [], [], [], []
    corners = [[0, 0], [0, size], [size, size], [size, 0]]
    for i in range(n):
        quad = quads[i].copy()
        qsize = np.hypot(*((quad[3] - quad[1]) / 2)) * 2
        shrink = int(np.floor(qsize / size * 0.5))
        rw, rh = w, h
        if shrink > 1:
            rw, rh = int(np.rint(float(w) / shrink)), int(np.rint(float(h) / shrink))
            quad /= shrink
            qsize /= shrink
        else:
            shrink = 1
        border = max(int(np.rint(qsize * 0.1)), 3)
        box = (int(np.floor(min(quad[:, 0]))), int(np.floor(min(quad[:, 1]))), int(np.ceil(max(quad[:, 0]))), int(np.ceil(max(quad[:, 1]))))
        box = (max(box[0] - border, 0), max(box[1] - border, 0), min(box[2] + border, rw), min(box[3] + border, rh))
        if box[2] < box[0] or box[3] < box[1]:
            raise ValueError(f"crop_plan: the face quad of frame {i} lies outside the {w}x{h} frame")
        if box[2] - box[0] < rw or box[3] - box[1] < rh:
            quad -= box[0:2]
        qc.append(quad_coefficients(quad + 0.5, size))
        q0 = quads[i] + 0.5
        ic.append(perspective_coefficients(q0, corners))
        lo, hi = np.floor(quads[i].min(axis=0)).astype(np.int64) - 1, np.ceil(quads[i].max(axis=0)).astype(np.int64) + 2
        pboxes.append((int(min(max(lo[0], 0), w)), int(min(max(lo[1], 0), h)), int(min(max(hi[0], 0), w)), int(min(max(hi[1], 0), h))))
        shrinks.append(shrink)
        rwh.append((rw, rh))
        boxes.append(box)
    return CropPlan(frame_hw=(h, w), output_size=size, quads=quads.copy(), shrink=np.array(shrinks, dtype=np.int64),
                    resized_wh=np.array(rwh, dtype=np.int64).reshape(n, 2),
                    boxes=torch.tensor(boxes, dtype=torch.int32).reshape(n, 4),
                    paste_boxes=torch.tensor(pboxes, dtype=torch.int32).reshape(n, 4),
                    quad_coeffs=torch.tensor(np.array(qc, dtype=np.float64)).reshape(n, 8),
                    inv_coeffs=torch.tensor(np.array(ic, dtype=np.float64)).reshape(n, 8))


def plan_from_landmarks(lm, frame_hw, output_size: int = 1024, scale: float = 1.0, center_sigma: float = 1.0,
                        xy_sigma: float = 3.0) -> CropPlan:
    """Landmarks ``[n, 68, 2]`` of a clip's consecutive frames -> ``CropPlan``.  The defaults are the target side of the video pipeline
    (face_swap_video_pipeline.py:181-210); a single source image uses ``center_sigma=0, xy_sigma=0``."""
    c, x, y = transform_from_landmarks(lm, scale)
    c, x, y = smooth_transforms(c, x, y, center_sigma, xy_sigma)
    return crop_plan(quads_from_transforms(c, x, y), frame_hw, output_size)


__all__ = ["transform_from_landmarks", "gaussian_smooth", "smooth_transforms", "quads_from_transforms", "CropPlan", "quad_coefficients",
           "perspective_coefficients", "crop_plan", "plan_from_landmarks"]
