"""Rows f2 / f3 of the scope table: what the video pipeline does to a frame around the swap — mask surgery, paste-back masks, uint8 <-> float frames,
Pillow's bicubic resize and the multi-band blend (``csrc/maskops.hip``).  Reference: ``swap_face_fine/swap_face_mask.py:194-367``,
``face_swap_video_pipeline.py:447-473``, ``swap_face_fine/multi_band_blending.py:5-74``.  Re-exported by ``ops``.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

from ._lib import lib
from .ops import _c, _p, _stream

# ------------------------------------------------------------------------------------ f2 / f3 (maskops.hip)
def _labels_u8(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError(f"{name}: expected a uint8 [bs, H, W] label map, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def swap_head_mask(source: torch.Tensor, target: torch.Tensor):
    """``swap_head_mask_hole_first`` (swap_face_fine/swap_face_mask.py:194-333) for a batch of 12-class maps on the device.
    ``source`` = the driven face's map, ``target`` = the target frame's map, both uint8 ``[bs, H, W]``.
    Returns ``(res, hole_mask, hole_map, lines)``: uint8 maps (``hole_mask`` in {0,1}) and int32 ``[bs, 2]`` = (eye_line, nose_line)."""
    s, t = _labels_u8(source, "source"), _labels_u8(target, "target")
    if s.shape != t.shape:
        raise ValueError(f"source {tuple(s.shape)} and target {tuple(t.shape)} maps differ in shape")
    bs, h, w = t.shape
    res, hole, hole_map = torch.empty_like(t), torch.empty_like(t), torch.empty_like(t)
    lines = torch.empty((bs, 2), dtype=torch.int32, device=t.device)
    scratch = torch.empty((bs * (3 + w),), dtype=torch.int32, device=t.device)
    if bs == 0:
        return res, hole, hole_map, lines
    lib().call("e4s_swap_head_mask", _p(res), _p(hole), _p(hole_map), _p(lines), _p(s), _p(t), _p(scratch), bs, h, w, _stream())
    return res, hole, hole_map, lines


def foreground_masks(swapped: torch.Tensor, hole_mask: Optional[torch.Tensor] = None, radius: int = 5):
    """Foreground of a swapped map (everything but background / ear-ring / ear / hair / neck, plus the hole:
    face_swap_video_pipeline.py:456-461) and ``create_masks(foreground, operation='expansion', radius)``
    (gradio_utils/face_swapping.py:203-221).  Returns float32 ``[bs, 1, H, W]`` ``(content, border, full)``."""
    m = _labels_u8(swapped, "swapped")
    hm = _labels_u8(hole_mask, "hole_mask") if hole_mask is not None else None
    if hm is not None and hm.shape != m.shape:
        raise ValueError("hole_mask and swapped map differ in shape")
    bs, h, w = m.shape
    content = torch.empty((bs, 1, h, w), dtype=torch.float32, device=m.device)
    border, full = torch.empty_like(content), torch.empty_like(content)
    if bs == 0:
        return content, border, full
    lib().call("e4s_foreground_masks", _p(content), _p(border), _p(full), _p(m), _p(hm), bs, h, w, int(radius), _stream())
    return content, border, full


def frames_to_tensor(frames_u8: torch.Tensor) -> torch.Tensor:
    """uint8 frames ``[bs, H, W, 3]`` -> ``[bs, 3, H, W]`` float in [-1, 1]: ``Compose([ToTensor(), Normalize(.5, .5)])`` (datasets/dataset.py:32, 45;
    face_swap_video_pipeline.py:338-339) on the device, bit for bit (``(x / 255 - 0.5) / 0.5`` in float32)."""
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise ValueError("frames_to_tensor: uint8 [bs, H, W, 3] frames")
    if not frames_u8.is_cuda:
        raise RuntimeError("frames must be a CUDA tensor")
    x = frames_u8.contiguous()
    bs, h, w, _ = x.shape
    out = torch.empty((bs, 3, h, w), dtype=torch.float32, device=x.device)
    lib().call("e4s_frames_to_tensor", _p(out), _p(x), bs, h, w, _stream())
    return out


PTI_BG_CLASSES = (0, 4, 11)        # background, hair, ear-rings: what erode_mask / the PTI foreground leave out (video_swap_ft_coach.py:72, 277)


def erode_labels(labels: torch.Tensor, radius: int, bg_classes: Sequence[int] = PTI_BG_CLASSES) -> torch.Tensor:
    """``erode_mask(mask, img, radius)[0]`` (training/video_swap_ft_coach.py:64-93) for a batch of uint8 ``[bs, H, W]`` 12-class maps."""
    m = _labels_u8(labels, "labels")
    bits = 0
    for c in bg_classes:
        bits |= 1 << int(c)
    out = torch.empty_like(m)
    if m.shape[0]:
        lib().call("e4s_erode_labels", _p(out), _p(m), m.shape[0], m.shape[1], m.shape[2], int(radius), bits, _stream())
    return out


# ------------------------------------------------------------------------------------ f3: Pillow's resize on the device
_pil_tables = {}


def _pil_bicubic_filter(x: float) -> float:
    """Pillow's ``bicubic_filter`` (a = -0.5, support 2)."""
    x = abs(x)
    return ((1.5 * x - 2.5) * x * x + 1.0) if x < 1.0 else ((((x - 5.0) * x + 8.0) * x - 4.0) * -0.5 if x < 2.0 else 0.0)


def _pil_sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _pil_lanczos_filter(x: float) -> float:
    """Pillow's ``lanczos_filter``: the sinc truncated to [-3, 3) and windowed by sinc(x / 3) (not symmetric at the ends, like the library)."""
    return _pil_sinc(x) * _pil_sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_PIL_FILTERS = {"bicubic": (_pil_bicubic_filter, 2.0), "lanczos": (_pil_lanczos_filter, 3.0)}


def _pil_resample_tables(in_size: int, out_size: int, device, resample: str = "bicubic"):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` (src/libImaging/Resample.c) for one filter: per output index the first input
    index, the tap count and the taps in 22-bit fixed point.  Computed once per (in, out, filter, device) in float64 like the library."""
    key = (in_size, out_size, resample, str(device))
    hit = _pil_tables.get(key)
    if hit is None:
        filt, fsupport = _PIL_FILTERS[resample]
        scale = in_size / out_size
        fscale = max(scale, 1.0)
        support = fsupport * fscale
        ksize = int(math.ceil(support)) * 2 + 1
        xmin, cnt, kk = [], [], []
        ss = 1.0 / fscale
        for xx in range(out_size):
            center = (xx + 0.5) * scale
            lo = max(int(center - support + 0.5), 0)
            hi = min(int(center + support + 0.5), in_size)
            ws = [filt((x + lo - center + 0.5) * ss) for x in range(hi - lo)]
            tot = sum(ws)
            if tot != 0.0:
                ws = [v / tot for v in ws]
            row = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in ws]
            xmin.append(lo); cnt.append(hi - lo); kk.append(row + [0] * (ksize - len(row)))
        hit = (torch.tensor(xmin, dtype=torch.int32, device=device), torch.tensor(cnt, dtype=torch.int32, device=device),
               torch.tensor(kk, dtype=torch.int32, device=device), ksize)
        if len(_pil_tables) > 32:
            _pil_tables.clear()
        _pil_tables[key] = hit
    return hit


def _pil_bicubic_tables(in_size: int, out_size: int, device):
    """The BICUBIC tables (Pillow's default resize filter)."""
    return _pil_resample_tables(in_size, out_size, device, "bicubic")


def _pil_lanczos_tables(in_size: int, out_size: int, device):
    """The LANCZOS tables (support 3; Pillow < 10 called this filter ANTIALIAS)."""
    return _pil_resample_tables(in_size, out_size, device, "lanczos")


def pil_resize(img_u8: torch.Tensor, size, resample: str = "bicubic") -> torch.Tensor:
    """``PIL.Image.resize(size)`` (size = (width, height); Pillow's default BICUBIC with its 8-bit fixed-point arithmetic) of uint8
    ``[bs, H, W, C]`` frames on the device, bit for bit: a horizontal then a vertical pass, each rounded to 8 bits
    (face_swap_video_pipeline.py:447 softens the swapped face with ``.resize((512, 512)).resize((1024, 1024))``).
    ``resample="lanczos"``: ``Image.resize(size, LANCZOS)`` (the shrink step of ``crop_align``)."""
    if resample not in _PIL_FILTERS:
        raise ValueError(f"pil_resize: resample is one of {sorted(_PIL_FILTERS)}, got {resample!r}")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or not img_u8.is_cuda:
        raise ValueError("pil_resize: uint8 [bs, H, W, C] CUDA frames")
    wd, ht = int(size[0]), int(size[1])
    out = img_u8.contiguous()
    for axis, target in ((1, wd), (0, ht)):
        bs, h, w, c = out.shape
        if target == (w if axis == 1 else h):
            continue
        xmin, cnt, kk, ksize = _pil_resample_tables(w if axis == 1 else h, target, out.device, resample)
        nxt = torch.empty((bs, h, target, c) if axis == 1 else (bs, target, w, c), dtype=torch.uint8, device=out.device)
        lib().call("e4s_resample_u8", _p(nxt), _p(out), _p(xmin), _p(cnt), _p(kk), ksize, bs, h, w, c, target, axis, _stream())
        out = nxt
    return out


# ------------------------------------------------------------------------------------ f5: crop-align and paste into the frame (align.hip)
def _frames_u8(t: torch.Tensor, name: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
        raise ValueError(f"{name}: expected uint8 [n, H, W, 3] frames, got {t.dtype} {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _plan_checked(plan, frames: torch.Tensor, name: str):
    from .align import CropPlan
    if not isinstance(plan, CropPlan):
        raise TypeError(f"{name}: plan must be an align.CropPlan (align.crop_plan / align.plan_from_landmarks)")
    n, h, w, _ = frames.shape
    if len(plan) != n or tuple(plan.frame_hw) != (h, w):
        raise ValueError(f"{name}: the plan covers {len(plan)} frames of {plan.frame_hw[1]}x{plan.frame_hw[0]}, got {n} of {w}x{h}")
    qc, ic = (t if t.device == frames.device else t.to(frames.device) for t in (plan.quad_coeffs, plan.inv_coeffs))
    return qc.contiguous(), ic.contiguous(), plan.boxes.to(torch.int32).cpu().contiguous(), plan.paste_boxes.to(torch.int32).cpu().contiguous()


def crop_align(frames_u8: torch.Tensor, plan) -> torch.Tensor:
    """``crop_image(frame, S, quad)`` (utils/alignment.py:101-147, ``enable_padding=False``) for a batch of video frames on the device, bit for bit
    with Pillow: uint8 ``[n, H, W, 3]`` frames + ``align.CropPlan`` -> uint8 ``[n, S, S, 3]`` aligned face crops.  A frame whose face quad is 4 S or more
    across (its diagonal) is first resized by its plan's ``shrink`` with Pillow's LANCZOS (``pil_resize``); every other frame is warped straight from
    the input, all of them in one launch."""
    x = _frames_u8(frames_u8, "frames")
    qc, _, boxes, _ = _plan_checked(plan, x, "crop_align")
    n, h, w, _ = x.shape
    s = int(plan.output_size)
    out = torch.empty((n, s, s, 3), dtype=torch.uint8, device=x.device)
    if n == 0:
        return out
    shrink = [int(v) for v in plan.shrink]
    i = 0
    while i < n:
        j = i + 1
        if shrink[i] > 1:           # this frame's own resize, then its warp from the resized frame
            rw, rh = (int(v) for v in plan.resized_wh[i])
            src = pil_resize(x[i:j], (rw, rh), resample="lanczos")
            lib().call("e4s_warp_quad_u8", _p(out[i:j]), _p(src), boxes[i:j].data_ptr(), _p(qc[i:j]), 1, rh, rw, s, _stream())
        else:                       # a run of frames warped from the input as they are
            while j < n and shrink[j] <= 1:
                j += 1
            lib().call("e4s_warp_quad_u8", _p(out[i:j]), _p(x[i:j]), boxes[i:j].data_ptr(), _p(qc[i:j]), j - i, h, w, s, _stream())
        i = j
    return out


def paste_into_frames(faces_u8: torch.Tensor, frames_u8: torch.Tensor, plan, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's "op2. paste back" (face_swap_video_pipeline.py:474-483) for a batch on the device, bit for bit with Pillow: each face crop
    uint8 ``[n, S, S, 3]`` is warped into its frame by ``transform(frame.size, PERSPECTIVE, inv_coeffs, BILINEAR)`` and composited over it as an
    opaque layer.  Only the quad's bounding box (plus one pixel) is read and written.  ``out=None`` returns new frames; ``out=frames_u8`` pastes
    in place; any other contiguous uint8 ``[n, H, W, 3]`` buffer receives a copy of the frames, then the faces."""
    x = _frames_u8(frames_u8, "frames")
    n, h, w, _ = x.shape
    _, ic, _, pboxes = _plan_checked(plan, x, "paste_into_frames")
    s = int(plan.output_size)
    f = _frames_u8(faces_u8, "faces", (n, s, s, 3))
    if out is None:
        out = x.clone()
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch.Tensor")
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"paste_into_frames: out must be a contiguous uint8 [{n}, {h}, {w}, 3] tensor on {x.device}")
        if out.data_ptr() != x.data_ptr():
            out.copy_(x)
    if n:
        lib().call("e4s_warp_perspective_paste_u8", _p(out), _p(f), pboxes.data_ptr(), _p(ic), n, h, w, s, _stream())
    return out


# ------------------------------------------------------------------------------------ f3: multi-band blend
def pyr_down(x: torch.Tensor, round_u8: bool = False) -> torch.Tensor:
    """``cv2.pyrDown`` on ``[..., H, W]`` float planes (``round_u8``: the 8-bit variant's rounding, for a pyramid of a uint8 image)."""
    x = _c(x, "image")
    h, w = x.shape[-2:]
    out = torch.empty(x.shape[:-2] + ((h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=x.device)
    lib().call("e4s_pyr_down", _p(out), _p(x), x.numel() // (h * w), h, w, int(round_u8), _stream())
    return out


def pyr_up(x: torch.Tensor, minuend: Optional[torch.Tensor] = None, addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``cv2.pyrUp`` on ``[..., H, W]`` float planes -> ``[..., 2H, 2W]``; ``minuend - up(x)`` or ``up(x) + addend`` when given."""
    x = _c(x, "image")
    h, w = x.shape[-2:]
    out = torch.empty(x.shape[:-2] + (2 * h, 2 * w), dtype=torch.float32, device=x.device)
    for name, t in (("minuend", minuend), ("addend", addend)):
        if t is not None and (tuple(t.shape) != tuple(out.shape) or not t.is_contiguous() or t.dtype != torch.float32):
            raise ValueError(f"pyr_up: {name} must be a contiguous float32 tensor of the output shape {tuple(out.shape)}")
    lib().call("e4s_pyr_up", _p(out), _p(x), _p(minuend), _p(addend), x.numel() // (h * w), h, w, _stream())
    return out


def laplacian_blend(a_u8: torch.Tensor, b: torch.Tensor, mask: torch.Tensor, num_levels: int = 10) -> torch.Tensor:
    """``Laplacian_Pyramid_Blending_with_mask(A, B, m, num_levels)`` (swap_face_fine/multi_band_blending.py:5-48) on the device, with the
    types of its call site: ``a_u8`` uint8 ``[bs, 3, H, W]`` (its Gaussian pyramid is rounded to 8 bits per level like cv2's), ``b`` float
    ``[bs, 3, H, W]`` in [0, 255], ``mask`` float ``[bs, 1 or 3, H, W]``.  Returns the float blend ``[bs, 3, H, W]``."""
    if a_u8.dtype != torch.uint8 or a_u8.dim() != 4 or b.shape != a_u8.shape:
        raise ValueError("laplacian_blend: A is uint8 [bs, 3, H, W] and B a float tensor of the same shape")
    h, w = a_u8.shape[-2:]
    if (h >> num_levels) < 1 or (w >> num_levels) < 1 or h % (1 << (num_levels - 1)) or w % (1 << (num_levels - 1)):
        raise ValueError(f"laplacian_blend: {h}x{w} cannot carry {num_levels} pyramid levels (the reference runs 1024x1024 with 10)")
    ga, gb = a_u8.float().contiguous(), _c(b, "B")
    gm = _c(mask.expand(-1, 3, -1, -1) if mask.shape[1] == 1 else mask, "mask")
    gpa, gpb, gpm = [ga], [gb], [gm]
    for _ in range(num_levels - 1):              # (the reference's last pyrDown, level num_levels, is never used)
        ga, gb, gm = pyr_down(ga, True), pyr_down(gb), pyr_down(gm)
        gpa.append(ga); gpb.append(gb); gpm.append(gm)
    out = torch.lerp(gpb[-1], gpa[-1], gpm[-1])                                    # la*gm + lb*(1-gm) at the coarsest level
    for i in range(num_levels - 1, 0, -1):
        # Laplacian levels of A and B, their masked mix and the reconstruction step in one pass (10 -> 4 plane sets of traffic per level)
        hi, lo = gpa[i - 1], gpa[i]
        nxt = torch.empty_like(hi)
        lib().call("e4s_pyr_blend_level", _p(nxt), _p(out), _p(hi), _p(lo), _p(gpb[i - 1]), _p(gpb[i]), _p(gpm[i - 1]),
                   lo.numel() // (lo.shape[-2] * lo.shape[-1]), lo.shape[-2], lo.shape[-1], _stream())
        out = nxt
    return out


def blending(full_img_u8: torch.Tensor, ori_img: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """``blending(full_img, ori_img, mask)`` (multi_band_blending.py:51-74) for 1024 x 1024 frames (its resizes are then identities):
    uint8 ``[bs, 3, H, W]`` = the clipped, truncated ten-level blend."""
    if tuple(full_img_u8.shape[-2:]) != (1024, 1024):
        raise NotImplementedError("blending: the reference resizes to 1024x1024 first; pass 1024x1024 frames")
    return laplacian_blend(full_img_u8, ori_img, mask, 10).clamp_(0, 255).to(torch.uint8)


# ------------------------------------------------------------------------------------ f6: the image caller's soft paste masks and uint8 blends (softmask.hip)
_soft_weights = {}
_class_luts = {}
FACIAL_CLASSES = (1, 2, 3, 5, 6, 8, 9)        # Trick.get_facial_mask_from_seg19 (utils/paste_back_tricks.py:191): lips, brows, eyes, nose, skin, neck, teeth


def _soft_erosion_weights(kernel_size: int, device) -> torch.Tensor:
    """``SoftErosion.__init__``'s ``weight`` buffer (utils/paste_back_tricks.py:20-30), float32 on the host with its own expressions, transposed for
    the kernel.  Built once per (size, device), so that no host-to-device copy happens inside a hipGraph capture."""
    key = (int(kernel_size), str(device))
    wt = _soft_weights.get(key)
    if wt is None:
        r = kernel_size // 2
        yy, xx = torch.meshgrid(torch.arange(0., kernel_size), torch.arange(0., kernel_size), indexing="ij")
        dist = torch.sqrt((xx - r) ** 2 + (yy - r) ** 2)          # float32 throughout, like the module
        cone = dist.max() - dist
        cone /= cone.sum()
        wt = _soft_weights[key] = cone.t().contiguous().to(device)
    return wt


def _softer_checked(kernel_size, threshold, iterations):
    if not isinstance(kernel_size, int) or kernel_size % 2 != 1 or not 3 <= kernel_size <= 33:
        raise ValueError(f"soft_erosion: kernel_size is an odd integer in 3..33, got {kernel_size!r}")
    if not isinstance(iterations, int) or iterations < 1:
        raise ValueError(f"soft_erosion: iterations is an integer >= 1, got {iterations!r}")
    return int(kernel_size), float(threshold), int(iterations)


def soft_erosion(x: torch.Tensor, kernel_size: int = 15, threshold: float = 0.6, iterations: int = 1):
    """``SoftErosion(kernel_size, threshold, iterations)(x)`` (utils/paste_back_tricks.py:17-43; MegaFS) for float32 ``[bs, C, H, W]`` on the device,
    every plane on its own: ``iterations - 1`` times ``x = min(x, conv(x))`` with the cone-weighted ``kernel_size``² kernel, ``c = conv(x)``,
    ``hard = c >= threshold``, ``soft = 1`` where hard, else ``c / max(c over the plane's not-hard pixels)``.  Returns ``(soft, hard)``: float32 and
    bool ``[bs, C, H, W]``.  No host synchronisation (the reference's ``x[~mask].max()`` is one); capturable in a hipGraph.

    The reference normalises by the maximum over the whole tensor but is only ever called with ``[1, 1, H, W]``; per plane is the batch form of that.
    Two departures, both where the reference misbehaves: a plane in which EVERY pixel passes the threshold comes back as all ones (the reference
    raises on ``max()`` of an empty tensor), and a plane whose below-threshold maximum is 0 — an all-zero mask, no face — gives 0 at those pixels
    (the reference returns NaN from 0 / 0), so that a paste through such a mask leaves the target untouched."""
    k, thr, it = _softer_checked(kernel_size, threshold, iterations)
    x = _c(x, "x")
    if x.dim() != 4:
        raise ValueError(f"soft_erosion: expected a float32 [bs, C, H, W] tensor, got {tuple(x.shape)}")
    bs, ch, h, w = x.shape
    soft = torch.empty_like(x)
    hard = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if x.numel() == 0:
        return soft, hard.bool()
    wt = _soft_erosion_weights(k, x.device)
    nbytes = ctypes.c_int64(0)
    lib().call("e4s_soft_erosion_scratch_bytes", bs * ch, h, w, it, ctypes.byref(nbytes))
    scratch = torch.empty((nbytes.value // 4,), dtype=torch.float32, device=x.device)
    lib().call("e4s_soft_erosion", _p(soft), _p(hard), _p(x), _p(wt), _p(scratch), bs * ch, h, w, k, thr, it, _stream())
    return soft, hard.view(torch.bool)


def soft_paste_masks(swapped: torch.Tensor, hole_mask: Optional[torch.Tensor] = None, radius: int = 2, kernel_size: int = 15, threshold: float = 0.6,
                     iterations: int = 1):
    """The paste masks of the two-image caller: the foreground of ``_past_back`` (Face_swap_with_two_imgs.py:178-182: everything but background /
    ear-ring / hair / ear / neck, the hole forced to foreground) through ``_create_masks(..., 'expansion', radius)`` (:784-792), whose masks all pass
    through ``SoftErosion``: ``full = soft(dilate)``, ``border = clip(full - soft(erode), 0, 1)``, ``content = soft(foreground)``.
    ``swapped`` / ``hole_mask``: uint8 ``[bs, H, W]``.  Returns float32 ``[bs, 1, H, W]`` ``(content, border, full)``; the three planes of a face are
    softened in one ``soft_erosion`` call."""
    _softer_checked(kernel_size, threshold, iterations)
    fg, hard_border, hard_full = foreground_masks(swapped, hole_mask, radius)
    if fg.shape[0] == 0:
        return fg, hard_border, hard_full
    planes = torch.cat([hard_full, hard_full - hard_border, fg], dim=1)          # (dilated, eroded, foreground): binary, so eroded = full - border exactly
    s, _ = soft_erosion(planes, kernel_size, threshold, iterations)
    full = s[:, 0:1]
    return s[:, 2:3].contiguous(), (full - s[:, 1:2]).clamp_(0, 1), full.contiguous()


def _class_lut(classes, device) -> torch.Tensor:
    key = (tuple(classes), str(device))
    lut = _class_luts.get(key)
    if lut is None:
        t = torch.zeros(256, dtype=torch.float32)
        t[list(classes)] = 1.0
        lut = _class_luts[key] = t.to(device)
    return lut


def facial_mask12(labels: torch.Tensor, size=None, **softer) -> torch.Tensor:
    """``Trick.get_facial_mask_from_seg19(labels, size, SoftErosion(**softer))`` (utils/paste_back_tricks.py:173-200) for uint8 ``[bs, H, W]`` 12-class
    maps: 1 on lips, brows, eyes, nose, skin, neck and teeth, bilinear resize to ``size = (H', W')`` with ``align_corners=True``, then
    ``soft_erosion`` (its defaults are the image caller's ``mask_softer``).  Returns float32 ``[bs, 1, H', W']``."""
    unknown = set(softer) - {"kernel_size", "threshold", "iterations"}
    if unknown:
        raise TypeError(f"facial_mask12: unexpected arguments {sorted(unknown)}")
    _softer_checked(softer.get("kernel_size", 15), softer.get("threshold", 0.6), softer.get("iterations", 1))
    m = _labels_u8(labels, "labels")
    mask = _class_lut(FACIAL_CLASSES, m.device)[m.long()][:, None]
    if size is not None:
        size = (int(size[0]), int(size[1]))
        if mask.shape[0] and tuple(mask.shape[-2:]) != size:
            from .ops_encode import bilinear_resize
            mask = bilinear_resize(mask, size, align_corners=True)
        elif not mask.shape[0]:
            mask = mask.new_empty((0, 1) + size)
    return soft_erosion(mask, **softer)[0]


def blend_with_mask(bottom_u8: torch.Tensor, up_u8: torch.Tensor, mask: torch.Tensor, up_ratio: float = 1.0) -> torch.Tensor:
    """``Trick.blending_two_images_with_mask(bottom, up, up_ratio, mask)`` (utils/paste_back_tricks.py:131-147) for uint8 ``[n, H, W, 3]`` frames and a
    float32 ``[n, 1 or 3, H, W]`` mask, bit for bit with numpy: NaN in the mask counts as 0, ``m = mask * up_ratio``, ``trunc(bottom * (1 - m) + up * m)``
    in float32 (clamped to [0, 255] first: the same wherever the reference is defined).  ``bottom = T, up = swapped, up_ratio = 1`` is the crop paste
    ``np.uint8(swapped * content + T * (1 - content))`` of Face_swap_with_two_imgs.py:216-217."""
    b = _frames_u8(bottom_u8, "bottom")
    u = _frames_u8(up_u8, "up", b.shape)
    m = _c(mask, "mask")
    n, h, w, _ = b.shape
    if m.dim() != 4 or m.shape[0] != n or m.shape[1] not in (1, 3) or tuple(m.shape[2:]) != (h, w):
        raise ValueError(f"blend_with_mask: expected a float32 [{n}, 1 or 3, {h}, {w}] mask, got {tuple(m.shape)}")
    if not 0.0 <= float(up_ratio) <= 1.0:
        raise ValueError(f"blend_with_mask: up_ratio {up_ratio} is not in [0, 1]")
    out = torch.empty_like(b)
    if n:
        lib().call("e4s_blend_u8", _p(out), _p(b), _p(u), _p(m), float(up_ratio), n, h, w, m.shape[1], _stream())
    return out


# ------------------------------------------------------------------------------------ f7: the image caller's skin colour transfer (colortransfer.hip)
CT_MODES = ("lct", "mkl")
# every other ct_mode of the reference needs code this project cannot pin: cv2 colour conversions / bilateral filter, random rotations, a network
CT_MODES_UNSUPPORTED = ("rct", "mix", "sot", "idt", "adaptive", "blender")
GREY_MORPH_MAX_RADIUS = 16
_CT_CHUNK = 4096


def _radius_checked(radius, name):
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius <= GREY_MORPH_MAX_RADIUS:
        raise ValueError(f"{name}: radius is an integer in 0..{GREY_MORPH_MAX_RADIUS}, got {radius!r}")
    return radius


def _ct_mode_checked(ct_mode, name):
    if ct_mode not in CT_MODES:
        why = " (it needs cv2, random rotations or a network: not on the device)" if ct_mode in CT_MODES_UNSUPPORTED else ""
        raise ValueError(f"{name}: ct_mode is one of {list(CT_MODES)}, got {ct_mode!r}{why}")
    return CT_MODES.index(ct_mode)


def _grey_morph(x: torch.Tensor, radius: int, op: int, name: str) -> torch.Tensor:
    _radius_checked(radius, name)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: x must be a torch.Tensor")
    if x.dtype != torch.float32 or x.dim() < 2:
        raise ValueError(f"{name}: expected float32 [..., H, W] planes, got {x.dtype} {tuple(x.shape)}")
    x = _c(x, "x")
    h, w = x.shape[-2:]
    out = torch.empty_like(x)
    if x.numel():
        lib().call("e4s_grey_morph", _p(out), _p(x), x.numel() // (h * w), h, w, radius, op, _stream())
    return out


def grey_dilate(x: torch.Tensor, radius: int) -> torch.Tensor:
    """``dilation(x, ones(2r+1, 2r+1), engine='convolution')`` (utils/morphology.py:23-108) on float32 ``[..., H, W]`` planes: the flat maximum filter
    with the 'geodesic' border (pixels outside the image are ignored), exact.  ``radius`` 0 .. 16; 0 is a copy."""
    return _grey_morph(x, radius, 0, "grey_dilate")


def grey_erode(x: torch.Tensor, radius: int) -> torch.Tensor:
    """``erosion(x, ones(2r+1, 2r+1), engine='convolution')`` (utils/morphology.py:111-198): the flat minimum filter, as ``grey_dilate``."""
    return _grey_morph(x, radius, 1, "grey_erode")


def soft_expansion_masks(mask: torch.Tensor, radius: int, kernel_size: int = 15, threshold: float = 0.6, iterations: int = 1):
    """``_create_masks(mask, 'expansion', radius)`` (Face_swap_with_two_imgs.py:784-792) for a FLOAT mask ``[bs, 1, H, W]`` (``soft_paste_masks`` is the
    same for a label map): ``full = soft(dilate(mask))``, ``border = clip(full - soft(erode(mask)), 0, 1)``, ``content = soft(mask)``, the three planes
    of a face softened in one ``soft_erosion`` call.  Returns float32 ``[bs, 1, H, W]`` ``(content, border, full)``."""
    _radius_checked(radius, "soft_expansion_masks")
    _softer_checked(kernel_size, threshold, iterations)
    if not isinstance(mask, torch.Tensor):
        raise TypeError("soft_expansion_masks: mask must be a torch.Tensor")
    if mask.dtype != torch.float32 or mask.dim() != 4 or mask.shape[1] != 1:
        raise ValueError(f"soft_expansion_masks: expected a float32 [bs, 1, H, W] mask, got {mask.dtype} {tuple(mask.shape)}")
    m = _c(mask, "mask")
    if m.shape[0] == 0:
        return m, torch.empty_like(m), torch.empty_like(m)
    planes = torch.cat([grey_dilate(m, radius), grey_erode(m, radius), m], dim=1)
    s, _ = soft_erosion(planes, kernel_size, threshold, iterations)
    full = s[:, 0:1]
    return s[:, 2:3].contiguous(), (full - s[:, 1:2]).clamp_(0, 1), full.contiguous()


def _ct_inputs(name, src_u8, trg_u8, src_mask, trg_mask):
    for nm, t in (("src", src_u8), ("trg", trg_u8)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {nm} must be a torch.Tensor")
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError(f"{name}: {nm}: expected uint8 [bs, H, W, 3] frames, got {t.dtype} {tuple(t.shape)}")
    if src_u8.shape != trg_u8.shape:
        raise ValueError(f"{name}: src {tuple(src_u8.shape)} and trg {tuple(trg_u8.shape)} frames differ in shape")
    bs, h, w, _ = src_u8.shape
    for nm, t in (("src_mask", src_mask), ("trg_mask", trg_mask)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {nm} must be a torch.Tensor")
        if t.dtype != torch.float32 or tuple(t.shape) != (bs, 1, h, w):
            raise ValueError(f"{name}: {nm}: expected a float32 [{bs}, 1, {h}, {w}] mask, got {t.dtype} {tuple(t.shape)}")
    for nm, t in (("src", src_u8), ("trg", trg_u8), ("src_mask", src_mask), ("trg_mask", trg_mask)):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {nm} must be a CUDA tensor")
    return src_u8.contiguous(), trg_u8.contiguous(), src_mask.contiguous(), trg_mask.contiguous()


def color_transfer_coefficients(src_u8: torch.Tensor, trg_u8: torch.Tensor, src_mask: torch.Tensor, trg_mask: torch.Tensor, ct_mode: str) -> torch.Tensor:
    """The linear map of ``skin_color_transfer``: float64 ``[bs, 15]`` = ``(A [3, 3] row-major, mu_src [3], mu_trg [3])`` with
    ``y = A (v - mu_src) + mu_trg`` for ``v = (u8 * mask) / 255``.  The statistics run over ALL pixels of each image, like the reference's; they are summed
    in float64 in a fixed order (bitwise reproducible) and never leave the device."""
    mode = _ct_mode_checked(ct_mode, "color_transfer_coefficients")
    s, t, sm, tm = _ct_inputs("color_transfer_coefficients", src_u8, trg_u8, src_mask, trg_mask)
    bs, h, w, _ = s.shape
    coef = torch.empty((bs, 15), dtype=torch.float64, device=s.device)
    if bs == 0:
        return coef
    nbytes = ctypes.c_int64(0)
    lib().call("e4s_ct_moments_scratch_bytes", bs, h, w, ctypes.byref(nbytes))
    part = torch.empty((2, nbytes.value // 8), dtype=torch.float64, device=s.device)
    lib().call("e4s_ct_moments", _p(part[0]), _p(s), _p(sm), bs, h, w, _stream())
    lib().call("e4s_ct_moments", _p(part[1]), _p(t), _p(tm), bs, h, w, _stream())
    lib().call("e4s_ct_solve", _p(coef), _p(part[0]), _p(part[1]), bs, h, w, mode, _stream())
    return coef


def skin_color_transfer(src_u8: torch.Tensor, trg_u8: torch.Tensor, src_mask: torch.Tensor, trg_mask: torch.Tensor, ct_mode: str = "lct",
                        with_q: bool = True):
    """Steps 3 - 6a of ``_color_transfer``'s arithmetic branch (Face_swap_with_two_imgs.py:555-568) for ``ct_mode`` 'lct' (``linear_color_transfer``,
    mode 'pca', swap_face_fine/color_transfer.py:345-381) or 'mkl' (``color_transfer_mkl``, :218-246) on the device:

        src = (D * src_mask) / 255, trg = (T * trg_mask) / 255;   q = uint8(skin_color_transfer(src, trg, ct_mode))      (truncated)
        composed = D * (1 - src_mask) + q * src_mask                                                                     (numpy's float32 arithmetic)

    ``src_u8`` (D, the swapped face) / ``trg_u8`` (T): uint8 ``[bs, H, W, 3]``; the masks float32 ``[bs, 1, H, W]``.  Returns ``(composed, q)``: float32
    ``[bs, 3, H, W]`` (the layout ``blending`` takes) and uint8 ``[bs, H, W, 3]`` (None with ``with_q=False``).  The other modes of the reference go through
    cv2, random rotations or a network and raise ``ValueError``."""
    _ct_mode_checked(ct_mode, "skin_color_transfer")
    s, t, sm, tm = _ct_inputs("skin_color_transfer", src_u8, trg_u8, src_mask, trg_mask)
    bs, h, w, _ = s.shape
    composed = torch.empty((bs, 3, h, w), dtype=torch.float32, device=s.device)
    q = torch.empty_like(s) if with_q else None
    if bs == 0:
        return composed, q
    coef = color_transfer_coefficients(s, t, sm, tm, ct_mode)
    lib().call("e4s_ct_apply", _p(composed), _p(q), _p(s), _p(sm), _p(coef), bs, h, w, _stream())
    return composed, q


__all__ = ['CT_MODES', 'CT_MODES_UNSUPPORTED', 'GREY_MORPH_MAX_RADIUS', 'grey_dilate', 'grey_erode', 'soft_expansion_masks', 'color_transfer_coefficients',
           'skin_color_transfer', '_labels_u8','swap_head_mask', 'foreground_masks', 'frames_to_tensor', 'PTI_BG_CLASSES', 'erode_labels', '_pil_tables', '_pil_resample_tables', '_pil_bicubic_tables', '_pil_lanczos_tables', 'pil_resize', 'crop_align', 'paste_into_frames', 'pyr_down', 'pyr_up', 'laplacian_blend', 'blending',
           'FACIAL_CLASSES', 'soft_erosion', 'soft_paste_masks', 'facial_mask12', 'blend_with_mask']
