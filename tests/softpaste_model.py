"""CPU restatement (numpy / torch) of the two-image caller's paste-back, the model the GPU tests of ``csrc/softmask.hip``, ``ops.soft_erosion`` ...
``pipeline.swap_images`` compare against.  ``tests/test_softpaste_cpu.py`` pins it against outputs of the reference's own ``SoftErosion``, ``Trick`` and
``utils.morphology`` (``tests/golden/g18_soft_paste.npz``).  Nothing under ``e4s2024_amd/`` imports this module.

Reference: utils/paste_back_tricks.py:17-43 (SoftErosion), :131-147 (blending_two_images_with_mask), :173-200 (get_facial_mask_from_seg19);
Face_swap_with_two_imgs.py:159-219 (_past_back), :416-453 (_swap_comp_style_vector), :469-472 (component sets), :775-794 (_create_masks), :909-924."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import e4s_oracle as O

FACIAL_CLASSES = (1, 2, 3, 5, 6, 8, 9)
IMAGE_COMP_INDICES = tuple(sorted(set(range(12)) - {0, 10, 4, 11}))
IMAGE_COMP_INDICES_CT = tuple(sorted(set(range(12)) - {0, 10, 4, 8, 7, 11}))


def soft_erosion_weights(kernel_size: int) -> torch.Tensor:
    """The constructor's ``weight`` buffer ``[k, k]``, in float32 like the constructor whatever the convolution's precision."""
    r = kernel_size // 2
    yy, xx = torch.meshgrid(torch.arange(0., kernel_size), torch.arange(0., kernel_size), indexing="ij")
    dist = torch.sqrt((xx - r) ** 2 + (yy - r) ** 2)
    cone = dist.max() - dist
    cone /= cone.sum()
    return cone


def soft_erosion_conv(x, kernel_size=15, iterations=1, dtype=torch.float32) -> torch.Tensor:
    """The convolution value ``c`` the threshold is applied to: ``[bs, C, H, W]`` in ``dtype``.  float32 is the reference's own ``F.conv2d``; any other
    precision sums the k^2 shifted planes (ATen's float64 convolution unfolds k^2 copies of the image)."""
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    ch = x.shape[1]
    w2 = soft_erosion_weights(kernel_size).to(dtype)
    pad = kernel_size // 2

    def conv(t):
        if dtype == torch.float32:
            return F.conv2d(t, weight=w2[None, None].expand(ch, 1, -1, -1).contiguous(), groups=ch, padding=pad)
        h, w = t.shape[-2:]
        tp = F.pad(t, (pad, pad, pad, pad))
        acc = torch.zeros_like(t)
        for ky in range(kernel_size):
            for kx in range(kernel_size):
                acc.add_(tp[..., ky:ky + h, kx:kx + w], alpha=float(w2[ky, kx]))
        return acc

    for _ in range(iterations - 1):
        x = torch.min(x, conv(x))
    return conv(x)


def soft_erosion(x, kernel_size=15, threshold=0.6, iterations=1, dtype=torch.float32):
    """``SoftErosion(kernel_size, threshold, iterations)(x)`` with the maximum taken per plane -> ``(soft [bs, C, H, W] in dtype, hard bool)`` as
    numpy arrays.  Where the reference misbehaves: an all-pass plane is all ones (reference: ``max()`` of an empty tensor raises), a plane whose
    below-threshold maximum is 0 gives 0 there (reference: NaN)."""
    c = soft_erosion_conv(x, kernel_size, iterations, dtype)
    hard = c >= threshold
    soft = c.clone()
    for b in range(c.shape[0]):
        for k in range(c.shape[1]):
            p, m = soft[b, k], hard[b, k]
            p[m] = 1.0
            if (~m).any():
                mx = p[~m].max()
                p[~m] = p[~m] / mx if mx != 0 else 0.0
    return soft.numpy(), hard.numpy()


def hard_paste_masks(swapped: np.ndarray, hole, radius: int):
    """(foreground, dilated, eroded) float32 ``[bs, 1, H, W]``: the foreground of _past_back:178-182 and its flat (2r+1)^2 dilation / erosion."""
    swapped = np.asarray(swapped)
    hole = np.zeros(swapped.shape, bool) if hole is None else np.asarray(hole).astype(bool)
    fg = O.foreground_mask(swapped, hole)[:, None]
    _, border, full = O.create_masks_expansion(fg, radius)
    return fg, full, full - border


def soft_paste_masks(swapped, hole=None, radius=2, kernel_size=15, threshold=0.6, iterations=1, dtype=torch.float32):
    """``_create_masks(foreground, 'expansion', radius)`` (:784-792) -> ``(content, border, full)`` ``[bs, 1, H, W]``."""
    fg, dil, ero = hard_paste_masks(swapped, hole, radius)
    s, _ = soft_erosion(np.concatenate([dil, ero, fg], axis=1), kernel_size, threshold, iterations, dtype)
    return s[:, 2:3], np.clip(s[:, 0:1] - s[:, 1:2], 0, 1), s[:, 0:1]


def facial_mask12_hard(labels, size=None) -> torch.Tensor:
    """The mask of get_facial_mask_from_seg19 before its softer: float32 ``[bs, 1, H', W']`` (ATen's own bilinear, align_corners=True)."""
    m = torch.from_numpy(np.isin(np.asarray(labels), FACIAL_CLASSES).astype(np.float32))[:, None]
    if size is not None:
        m = F.interpolate(m, size=tuple(size), mode="bilinear", align_corners=True)
    return m


def facial_mask12(labels, size=None, dtype=torch.float32, **softer) -> np.ndarray:
    return soft_erosion(facial_mask12_hard(labels, size), dtype=dtype, **softer)[0]


def blend_with_mask(bottom_u8: np.ndarray, up_u8: np.ndarray, mask: np.ndarray, up_ratio: float = 1.0) -> np.ndarray:
    """``blending_two_images_with_mask`` on uint8 ``[n, H, W, 3]`` with a float32 ``[n, 1 or 3, H, W]`` mask, in numpy's float32 arithmetic."""
    m = np.moveaxis(np.array(mask, dtype=np.float32), 1, -1)
    m[np.isnan(m)] = 0.
    m *= np.float32(up_ratio)
    v = bottom_u8 * (1 - m) + up_u8 * m
    assert v.dtype == np.float32
    return np.clip(v, 0, 255).astype(np.uint8)


def mix_style_vectors_image(target: torch.Tensor, driven: torch.Tensor, comp_indices, below_face_interpolation=False) -> torch.Tensor:
    """``_swap_comp_style_vector`` (Face_swap_with_two_imgs.py:416-453), sample by sample (the teeth rule sums over ``[:, 9, :]`` of a batch of 1)."""
    out = target.clone()
    for b in range(target.shape[0]):
        for c in comp_indices:
            out[b, c] = driven[b, c]
        out[b, 11] = target[b, 11]
        if below_face_interpolation:
            out[b, 8] = (target[b, 8] + driven[b, 8]) / 2
        if torch.sum(driven[b, 9]) == 0:
            out[b, 9] = target[b, 9]
    return out


def _resize(m: np.ndarray, hw) -> np.ndarray:
    return F.interpolate(torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)), tuple(hw), mode="bilinear", align_corners=False).numpy()


def paste_back_soft(swapped_u8: np.ndarray, target_u8: np.ndarray, labels, hole=None, radius=2, masks=None) -> np.ndarray:
    """``_past_back`` up to :219: soft masks -> resize -> truncating paste -> the oracle's multi-band blend.  ``masks``: (content, border) to use
    instead of this module's own (to separate the blend's deviation from the masks')."""
    content, border = masks if masks is not None else soft_paste_masks(labels, hole, radius)[:2]
    h, w = swapped_u8.shape[1:3]
    cm, bm = _resize(content, (h, w)), _resize(border, (h, w))
    pasted = blend_with_mask(target_u8, swapped_u8, cm, 1.0)
    return np.stack([O.blending(target_u8[b], pasted[b], bm[b, 0, :, :, None].repeat(3, -1)) for b in range(swapped_u8.shape[0])])


def color_blend(swapped_u8, recolored_u8, labels, edge=None, up_ratio=0.75) -> np.ndarray:
    h, w = swapped_u8.shape[1:3]
    mask = facial_mask12(labels, (h, w))
    if edge is not None:
        mask = np.clip(mask - np.asarray(edge, dtype=np.float32).reshape(mask.shape), 0., 1.)
    return blend_with_mask(swapped_u8, recolored_u8, mask, up_ratio)
