"""CPU restatement (numpy, float64 statistics) of the two-image caller's skin colour transfer for ``ct_mode`` 'lct' / 'mkl', the model the GPU tests of
``csrc/colortransfer.hip``, ``ops.grey_dilate`` ... ``pipeline.color_transfer`` compare against.  ``tests/test_colortransfer_cpu.py`` pins it against
outputs of the reference's own ``utils.morphology`` and ``swap_face_fine.color_transfer`` (``tests/golden/g19_color_transfer.npz``).  It composes the
pieces that are pinned already: ``softpaste_model``'s SoftErosion and the oracle's flat morphology and multi-band blend.  Nothing under ``e4s2024_amd/``
imports this module.

Reference: Face_swap_with_two_imgs.py:537-572 (_color_transfer), :784-792 (_create_masks); swap_face_fine/color_transfer.py:218-246 (color_transfer_mkl),
:345-381 (linear_color_transfer), :538-561 (skin_color_transfer); utils/morphology.py:23-198.

Where the reference and this model differ: the reference takes its means (and, for lct, its covariances) in float32 before it goes on in float64; the
model is float64 from the float32 pixel values on.  ``test_colortransfer_cpu.py`` bounds what that costs in bytes."""
import numpy as np
import torch
import torch.nn.functional as F

import softpaste_model as SP
from oracle import e4s_oracle as O

CT_FACE_CLASSES = (1, 2, 3, 5, 6, 9, 7, 8)
MODES = ("lct", "mkl")
MORPH_SHAPES = (((1, 1, 7, 5), (10,)), ((2, 1, 33, 1), (2,)), ((1, 2, 1, 90), (10,)), ((1, 1, 96, 80), (0, 1, 2, 10)))
CT_SIZE = 192
CT_PAIRS = 3


# ------------------------------------------------------------------------------------------------ seeded inputs (shared by the fixture generator and the tests)
def morph_input(shape, seed=None) -> np.ndarray:
    """float32 ``shape`` = [bs, C, H, W] in [0, 1]: flat regions of exact 0 and exact 1 with soft random edges between."""
    rs = np.random.RandomState(sum(shape) * 7 + 19 if seed is None else seed)
    x = rs.rand(*shape).astype(np.float32)
    sel = rs.rand(*shape)
    x[sel < 0.3] = 0.0
    x[sel > 0.7] = 1.0
    h, w = shape[-2:]
    if h >= 24 and w >= 24:                     # a solid block of ones and one of zeros: larger than a radius-10 window only where there is room
        x[..., h // 8: h // 8 + 30, w // 8: w // 8 + 30] = 1.0
        x[..., h // 2: h // 2 + 30, w // 2: w // 2 + 30] = 0.0
    return x


def soft_mask(size: int, seed: int) -> np.ndarray:
    """float32 ``[1, 1, size, size]``: a face-like ellipse with eye / mouth holes, resized from ``size // 2`` with bilinear (align_corners=False): exact
    0 and 1 inside and outside, soft edges."""
    rs = np.random.RandomState(seed)
    n = size // 2
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    cy, cx = n * (0.5 + 0.06 * rs.randn()), n * (0.5 + 0.06 * rs.randn())
    m = ((yy - cy) / (0.38 * n)) ** 2 + ((xx - cx) / (0.30 * n)) ** 2 <= 1.0
    m &= ((yy - cy + 0.1 * n) / (0.04 * n)) ** 2 + ((np.abs(xx - cx) - 0.12 * n) / (0.07 * n)) ** 2 > 1.0
    t = torch.from_numpy(m.astype(np.float32))[None, None]
    return F.interpolate(t, size=(size, size), mode="bilinear", align_corners=False).numpy()


def ct_pair(index: int, size: int = CT_SIZE):
    """Seeded pair ``index`` -> ``(D, T, md, mt)``: uint8 ``[size, size, 3]`` smooth three-channel colour fields plus noise, float32 ``[size, size, 1]`` masks
    (pair 0: elliptical, binary; pair 1: bilinear-softened; pair 2: one of each)."""
    rs = np.random.RandomState(1900 + index)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size

    def image():
        base = rs.uniform(0.25, 0.75, 3)
        gx, gy = rs.uniform(-0.35, 0.35, 3), rs.uniform(-0.35, 0.35, 3)
        ph = rs.uniform(0, 2 * np.pi, 3)
        field = base + gx * (xx[..., None] - 0.5) + gy * (yy[..., None] - 0.5) + 0.12 * np.sin(2 * np.pi * (xx + 1.3 * yy)[..., None] * rs.uniform(0.5, 2.0, 3) + ph)
        noise = 0.14 * rs.randn(size, size, 3)
        return np.clip(np.round((field + noise) * 255), 0, 255).astype(np.uint8)

    def mask(soft, seed):
        if soft:
            return soft_mask(size, seed)[0, 0, :, :, None]
        cy, cx = 0.5 + 0.05 * rs.randn(), 0.5 + 0.05 * rs.randn()
        return ((((yy - cy) / 0.40) ** 2 + ((xx - cx) / 0.31) ** 2) <= 1.0).astype(np.float32)[..., None]

    d, t = image(), image()
    soft_d, soft_t = ((False, False), (True, True), (True, False))[index]
    return d, t, mask(soft_d, 40 + index), mask(soft_t, 50 + index)


# ------------------------------------------------------------------------------------------------ the pieces
def _flat_morph(x: np.ndarray, radius: int, op) -> np.ndarray:
    """Flat (2r+1)^2 maximum / minimum with the 'geodesic' border, one axis after the other (a maximum of maxima: exact, and 2 (2r+1) passes over the
    plane where the oracle's ``_flat_morph`` makes (2r+1)^2; ``test_colortransfer_cpu.py`` holds the two against each other and against the reference)."""
    out = np.asarray(x, dtype=np.float32)
    pad_val = -np.inf if op is np.maximum else np.inf
    for axis in (-1, -2):
        n = out.shape[axis]
        pad = [(0, 0)] * out.ndim
        pad[axis] = (radius, radius)
        p = np.pad(out, pad, constant_values=pad_val)
        acc = np.full_like(out, pad_val)
        for d in range(2 * radius + 1):
            acc = op(acc, np.take(p, np.arange(d, d + n), axis=axis))
        out = acc
    return out


def grey_dilate(x: np.ndarray, radius: int) -> np.ndarray:
    """``dilation(x, ones(2r+1, 2r+1), engine='convolution')``: the flat maximum filter, pixels outside the image ignored."""
    return _flat_morph(x, radius, np.maximum)


def grey_erode(x: np.ndarray, radius: int) -> np.ndarray:
    return _flat_morph(x, radius, np.minimum)


def soft_expansion_masks(mask: np.ndarray, radius: int, kernel_size=15, threshold=0.6, iterations=1, dtype=torch.float32):
    """``_create_masks(mask, 'expansion', radius)`` (:784-792) for a float ``[bs, 1, H, W]`` mask -> ``(content, border, full)``."""
    mask = np.asarray(mask, dtype=np.float32)
    s, _ = SP.soft_erosion(np.concatenate([grey_dilate(mask, radius), grey_erode(mask, radius), mask], axis=1), kernel_size, threshold, iterations, dtype)
    return s[:, 2:3], np.clip(s[:, 0:1] - s[:, 1:2], 0, 1), s[:, 0:1]


def face_masks(labels: np.ndarray, hw) -> np.ndarray:
    """:540-547: the face classes of uint8 ``[bs, h, w]`` maps, bilinear to ``hw`` (align_corners=False) -> float32 ``[bs, 1, H, W]``."""
    m = torch.from_numpy(np.isin(np.asarray(labels), CT_FACE_CLASSES).astype(np.float32))[:, None]
    return F.interpolate(m, size=tuple(hw), mode="bilinear", align_corners=False).numpy()


def inner(img_u8: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """:555-564: ``np.array(D * mask) / 255.`` — a float32 product, then a float32 true division.  ``img_u8`` [..., H, W, 3], ``mask`` [..., H, W, 1]."""
    v = (img_u8 * np.asarray(mask, dtype=np.float32)) / 255.
    assert v.dtype == np.float32
    return v


def _sqrtm_sym(c: np.ndarray, floor: float):
    lam, v = np.linalg.eigh((c + c.T) / 2)
    d = np.sqrt(np.clip(lam, floor, None))
    return v, d


def coefficients(src: np.ndarray, trg: np.ndarray, mode: str):
    """``(A, mu_src, mu_trg)`` in float64 with ``y = A (v - mu_src) + mu_trg``, from the float32 inner images ``[H, W, 3]``; the statistics run over all
    pixels."""
    x0, x1 = src.reshape(-1, 3).astype(np.float64), trg.reshape(-1, 3).astype(np.float64)
    mu0, mu1 = x0.mean(axis=0), x1.mean(axis=0)
    n = x0.shape[0]
    c0, c1 = (x0 - mu0).T @ (x0 - mu0), (x1 - mu1).T @ (x1 - mu1)
    if mode == "lct":            # linear_color_transfer(src, trg, 'pca'): Qs inv(Qt) with "t" the image that is changed
        vt, dt = _sqrtm_sym(c0 / n + 1e-5 * np.eye(3), 0.0)
        vs, ds = _sqrtm_sym(c1 / x1.shape[0] + 1e-5 * np.eye(3), 0.0)
        a = (vs * ds) @ vs.T @ ((vt / dt) @ vt.T)
    elif mode == "mkl":          # color_transfer_mkl: result = (x0 - mx0) t + mx1, so A = t^T
        eps = np.finfo(float).eps
        ua, da = _sqrtm_sym(c0 / max(n - 1, 1), eps)
        b = c1 / max(x1.shape[0] - 1, 1)
        uc, dc = _sqrtm_sym((da[:, None] * (ua.T @ b @ ua)) * da[None, :], eps)
        left = ua / da
        t = left @ ((uc * dc) @ uc.T) @ left.T
        a = t.T
    else:
        raise ValueError(f"unknown ct_mode {mode}")
    return a, mu0, mu1


def transfer(src: np.ndarray, trg: np.ndarray, mode: str) -> np.ndarray:
    """``skin_color_transfer(src, trg, mode)`` without its final ``* 255``: float32 ``[H, W, 3]`` in [0, 1]."""
    a, mu0, mu1 = coefficients(src, trg, mode)
    y = (src.reshape(-1, 3).astype(np.float64) - mu0) @ a.T + mu1
    return np.clip(y.reshape(src.shape).astype(np.float32), 0, 1)


def quantise(y: np.ndarray) -> np.ndarray:
    """:563-565 with color_transfer.py:561: ``np.uint8(y * 255)`` — a float32 product, truncated."""
    v = y * 255
    assert v.dtype == np.float32
    return np.uint8(v)


def compose(d_u8: np.ndarray, q_u8: np.ndarray, md: np.ndarray) -> np.ndarray:
    """:568: ``D * (1 - mask) + inner * mask`` in float32."""
    md = np.asarray(md, dtype=np.float32)
    v = d_u8 * (1 - md) + q_u8 * md
    assert v.dtype == np.float32
    return v


def skin_color_transfer(d_u8, t_u8, md, mt, mode):
    """One image: uint8 ``[H, W, 3]`` frames, float32 ``[H, W, 1]`` masks -> ``(composed float32 [H, W, 3], q uint8 [H, W, 3])``."""
    q = quantise(transfer(inner(d_u8, md), inner(t_u8, mt), mode))
    return compose(d_u8, q, md), q


def color_transfer(d_u8, t_u8, labels_d, labels_t, mode="lct", radius=10) -> np.ndarray:
    """Steps 1 - 6 for a batch: uint8 ``[bs, 1024, 1024, 3]`` frames and uint8 ``[bs, h, w]`` maps -> uint8 ``[bs, 1024, 1024, 3]``."""
    h, w = d_u8.shape[1:3]
    md, mt = face_masks(labels_d, (h, w)), face_masks(labels_t, (h, w))
    border = soft_expansion_masks(md, radius)[1]
    out = []
    for b in range(d_u8.shape[0]):
        composed, _ = skin_color_transfer(d_u8[b], t_u8[b], md[b, 0, :, :, None], mt[b, 0, :, :, None], mode)
        out.append(O.blending(d_u8[b], composed, border[b, 0, :, :, None].repeat(3, -1)))
    return np.stack(out)
