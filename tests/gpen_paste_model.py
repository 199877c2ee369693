"""Row f15: what ``FaceEnhancement.process(aligned=False)`` (swap_face_fine/gpen/face_enhancement.py:68-108) does between its three networks, restated in
numpy.  cv2 and skimage are installed nowhere this project is built or tested, so every cv2 call is written here from OpenCV's algorithm — integer arithmetic
for uint8 images, float64 or float32 as stated otherwise — and the reference's own ``process`` is run over these functions as its ``cv2``
(tests/golden/make_golden_gpen_paste.py).  csrc/gpen_paste.hip follows this file.

    reference_points(S)      get_reference_facial_points((S, S), 0.25, (0, 0), True) in float64
    transforms(...)          the 5-point similarity pair of warp_and_crop_face ('smilarity') in float64 closed form, and the face flags
    warp_affine(...)         cv2.warpAffine(src, M, (w, h), flags=3): bilinear on the 1/32 grid of the fixed-point map, constant-0 border; uint8 and float32
    filter2d_smooth(...)     cv2.filter2D(ef, -1, [[1,2,1],[2,4,2],[1,2,1]] / 16) on uint8, BORDER_REFLECT_101
    gaussian_taps / gaussian_blur / mask_postprocess
    convert_scale_abs(...)   cv2.convertScaleAbs of a float32 image
    process(...)             the loop and the blend of FaceEnhancement.process over those functions

``MUT`` switches one step to a wrong variant each; tests/test_gpen_paste_cpu.py checks that every one of them moves a stored output."""
import numpy as np

REFERENCE_FACIAL_POINTS = [[30.29459953, 51.69630051], [65.53179932, 51.50139999], [48.02519989, 71.73660278], [33.54930115, 92.3655014],
                           [62.72990036, 92.20410156]]
FACE_SKIP, FACE_SMALL = 1, 2
MUTANTS = ("blur_once", "border_kept", "reflect", "no_round_offset", "truncate", "ge", "reverse", "half_up", "small_max", "not_inverted")
MUT = set()                                  # the active mutants (tests only)
f32 = np.float32


def reference_points(S):
    """[5, 2] float64: the square default (x + 8), the inner padding of 0.25 (+ 28 on a 168 crop), the resize by S / 168."""
    pts = np.array(REFERENCE_FACIAL_POINTS)
    pts += np.array([16, 0]) / 2
    pts += np.array([112, 112]) * 0.25 * 2 / 2
    return pts * (f32(S) / np.int64(168))


def flags_of(dets, threshold, small_face):
    """int32 [n] from ``dets [n, 5]`` (x1, y1, x2, y2, score), float32 throughout: FACE_SKIP if score < threshold, FACE_SMALL if min(h, w) < small_face."""
    d = np.asarray(dets, f32).reshape(-1, 5)
    side = np.maximum(d[:, 3] - d[:, 1], d[:, 2] - d[:, 0]) if "small_max" in MUT else np.minimum(d[:, 3] - d[:, 1], d[:, 2] - d[:, 0])
    return ((d[:, 4] < f32(threshold)) * FACE_SKIP + (side < f32(small_face)) * FACE_SMALL).astype(np.int32)


def similarity_pair(landm, ref_pts):
    """(tfm [2, 3], tfm_inv [2, 3], ok) in float64 from one face's landmarks ``(x0..x4, y0..y4)`` (float32) and the reference points (cast to float32)."""
    l = np.asarray(landm, f32).reshape(2, 5).astype(np.float64)
    src = l.T                                                            # [5, 2]
    dst = np.asarray(ref_pts, f32).astype(np.float64).reshape(5, 2)
    if not np.isfinite(src).all():
        return np.zeros((2, 3)), np.zeros((2, 3)), False
    sm, dm = src.sum(0) / 5, dst.sum(0) / 5
    s, d = src - sm, dst - dm
    a = (s[:, 0] * d[:, 0] + s[:, 1] * d[:, 1]).sum()
    b = (s[:, 0] * d[:, 1] - s[:, 1] * d[:, 0]).sum()
    var = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]).sum()
    if var == 0:
        return np.zeros((2, 3)), np.zeros((2, 3)), False
    R = np.array([[a, -b], [b, a]]) / var
    tfm = np.concatenate([R, (dm - R @ sm)[:, None]], 1)
    h = np.hypot(a, b)
    with np.errstate(all="ignore"):
        Ri = np.array([[a, b], [-b, a]]) / (h * (h / var))
        tinv = np.concatenate([Ri, (sm - Ri @ dm)[:, None]], 1)
    return tfm, tinv, True


def transforms(dets, landms, ref_pts, threshold, small_face):
    """(T float64 [n, 2, 2, 3]: forward then inverse; flags int32 [n])."""
    landms = np.asarray(landms, f32).reshape(-1, 10)
    flags = flags_of(dets, threshold, small_face)
    T = np.zeros((len(landms), 2, 2, 3))
    for i, l in enumerate(landms):
        T[i, 0], T[i, 1], ok = similarity_pair(l, ref_pts)
        if not ok:
            flags[i] |= FACE_SKIP
    return T, flags


# ------------------------------------------------------------------------------------------------ warpAffine
def _rne_sat(v):
    with np.errstate(invalid="ignore"):
        return np.clip(np.nan_to_num(np.rint(v), nan=-2.0 ** 31), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _wrap32(v):
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def invert_affine(M):
    """OpenCV's in-place inversion of a 2 x 3 map in float64, in its order."""
    M = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    with np.errstate(all="ignore"):
        D = np.float64(M[0]) * M[4] - np.float64(M[1]) * M[3]
        D = 1.0 / D if D != 0 else 0.0
        A11, A22 = M[4] * D, M[0] * D
        M[0], M[1], M[3], M[4] = A11, M[1] * -D, M[3] * -D, A22
        b1 = -M[0] * M[2] - M[1] * M[5]
        b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return np.array(M, np.float64)


def source_coords(M, w, h, rows=None):
    """(sx, sy, ax, ay) int64 [h, w] of the destination grid (or of its rows ``rows[0] .. rows[1] - 1``): the integer source pixel and the 1/32 fractions."""
    m = np.asarray(M, np.float64).reshape(6) if "not_inverted" in MUT else invert_affine(M)
    x, y = np.arange(w, dtype=np.float64), np.arange(*((0, h) if rows is None else rows), dtype=np.float64)
    off = 0 if "no_round_offset" in MUT else 16
    with np.errstate(all="ignore"):
        adelta, bdelta = _rne_sat(m[0] * x * 1024), _rne_sat(m[3] * x * 1024)
        X0 = _wrap32(_rne_sat((m[1] * y + m[2]) * 1024) + off)
        Y0 = _wrap32(_rne_sat((m[4] * y + m[5]) * 1024) + off)
    X = _wrap32(X0[:, None] + adelta[None, :]) >> 5
    Y = _wrap32(Y0[:, None] + bdelta[None, :]) >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def _taps(src, sx, sy):
    """The four neighbours [4, h, w(, c)] with 0 outside."""
    H, W = src.shape[:2]
    out = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        out.append(np.where(ok if v.ndim == 2 else ok[..., None], v, 0))
    return out


def warp_affine(src, M, dsize, flags=3, rows=None):
    """cv2.warpAffine(src, M, (w, h), flags=3) for a uint8 [H, W(, 3)] or float32 [H, W] image; ``rows``: only that band of the destination."""
    assert flags == 3
    w, h = int(dsize[0]), int(dsize[1])
    src = np.asarray(src)
    sx, sy, ax, ay = source_coords(M, w, h, rows)
    v = _taps(src, sx, sy)
    if src.dtype == np.uint8:
        e = (lambda t: t[..., None]) if src.ndim == 3 else (lambda t: t)
        wts = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
        acc = sum(v[k].astype(np.int64) * e(wts[k]) for k in range(4))
        return ((acc + (0 if "truncate" in MUT else 512)) >> 10).astype(np.uint8)
    assert src.dtype == np.float32 and src.ndim == 2
    fx, fy = ax.astype(f32) / f32(32), ay.astype(f32) / f32(32)
    w0, w1, w2, w3 = (f32(1) - fx) * (f32(1) - fy), fx * (f32(1) - fy), (f32(1) - fx) * fy, fx * fy
    with np.errstate(all="ignore"):
        return ((v[0] * w0 + v[1] * w1) + v[2] * w2) + v[3] * w3


# ------------------------------------------------------------------------------------------------ the filters
def _border(n, lo, hi):
    """BORDER_REFLECT_101 source indices of positions lo .. hi - 1 on an axis of n (|overhang| < n)."""
    i = np.arange(lo, hi)
    if n == 1:
        return np.zeros_like(i)
    if "reflect" in MUT:
        return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def filter2d_smooth(img):
    """uint8 [S, S, 3]: the 3 x 3 binomial filter, sum / 16 rounded half to even."""
    a = np.asarray(img, np.uint8).astype(np.int64)
    a = a[_border(a.shape[0], -1, a.shape[0] + 1)][:, _border(a.shape[1], -1, a.shape[1] + 1)]
    H, W = a.shape[0] - 2, a.shape[1] - 2
    s = sum(wy * wx * a[dy:dy + H, dx:dx + W] for dy, wy in enumerate((1, 2, 1)) for dx, wx in enumerate((1, 2, 1)))
    return ((s + 7 + ((s >> 4) & 1)) >> 4).astype(np.uint8)


def gaussian_taps(k, sigma):
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2
    t = np.exp(-0.5 * x * x / (float(sigma) * float(sigma)))
    return t / t.sum()


def gaussian_blur(img, ksize, sigma):
    """cv2.GaussianBlur(img, (k, k), sigma) of a float64 [S, S] plane: rows, then columns, BORDER_REFLECT_101, float64 throughout."""
    k = int(ksize[0]) if isinstance(ksize, (tuple, list)) else int(ksize)
    a = np.asarray(img, np.float64)
    H, W = a.shape
    if k % 2 != 1 or k // 2 >= min(H, W):
        raise ValueError(f"gaussian_blur: ksize {k} on a {H} x {W} plane")
    t, r = gaussian_taps(k, sigma), k // 2
    ix = _border(W, -r, W + r)
    row = np.zeros_like(a)
    for i in range(k):
        row += t[i] * a[:, ix[i:i + W]]
    iy = _border(H, -r, H + r)
    out = np.zeros_like(a)
    for i in range(k):
        out += t[i] * row[iy[i:i + H]]
    return out


def mask_postprocess(mask01, thres, ksize, sigma):
    """``FaceEnhancement.mask_postprocess`` with its constants as arguments: float64 [S, S] in, float32 out."""
    m = np.array(mask01, np.float64)
    if "border_kept" not in MUT:
        m[:thres, :] = 0
        m[-thres:, :] = 0
        m[:, :thres] = 0
        m[:, -thres:] = 0
    m = gaussian_blur(m, ksize, sigma)
    if "blur_once" not in MUT:
        m = gaussian_blur(m, ksize, sigma)
    return m.astype(f32)


def feather(mask_u8, thres, ksize, sigma):
    """uint8 0 / 255 parse mask [S, S] to the float32 paste mask."""
    return mask_postprocess(np.asarray(mask_u8, np.uint8) / 255., thres, ksize, sigma)


def convert_scale_abs(x):
    """cv2.convertScaleAbs of a float32 array: |x| rounded half to even, saturated to uint8."""
    x = np.abs(np.asarray(x, f32))
    r = np.floor(x + f32(0.5)) if "half_up" in MUT else np.rint(x)
    return np.clip(r, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the composition
def compose(base, warped_masks, warped_imgs):
    """full_mask / full_img over the faces in order, then the blend.  Returns (out uint8 [H, W, 3], full_mask float32 [H, W], pre: the float32 sum)."""
    H, W = base.shape[:2]
    full_mask, full_img = np.zeros((H, W), f32), np.zeros((H, W, 3), np.uint8)
    order = list(zip(warped_masks, warped_imgs))
    for m, p in (reversed(order) if "reverse" in MUT else order):
        diff = m - full_mask
        win = diff >= 0 if "ge" in MUT else diff > 0
        full_mask[win] = m[win]
        full_img[win] = p[win]
    fm = full_mask[:, :, None]
    pre = base * (1 - fm) + full_img * fm
    return convert_scale_abs(pre), full_mask, pre


def paste(base, faces, masks, T, flags, rows=None):
    """What e4s_gpen_paste_u8 computes: ``faces`` uint8 [n, S, S, 3] (already smoothed where small), ``masks`` float32 [n, S, S] (feathered), ``T`` [n, 2, 2, 3],
    ``flags`` [n] of one frame; ``rows``: only that band of the frame.  Returns (out, full_mask, pre, warped masks)."""
    H, W = base.shape[:2]
    keep = [i for i in range(len(faces)) if not flags[i] & FACE_SKIP]
    wm = [warp_affine(np.asarray(masks[i], f32), T[i, 1], (W, H), rows=rows) for i in keep]
    wi = [warp_affine(faces[i], T[i, 1], (W, H), rows=rows) for i in keep]
    out, fm, pre = compose(base if rows is None else base[rows[0]:rows[1]], wm, wi)
    return out, fm, pre, wm


def process(frame, dets, landms, enhance, parse, S, ksize, sigma, thres, threshold, small_face, base=None):
    """``FaceEnhancement.process(frame)`` of one frame with the networks as callables (``enhance``: uint8 crop -> uint8 face; ``parse``: face -> 0 / 255 mask).
    Returns (out, orig_faces, enhanced_faces, full_mask, pre, T, flags)."""
    T, flags = transforms(dets, landms, reference_points(S), threshold, small_face)
    faces, masks, orig, enh = [], [], [], []
    for i in range(len(flags)):
        if flags[i] & FACE_SKIP:
            faces.append(np.zeros((S, S, 3), np.uint8))
            masks.append(np.zeros((S, S), f32))
            continue
        of = warp_affine(frame, T[i, 0], (S, S))
        ef = enhance(of)
        orig.append(of)
        enh.append(ef)
        masks.append(feather(parse(ef), thres, ksize, sigma))
        faces.append(filter2d_smooth(ef) if flags[i] & FACE_SMALL else ef)
    out, fm, pre, _ = paste(frame if base is None else base, np.array(faces).reshape(-1, S, S, 3), np.array(masks).reshape(-1, S, S), T, flags)
    return out, orig, enh, fm, pre, T, flags


def strict_pixels(base, faces, masks, T, flags, eps=2.0 ** -20, rows=None):
    """bool [H, W]: the pixels at which a 2^-24-class difference in the warped masks cannot change the composition's choice or the rounding: every comparison
    ``m_i - full_mask > 0`` has |margin| > eps (or both sides are exactly 0: no face reaches the pixel), and the pre-rounding value of every channel lies farther
    than 255 eps from a half-integer."""
    out, fm, pre, wm = paste(base, faces, masks, T, flags, rows)
    strict, full = np.ones(fm.shape, bool), np.zeros(fm.shape, f32)
    for m in wm:
        diff = m.astype(np.float64) - full
        strict &= (np.abs(diff) > eps) | ((m == 0) & (full == 0))
        win = m - full > 0
        full[win] = m[win]
    frac = np.abs(pre.astype(np.float64) - np.floor(pre.astype(np.float64)) - 0.5)
    return strict & (frac > 255 * eps).all(-1)


# ------------------------------------------------------------------------------------------------ the fixture's cases
CASE_TAGS = ("A", "B", "C", "D", "E")
CASE_KEYS = ("frame", "dets", "landms", "ef", "pm", "out", "orig", "T", "cfg")


def load_case(golden, tag):
    rec = {k: golden[f"{tag}.{k}"] for k in CASE_KEYS}
    if f"{tag}.base" in golden:
        rec["base"] = golden[f"{tag}.base"]
    return rec


def config(rec):
    """(S, H, W, ksize, sigma, thres, small_face) of a stored case."""
    c = rec["cfg"]
    return int(c[0]), int(c[1]), int(c[2]), int(c[3]), float(c[4]), int(c[5]), float(c[6])


def model_outputs(rec, T=None):
    """The model on a stored case with the stored matrices (the reference's own) or ``T``: (out, orig crops, full_mask, pre, flags, faces, masks)."""
    S, H, W, k, sigma, thres, small = config(rec)
    T = rec["T"] if T is None else T
    flags = flags_of(rec["dets"], 0.9, small)
    orig = [warp_affine(rec["frame"], T[i, 0], (S, S)) for i in range(len(flags)) if not flags[i] & FACE_SKIP]
    faces = np.array([filter2d_smooth(f) if flags[i] & FACE_SMALL else f for i, f in enumerate(rec["ef"])], np.uint8).reshape(-1, S, S, 3)
    masks = np.array([feather(m, thres, k, sigma) for m in rec["pm"]], f32).reshape(-1, S, S)
    base = rec["base"] if "base" in rec else rec["frame"]
    out, fm, pre, _ = paste(base, faces, masks, T, flags)
    return out, np.array(orig, np.uint8).reshape(-1, S, S, 3), fm, pre, flags, faces, masks
