"""CPU tests of the crop-align / paste-into-frame path (row f5): the host geometry of ``e4s2024_amd.align`` against a direct evaluation of its
formulas and against scipy, the numpy model of Pillow's warps (``tests/align_model.py``) against Pillow itself byte for byte — which is what
lets the GPU tests trust the model — the Lanczos tables, and the argument checks of the two C entry points (no launches)."""
import ctypes

import numpy as np
import pytest
import torch

import align_model as M
from e4s2024_amd import align


def _landmarks(seed, n):
    """Plausible 68-point sets: a face of random size / position / roll, jittered per point."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(68, 2)) * 3
    base[36:42] += [-30, -20]                  # left eye
    base[42:48] += [30, -20]                   # right eye
    base[48] += [-25, 40]                      # mouth corners
    base[54] += [25, 40]
    out = []
    for _ in range(n):
        s, a = rng.uniform(0.5, 3.0), rng.uniform(-0.6, 0.6)
        r = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        out.append(base @ r.T * s + rng.uniform(100, 900, size=2) + rng.normal(size=(68, 2)))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_transform_from_landmarks_matches_the_formula(seed):
    lm = _landmarks(seed, 6)
    for scale in (1.0, 1.3):
        c, x, y = align.transform_from_landmarks(lm, scale)
        eye_l, eye_r = lm[:, 36:42].mean(1), lm[:, 42:48].mean(1)
        eye_avg = (eye_l + eye_r) / 2
        e2e = eye_r - eye_l
        e2m = (lm[:, 48] + lm[:, 54]) / 2 - eye_avg
        xx = e2e - e2m[:, ::-1] * [-1, 1]
        xx = xx / np.hypot(xx[:, 0], xx[:, 1])[:, None]
        xx = xx * np.maximum(np.hypot(e2e[:, 0], e2e[:, 1]) * 2.0, np.hypot(e2m[:, 0], e2m[:, 1]) * 1.8)[:, None] * scale
        np.testing.assert_allclose(x, xx, rtol=1e-13, atol=1e-10)
        np.testing.assert_allclose(y, np.stack([-xx[:, 1], xx[:, 0]], 1), rtol=1e-13, atol=1e-10)
        np.testing.assert_allclose(c, eye_avg + 0.1 * e2m, rtol=1e-13, atol=1e-10)
    q = align.quads_from_transforms(c, x, y)
    assert q.shape == (6, 4, 2)
    np.testing.assert_array_equal(q[:, 0], c - x - y)
    np.testing.assert_array_equal(q[:, 1], c - x + y)
    np.testing.assert_array_equal(q[:, 2], c + x + y)
    np.testing.assert_array_equal(q[:, 3], c + x - y)


@pytest.mark.parametrize("n", [1, 2, 5, 40])
@pytest.mark.parametrize("sigma", [0.0, 1.0, 3.0])
def test_smooth_transforms_matches_scipy(n, sigma):
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(n)
    c, x, y = (rng.normal(size=(n, 2)) * 100 + 500 for _ in range(3))
    sc, sx, sy = align.smooth_transforms(c, x, y, center_sigma=sigma, xy_sigma=sigma)
    for got, src in ((sc, c), (sx, x), (sy, y)):
        want = src if sigma == 0 else nd.gaussian_filter1d(src, sigma=sigma, axis=0)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    sc, sx, sy = align.smooth_transforms(c, x, y, center_sigma=1.0, xy_sigma=3.0)       # the target side's two sigmas
    np.testing.assert_allclose(sc, nd.gaussian_filter1d(c, 1.0, axis=0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(sy, nd.gaussian_filter1d(y, 3.0, axis=0), rtol=1e-12, atol=0)


def test_crop_plan_boxes_and_shift():
    h, w, s = 800, 1000, 1024
    # inside: a 400 px square at (500, 400): qsize = 400*sqrt2*... -> no shrink, border rint(0.1 * 565.7) = 57
    q = M.square_quad(500, 400, 200)
    p = align.crop_plan(q, (h, w), s)
    assert int(p.shrink[0]) == 1 and tuple(p.resized_wh[0]) == (w, h)
    assert p.boxes[0].tolist() == [300 - 57, 200 - 57, 700 + 57, 600 + 57]
    assert p.quad_coeffs[0, 0].item() == 300 - 243 + 0.5 and p.quad_coeffs[0, 4].item() == 200 - 143 + 0.5    # NW corner, shifted, + 0.5
    assert p.paste_boxes[0].tolist() == [299, 199, 702, 602]
    # overhanging each edge: the box is clipped to the frame and the shift is its clipped origin
    for cx, cy, want in ((50, 400, (0, 143, 307, 657)), (950, 400, (693, 143, 1000, 657)), (500, 30, (243, 0, 757, 287)),
                         (500, 780, (243, 523, 757, 800))):
        p = align.crop_plan(M.square_quad(cx, cy, 200), (h, w), s)
        assert tuple(p.boxes[0].tolist()) == want, (cx, cy)
        assert p.quad_coeffs[0, 0].item() == cx - 200 - want[0] + 0.5 and p.quad_coeffs[0, 4].item() == cy - 200 - want[1] + 0.5
    # the box covers the whole frame: no crop, no shift
    p = align.crop_plan(M.square_quad(500, 400, 460), (h, w), s)
    assert p.boxes[0].tolist() == [0, 0, w, h] and p.quad_coeffs[0, 0].item() == 40.5
    # shrink: diagonal >= 4 S -> shrink = floor(diag / S / 2), the frame resized by it (rint), quad and box in the resized frame
    p = align.crop_plan(M.square_quad(2000, 1100, 1500), (2160, 3840), 1024)      # diag = 4243 -> shrink 2
    assert int(p.shrink[0]) == 2 and tuple(p.resized_wh[0]) == (1920, 1080)
    border = int(np.rint(1500 * 2 * np.sqrt(2) / 2 * 0.1))
    assert p.boxes[0].tolist() == [max(250 - border, 0), 0, min(1750 + border, 1920), 1080]
    p = align.crop_plan(M.square_quad(1000, 700, 1100), (1401, 2001), 512)         # diag 3111 -> shrink 3, odd frame sizes round
    assert int(p.shrink[0]) == 3 and tuple(p.resized_wh[0]) == (667, 467)
    # the paste coefficients come from the UNSHRUNK, UNSHIFTED quad: they send its corners (+ 0.5) to the square's corners
    q = M.square_quad(2000, 1100, 1500, 0.3)
    p = align.crop_plan(q, (2160, 3840), 1024)
    a = p.inv_coeffs[0].numpy()
    for (px, py), (tx, ty) in zip(q + 0.5, [(0, 0), (0, 1024), (1024, 1024), (1024, 0)]):
        den = a[6] * px + a[7] * py + 1
        assert abs((a[0] * px + a[1] * py + a[2]) / den - tx) < 1e-6 and abs((a[3] * px + a[4] * py + a[5]) / den - ty) < 1e-6
    with pytest.raises(ValueError):
        align.crop_plan(M.square_quad(-5000, 400, 100), (h, w), s)                # the face is nowhere in the frame


def test_plan_slices_and_to():
    lm = _landmarks(3, 5)
    p = align.plan_from_landmarks(lm, (1080, 1920))
    assert len(p) == 5 and p.boxes.dtype == torch.int32 and p.quad_coeffs.dtype == torch.float64 and p.inv_coeffs.shape == (5, 8)
    sub = p[1:3]
    assert len(sub) == 2 and torch.equal(sub.quad_coeffs, p.quad_coeffs[1:3]) and torch.equal(sub.boxes, p.boxes[1:3])
    assert p.to("cpu").quad_coeffs.device.type == "cpu"
    c, x, y = align.smooth_transforms(*align.transform_from_landmarks(lm), 1.0, 3.0)
    q = align.crop_plan(align.quads_from_transforms(c, x, y), (1080, 1920))
    assert torch.equal(q.quad_coeffs, p.quad_coeffs) and torch.equal(q.inv_coeffs, p.inv_coeffs)


# ------------------------------------------------------------------------------------------------ the model against Pillow
CASES = [  # (frame h, w, output size, quad) — inside, rotated, overhanging, beyond the frame, tiny, shrink
    (120, 160, 64, M.square_quad(80, 60, 30)),
    (120, 160, 64, M.square_quad(70, 50, 33, 0.4)),
    (120, 160, 48, M.square_quad(10, 100, 40, -0.7)),
    (120, 160, 64, M.square_quad(150, 5, 45, 2.5)),
    (90, 70, 80, M.square_quad(35, 45, 200, 0.1)),
    (120, 160, 64, M.square_quad(90, 70, 2.3, 0.9)),
    (300, 400, 32, M.square_quad(200, 140, 70, 0.2)),          # diag 198 -> shrink 3
    (301, 399, 40, M.square_quad(180, 160, 60, -0.35)),        # diag 170 -> shrink 2
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_crop_model_and_plan_equal_pillow(case):
    pytest.importorskip("PIL.Image")
    h, w, s, q = CASES[case]
    frame = M.make_frame(np.random.default_rng(case), h, w)
    plan = align.crop_plan(q, (h, w), s)
    got = M.crop_align(frame, plan, 0)
    want = M.pil_crop_image(frame, q, s)
    assert int((got != want).sum()) == 0
    assert (want != 0).any()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_paste_model_equals_pillow_alpha_composite(case):
    pytest.importorskip("PIL.Image")
    h, w, s, q = CASES[case]
    rng = np.random.default_rng(100 + case)
    frame, face = M.make_frame(rng, h, w), M.make_frame(rng, s, s)
    plan = align.crop_plan(q, (h, w), s)
    got = M.paste(face, frame, plan, 0)
    want = M.pil_paste(face, frame, plan.inv_coeffs[0].numpy())
    assert int((got != want).sum()) == 0
    x0, y0, x1, y1 = plan.paste_boxes[0].tolist()        # nothing outside the paste box changes
    outside = np.ones((h, w), bool)
    outside[y0:y1, x0:x1] = False
    assert np.array_equal(want[outside], frame[outside])


def test_model_against_pillow_on_random_quads():
    """Arbitrary (non-square) quads and perspective data, partly outside the source: both warps, 0 differing bytes."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for k in range(6):
        src = M.make_frame(rng, int(rng.integers(20, 90)), int(rng.integers(20, 90)))
        quad = rng.uniform(-30, 120, size=(4, 2))
        size = int(rng.integers(16, 72))
        data = align.quad_coefficients(quad, size)
        want = np.asarray(Image.fromarray(src).transform((size, size), Image.QUAD, quad.flatten(), Image.BILINEAR))
        assert int((M.warp_quad(src, data, size) != want).sum()) == 0, k
        frame = M.make_frame(rng, 70, 90)
        inv = align.perspective_coefficients(quad, [[0, 0], [0, src.shape[0]], [src.shape[1], src.shape[0]], [src.shape[1], 0]])
        face = M.make_frame(rng, src.shape[0], src.shape[1])
        assert int((M.paste_perspective(face, frame, inv) != M.pil_paste(face, frame, inv)).sum()) == 0, k


@pytest.mark.parametrize("src_wh,dst_wh", [((160, 120), (80, 60)), ((401, 301), (134, 100)), ((97, 61), (33, 31)), ((64, 48), (130, 90))])
def test_lanczos_tables_and_two_pass_resample_equal_pillow(src_wh, dst_wh):
    Image = pytest.importorskip("PIL.Image")
    img = M.make_frame(np.random.default_rng(src_wh[0]), src_wh[1], src_wh[0])
    want = np.asarray(Image.fromarray(img).resize(dst_wh, Image.LANCZOS))
    assert int((M.pil_resize(img, dst_wh, "lanczos") != want).sum()) == 0
    want = np.asarray(Image.fromarray(img).resize(dst_wh))                  # the bicubic tables are unchanged
    assert int((M.pil_resize(img, dst_wh) != want).sum()) == 0


# ------------------------------------------------------------------------------------------------ C entry points: argument checks
def test_align_entry_points_reject_bad_arguments_without_gpu():
    from e4s2024_amd._lib import lib
    c = lib().cdll
    one = ctypes.c_void_p(16)          # non-null dummy device pointers: validation fails before they are touched
    good = np.array([[0, 0, 8, 8]], dtype=np.int32)
    box = lambda b: np.ascontiguousarray(b, dtype=np.int32).ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    for fn in (c.e4s_warp_quad_u8, c.e4s_warp_perspective_paste_u8):
        assert fn(None, one, box(good), one, 1, 8, 8, 4, None) == -1
        assert b"null" in c.e4s_last_error()
        assert fn(one, None, box(good), one, 1, 8, 8, 4, None) == -1
        assert fn(one, one, None, one, 1, 8, 8, 4, None) == -1
        assert fn(one, one, box(good), None, 1, 8, 8, 4, None) == -1
        for n in (0, -1):
            assert fn(one, one, box(good), one, n, 8, 8, 4, None) == -1
            assert b"frames" in c.e4s_last_error()
        for s in (0, -4):
            assert fn(one, one, box(good), one, 1, 8, 8, s, None) == -1
            assert b"output size" in c.e4s_last_error()
        assert fn(one, one, box(good), one, 1, 0, 8, 4, None) == -1
        for bad in ([0, 0, 9, 8], [-1, 0, 8, 8], [0, 0, 8, 9], [5, 0, 4, 8], [0, 6, 8, 5]):
            assert fn(one, one, box([good[0], bad]), one, 2, 8, 8, 4, None) == -1
            assert b"box 1" in c.e4s_last_error() and b"not inside" in c.e4s_last_error()


def test_align_ops_check_their_arguments():
    from e4s2024_amd import ops
    plan = align.crop_plan(M.square_quad(40, 30, 10), (60, 80), 32)
    with pytest.raises(TypeError):
        ops.crop_align(np.zeros((1, 60, 80, 3), np.uint8), plan)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.crop_align(torch.zeros((1, 60, 80, 3), dtype=torch.uint8), plan)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.paste_into_frames(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), torch.zeros((1, 60, 80, 3), dtype=torch.uint8), plan)
