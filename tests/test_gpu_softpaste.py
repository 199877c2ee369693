"""GPU tests of row f6, the two-image caller's paste-back on the device: ``ops.soft_erosion`` (csrc/softmask.hip) against the float64 restatement
and the reference's own outputs (``g18_soft_paste.npz``), its two documented departures, ``soft_paste_masks`` / ``facial_mask12`` /
``blend_with_mask``, and ``pipeline.paste_back_soft`` / ``color_blend`` / ``swap_images``.

The bar on a soft mask is not a fixed number.  For every input the test computes how far the REFERENCE's float32 arithmetic (ATen's ``F.conv2d``)
lies from the float64 result and allows the kernel 10 times that: a tiled sum adds in another order than ATen's, and an order change moves an n-term
float32 sum by about that factor.  The tolerance never exceeds the derived worst case k^2 * 2^-24 per convolution pass * iterations / the plane
maximum (about 2e-4 for (17, 0.9, 7)).  Pixels whose float64 convolution value lies within 2e-5 of the threshold may legitimately fall on either
side in float32 and are left out; their share is asserted to stay under 2e-4 (measured on the CPU: at most 3.4e-5 on these inputs)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import align_model as M
import softpaste_model as SP
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import align, ops, pipeline, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
BAND = 2e-5
BAND_SHARE = 2e-4
CONFIGS = ((15, 0.6, 1), (17, 0.9, 7))


class Bars:
    """float64 and reference-float32 results for planes ``x`` [bs, C, H, W] under one configuration, and the bars derived from them."""

    def __init__(self, x, k, thr, it):
        x = np.asarray(x, dtype=np.float32)
        c64 = SP.soft_erosion_conv(x, k, it, torch.float64).numpy()
        self.soft64, self.hard64 = SP.soft_erosion(x, k, thr, it, torch.float64)
        self.soft32, _ = SP.soft_erosion(x, k, thr, it, torch.float32)
        self.band = np.abs(c64 - thr) <= BAND
        self.band_share = float(self.band.mean())
        ok = ~self.band
        self.ref_dev = float(np.abs(self.soft32 - self.soft64)[ok].max()) if ok.any() else 0.0
        below = np.where(self.hard64, -np.inf, c64).reshape(c64.shape[0] * c64.shape[1], -1).max(axis=1)
        below = below[np.isfinite(below) & (below > 0)]
        self.worst = k * k * 2.0 ** -24 * it / (float(below.min()) if below.size else 1.0)
        self.tol = min(10 * self.ref_dev, self.worst)

    def check(self, tag, soft, hard, ref_soft=None):
        soft, hard = soft.cpu().numpy(), hard.cpu().numpy()
        ok = ~self.band
        flips = int((hard != self.hard64)[ok].sum())
        d = float(np.abs(soft - (self.soft64 if ref_soft is None else ref_soft))[ok].max()) if ok.any() else 0.0
        record_parity(f"softpaste.{tag}.soft_max_abs", d, self.tol, f"reference float32 vs float64 {self.ref_dev:.2e}, worst case {self.worst:.1e}")
        record_parity(f"softpaste.{tag}.band_share", self.band_share, BAND_SHARE)
        record_parity(f"softpaste.{tag}.hard_flips_outside_band", flips, 0)
        assert self.band_share < BAND_SHARE, (tag, self.band_share)
        assert self.tol <= self.worst
        assert flips == 0, (tag, flips)
        assert not np.isnan(soft).any() and d <= self.tol, (tag, d, self.tol)


def _seeded_foregrounds(size):
    """[2, 2, size, size]: the foregrounds of two portrait-like and two blocky 512^2 maps; 1024 = their align_corners=True resize."""
    labs = np.concatenate([seeded.facelike_labels(5, 2), seeded.blocky_labels(3, 2)])
    fg = T(np.stack([SP.hard_paste_masks(l[None], None, 0)[0][0, 0] for l in labs]).reshape(2, 2, 512, 512))
    if size != 512:
        fg = F.interpolate(fg, size=(size, size), mode="bilinear", align_corners=True)
    return fg.contiguous()


@pytest.mark.parametrize("size", [512, 1024])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "k%d_t%g_i%d" % c)
def test_soft_erosion_against_float64(size, cfg):
    x = _seeded_foregrounds(size)
    soft, hard = ops.soft_erosion(x.to(DEV), *cfg)
    assert soft.shape == x.shape and hard.dtype == torch.bool and soft.dtype == torch.float32
    Bars(x.numpy(), *cfg).check("%d.k%d_t%g_i%d" % ((size,) + cfg), soft, hard)
    again, _ = ops.soft_erosion(x.to(DEV), *cfg)
    assert torch.equal(again, soft)                                    # deterministic: no atomics in the maximum


@pytest.mark.parametrize("name", ["face_96x80", "blocky_128", "resized_90x75"])
def test_soft_erosion_goldens(name):
    g = load_golden("g18_soft_paste")
    x = g[f"se.{name}.x"].astype(np.float32)
    for ci, (k, thr, it) in enumerate(g["configs"]):
        cfg = (int(k), float(thr), int(it))
        soft, hard = ops.soft_erosion(T(x).to(DEV), *cfg)
        b = Bars(x, *cfg)
        b.check(f"g18.{name}.c{ci}", soft, hard, ref_soft=g[f"se.{name}.c{ci}.soft"])
        assert np.array_equal(hard.cpu().numpy()[~b.band], g[f"se.{name}.c{ci}.hard"][~b.band])


def test_the_two_documented_departures_and_plane_independence():
    """An all-pass plane is all ones (reference: raises), an all-zero plane all zeros without NaN (reference: NaN), and neither changes the
    other planes of the batch: the maximum is per plane."""
    x = np.zeros((2, 3, 40, 70), np.float32)
    x[0, 0] = 4.0                                   # c >= 0.6 everywhere, the corners included
    x[0, 2, 10:30, 20:50] = 1.0
    x[1, 0, 5:35, 5:60] = 1.0
    x[1, 2, 0:8, 0:8] = 0.5                         # nothing passes the threshold
    soft, hard = ops.soft_erosion(T(x).to(DEV))
    s, h = soft.cpu().numpy(), hard.cpu().numpy()
    assert h[0, 0].all() and (s[0, 0] == 1).all()
    assert not h[0, 1].any() and (s[0, 1] == 0).all() and not h[1, 1].any() and (s[1, 1] == 0).all()
    assert not np.isnan(s).any()
    assert not h[1, 2].any() and s[1, 2].max() == 1.0           # all below: normalised by its own maximum
    for b, c in ((0, 2), (1, 0), (1, 2)):
        alone, alone_h = ops.soft_erosion(T(x[b:b + 1, c:c + 1]).to(DEV))
        assert torch.equal(alone[0, 0], soft[b, c]) and torch.equal(alone_h[0, 0], hard[b, c]), (b, c)
    Bars(x, 15, 0.6, 1).check("departures", soft, hard)
    neg, _ = ops.soft_erosion(T(-x).to(DEV))                     # any finite input: the maximum of a negative plane is found, not assumed >= 0
    ref, _ = SP.soft_erosion(-x, dtype=torch.float64)
    assert np.abs(neg.cpu().numpy() - ref).max() <= 1e-5
    e, eh = ops.soft_erosion(torch.zeros(0, 1, 8, 8, device=DEV))
    assert e.shape == (0, 1, 8, 8) and eh.shape == (0, 1, 8, 8)


@pytest.mark.parametrize("shape,cfg", [((1, 1, 7, 5), (15, 0.15, 1)), ((2, 1, 33, 1), (5, 0.5, 2)), ((1, 2, 1, 90), (17, 0.9, 3)), ((1, 1, 9, 9), (33, 0.3, 2)),
                                       ((1, 3, 65, 129), (3, 0.5, 4)), ((2, 2, 100, 67), (9, 0.45, 2))])
def test_soft_erosion_ragged_sizes(shape, cfg):
    """Sizes that are no multiple of the 64 x 32 tile, a width and a height of 1, kernels larger than the image, every iteration count's buffers."""
    rs = np.random.RandomState(sum(shape) + cfg[0])
    x = (rs.rand(*shape) > 0.35).astype(np.float32)
    x[..., : shape[-2] // 2, :] *= rs.rand(*shape)[..., : shape[-2] // 2, :].astype(np.float32)          # half of it non-binary
    soft, hard = ops.soft_erosion(T(x).to(DEV), *cfg)
    Bars(x, *cfg).check("ragged.%dx%d.k%d" % (shape[-2], shape[-1], cfg[0]), soft, hard)


# ------------------------------------------------------------------------------------------------ masks and blends
def _masks_inputs(bs=2):
    lab = seeded.facelike_labels(9, bs)
    lab[1] = seeded.blocky_labels(4, 1)[0]
    hole = np.zeros(lab.shape, np.uint8)
    hole[:, 300:380, 150:300] = 1
    return lab, hole


@pytest.mark.parametrize("radius", [2, 10])
def test_soft_paste_masks_against_the_restatement(radius):
    lab, hole = _masks_inputs()
    content, border, full = ops.soft_paste_masks(T(lab).to(DEV), T(hole).to(DEV), radius)
    fg, dil, ero = SP.hard_paste_masks(lab, hole, radius)
    b = Bars(np.concatenate([dil, ero, fg], axis=1), 15, 0.6, 1)
    assert b.band_share < BAND_SHARE
    s64, ok = b.soft64, ~b.band
    got = np.concatenate([full.cpu().numpy(), border.cpu().numpy(), content.cpu().numpy()], axis=1)
    want = np.concatenate([s64[:, 0:1], np.clip(s64[:, 0:1] - s64[:, 1:2], 0, 1), s64[:, 2:3]], axis=1)
    keep = np.stack([ok[:, 0], ok[:, 0] & ok[:, 1], ok[:, 2]], axis=1)
    for i, (name, scale) in enumerate((("full", 1), ("border", 2), ("content", 1))):      # border is a difference of two soft masks
        d = float(np.abs(got[:, i] - want[:, i])[keep[:, i]].max())
        record_parity(f"softpaste.masks.r{radius}.{name}_max_abs", d, scale * b.tol)
        assert d <= scale * b.tol, (name, d, b.tol)
    r32 = SP.soft_paste_masks(lab, hole, radius)
    assert max(float(np.abs(a.cpu().numpy() - r)[keep[:, j:j + 1]].max()) for a, r, j in ((content, r32[0], 2), (border, r32[1], 1), (full, r32[2], 0))) <= 2 * b.tol
    nohole = ops.soft_paste_masks(T(lab).to(DEV), None, radius)
    assert nohole[0].shape == (2, 1, 512, 512) and not torch.equal(nohole[0], content)
    empty = ops.soft_paste_masks(torch.zeros(0, 16, 16, dtype=torch.uint8, device=DEV))
    assert all(t.shape == (0, 1, 16, 16) for t in empty)


def test_soft_paste_masks_goldens():
    g = load_golden("g18_soft_paste")
    lab, hole = g["exp.labels"][None], g["exp.hole"][None]
    for radius in (2, 10):
        fg, dil, ero = SP.hard_paste_masks(lab, hole, radius)
        b = Bars(np.concatenate([dil, ero, fg], axis=1), 15, 0.6, 1)
        ok = ~b.band
        got = ops.soft_paste_masks(T(lab).to(DEV), T(hole).to(DEV), radius)
        for t, name, keep, scale in zip(got, ("content", "border", "full"), (ok[:, 2:3], ok[:, 0:1] & ok[:, 1:2], ok[:, 0:1]), (1, 2, 1)):
            d = float(np.abs(t.cpu().numpy() - g[f"exp.r{radius}.{name}"])[keep].max())
            record_parity(f"softpaste.g18.exp.r{radius}.{name}_max_abs", d, scale * b.tol)
            assert d <= scale * b.tol, (radius, name, d, b.tol)


def test_facial_mask12_against_the_restatement_and_golden():
    g = load_golden("g18_soft_paste")
    size = tuple(int(v) for v in g["facial.size"])
    got = ops.facial_mask12(T(g["facial.labels"])[None].to(DEV), size)
    b = Bars(SP.facial_mask12_hard(g["facial.labels"][None], size).numpy(), 15, 0.6, 1)
    d = float(np.abs(got.cpu().numpy() - g["facial.out"])[~b.band].max())
    record_parity("softpaste.g18.facial_max_abs", d, b.tol)
    assert got.shape == (1, 1) + size and d <= b.tol
    lab = seeded.facelike_labels(12, 2)
    for kw in ({}, {"kernel_size": 17, "threshold": 0.9, "iterations": 7}):
        got = ops.facial_mask12(T(lab).to(DEV), (1024, 1024), **kw)
        hard = SP.facial_mask12_hard(lab, (1024, 1024))
        resized = ops.bilinear_resize(T(np.isin(lab, SP.FACIAL_CLASSES).astype(np.float32))[:, None].to(DEV), (1024, 1024), align_corners=True)
        rd = float((resized.cpu() - hard).abs().max())          # the device's bilinear resize against ATen's: the softer's input
        cfg = (kw.get("kernel_size", 15), kw.get("threshold", 0.6), kw.get("iterations", 1))
        b = Bars(hard.numpy(), *cfg)
        tol = min(b.tol + 2 * rd, b.worst)
        d = float(np.abs(got.cpu().numpy() - b.soft64)[~b.band].max())
        record_parity("softpaste.facial_1024.k%d_max_abs" % cfg[0], d, tol, f"resize deviation {rd:.1e}")
        assert b.band_share < BAND_SHARE and d <= tol, (d, tol)
    assert torch.equal(ops.facial_mask12(T(lab).to(DEV)), ops.soft_erosion(T(np.isin(lab, SP.FACIAL_CLASSES).astype(np.float32))[:, None].to(DEV))[0])


@pytest.mark.parametrize("ratio", [1.0, 0.75, 0.0])
@pytest.mark.parametrize("channels", [1, 3])
def test_blend_with_mask_equals_numpy_bit_for_bit(ratio, channels):
    rs = np.random.RandomState(31)
    n, h, w = 3, 67, 53
    bottom, up = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8), rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    mask = rs.rand(n, channels, h, w).astype(np.float32)
    mask[rs.rand(*mask.shape) < 0.05] = np.nan
    mask[rs.rand(*mask.shape) < 0.1] = 1.0
    mask[rs.rand(*mask.shape) < 0.1] = 0.0
    bottom[0, :8], up[0, :8], mask[0, :, :8] = 255, 255, rs.rand(channels, 8, w).astype(np.float32)       # sums that round to 255 or just above
    got = ops.blend_with_mask(T(bottom).to(DEV), T(up).to(DEV), T(mask).to(DEV), ratio).cpu().numpy()
    want = SP.blend_with_mask(bottom, up, mask, ratio)
    d = int((got != want).sum())
    record_parity(f"softpaste.blend.r{ratio:g}.c{channels}.bytes_vs_numpy", d, 0)
    assert d == 0
    if ratio != 0.0:
        g = load_golden("g18_soft_paste")
        m = np.repeat(g["blend.mask"][None, None], channels, axis=1)
        out = ops.blend_with_mask(T(g["blend.bottom"])[None].to(DEV), T(g["blend.up"])[None].to(DEV), T(m).to(DEV), ratio).cpu().numpy()[0]
        assert np.array_equal(out, g[f"blend.out_{int(ratio * 100)}"])
    fr = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.blend_with_mask(fr, fr, torch.zeros(1, 2, 8, 8, device=DEV))
    with pytest.raises(ValueError):
        ops.blend_with_mask(fr, fr, torch.zeros(1, 1, 8, 8, device=DEV), 1.5)
    assert ops.blend_with_mask(fr[:0], fr[:0], torch.zeros(0, 1, 8, 8, device=DEV)).shape == (0, 8, 8, 3)


# ------------------------------------------------------------------------------------------------ pipeline
def _paste_inputs(bs=1, seed=21):
    rs = np.random.RandomState(seed)
    sw = rs.randint(0, 256, (bs, 1024, 1024, 3)).astype(np.uint8)
    tg = rs.randint(0, 256, (bs, 1024, 1024, 3)).astype(np.uint8)
    lab = seeded.facelike_labels(5, bs)
    hole = np.zeros(lab.shape, np.uint8)
    hole[:, 320:400, 200:330] = 1
    return sw, tg, lab, hole


def test_paste_back_soft_chain_against_the_restatement():
    """pipeline.paste_back_soft = _past_back:177-219 against the restatement chain (soft masks -> resize -> truncating paste -> the oracle's multi-band
    blend), at the bar ``test_paste_back_chain_against_the_oracle`` uses for the video chain (the blend itself stays parity-unpinned: no cv2)."""
    sw, tg, lab, hole = _paste_inputs()
    out = pipeline.paste_back_soft(T(sw).to(DEV), T(tg).to(DEV), T(lab).to(DEV), T(hole).to(DEV)).cpu().numpy()
    ref = SP.paste_back_soft(sw, tg, lab, hole)
    diff = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    record_parity("softpaste.paste_back_soft.max_abs_levels", int(diff.max()), 1)
    record_parity("softpaste.paste_back_soft.share_off_by_one", float((diff > 0).mean()), 2e-3)
    assert out.shape == ref.shape and diff.max() <= 1 and (diff > 0).mean() <= 2e-3, (diff.max(), (diff > 0).mean())
    assert (out != tg).any() and (out != sw).any()
    # no face in the map: the documented all-zero departure leaves the target untouched where the reference would paste NaN
    zeros = torch.zeros(1, 512, 512, dtype=torch.uint8, device=DEV)
    content, border, _ = ops.soft_paste_masks(zeros)
    assert not content.any() and not border.any()
    assert torch.equal(ops.blend_with_mask(T(tg).to(DEV), T(sw).to(DEV), ops.bilinear_resize(content, (1024, 1024))), T(tg).to(DEV))
    none = pipeline.paste_back_soft(T(sw).to(DEV), T(tg).to(DEV), zeros).cpu().numpy().astype(np.int32)
    assert np.abs(none - tg).max() <= 1                    # (the multi-band blend of T with itself: a float pyramid, then truncation)


def test_color_blend_against_the_restatement():
    sw, rc, lab, _ = _paste_inputs(2, 22)
    rs = np.random.RandomState(23)
    edge = (rs.rand(2, 1024, 1024) ** 4).astype(np.float32)
    for e in (None, edge):
        got = pipeline.color_blend(T(sw).to(DEV), T(rc).to(DEV), T(lab).to(DEV), None if e is None else T(e).to(DEV)).cpu().numpy()
        want = SP.color_blend(sw, rc, lab, e)
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))        # masks agree to ~1e-5: a product may truncate to the neighbouring level
        record_parity("softpaste.color_blend.%s.share_off_by_one" % ("plain" if e is None else "edge"), float((diff > 0).mean()), 2e-3)
        assert diff.max() <= 1 and (diff > 0).mean() <= 2e-3, (diff.max(), (diff > 0).mean())
    mask = ops.facial_mask12(T(lab).to(DEV), (1024, 1024))
    assert torch.equal(pipeline.color_blend(T(sw).to(DEV), T(rc).to(DEV), T(lab).to(DEV)), ops.blend_with_mask(T(sw).to(DEV), T(rc).to(DEV), mask, 0.75))


def _capture(fn):
    eager = fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    graph.replay()
    torch.cuda.synchronize()
    return eager, out


def test_soft_erosion_and_paste_back_soft_inside_graph_capture():
    """No host synchronisation anywhere (the reference's ``x[~mask].max()`` is one): capture + replay gives the eager bits."""
    x = _seeded_foregrounds(512).to(DEV)
    for cfg in CONFIGS:
        eager, out = _capture(lambda: ops.soft_erosion(x, *cfg))
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    sw, tg, lab, hole = (T(a).to(DEV) for a in _paste_inputs())
    eager, out = _capture(lambda: pipeline.paste_back_soft(sw, tg, lab, hole))
    assert torch.equal(out, eager)


@pytest.fixture(scope="module")
def parser(bisenet_sd):
    install_dropin()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    p = FaceParser(seg_ckpt=None, device=DEV)
    p.seg.load_state_dict(bisenet_sd)
    p.seg.eval()
    return p


def _outside_quad(quad, h, w, margin=1.5):
    """bool [h, w]: pixels whose centre lies more than ``margin`` pixels outside the convex quad ``[4, 2]`` (x, y).  The paste samples the face
    bilinearly at the pixel centre, so a pixel up to a sample's footprint beyond the quad's edge may still take part of the face."""
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx + 0.5, yy + 0.5
    area = sum(quad[k][0] * quad[(k + 1) % 4][1] - quad[(k + 1) % 4][0] * quad[k][1] for k in range(4))
    sign = 1.0 if area > 0 else -1.0
    out = np.zeros((h, w), bool)
    for k in range(4):
        (ax, ay), (bx, by) = quad[k], quad[(k + 1) % 4]
        dist = sign * ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) / np.hypot(bx - ax, by - ay)          # > 0 inside this edge
        out |= dist < -margin
    return out


def _recolor(swapped, crops):
    return torch.lerp(swapped.float(), crops.float(), 0.5).to(torch.uint8)


@pytest.mark.parametrize("recolor", [False, True])
def test_swap_images_bs2(gpu_net3, parser, recolor):
    rng = np.random.default_rng(15)
    frames = np.stack([M.make_frame(rng, 1080, 1920) for _ in range(2)])
    quads = np.stack([M.square_quad(960, 540, 300, 0.35), M.square_quad(1800, 120, 380, -0.5)])
    plan = align.crop_plan(quads, (1080, 1920), 1024)
    driven = seeded.seeded_image(16, 2, 1024).to(DEV)
    fr = T(frames).to(DEV)
    fn = _recolor if recolor else None
    got = pipeline.swap_images(gpu_net3, parser, driven, fr, plan, recolor_fn=fn)
    assert got.shape == fr.shape and got.dtype == torch.uint8 and torch.equal(fr.cpu(), T(frames))
    # the step-by-step composition of the public pieces
    crops = ops.crop_align(fr, plan)
    sw, lab, extra = pipeline.swap_batch(gpu_net3, parser, driven, ops.frames_to_tensor(crops), mask_surgery=True, ear_interpolation=False,
                                         comp_indices=pipeline.IMAGE_COMP_INDICES_CT if recolor else pipeline.IMAGE_COMP_INDICES)
    if recolor:
        sw = pipeline.color_blend(sw, _recolor(sw, crops), lab)
    step = pipeline.paste_back_soft(sw, crops, lab, extra["hole_mask"])
    step = pipeline.paste_back_soft(step, crops, torch.full_like(lab, 6))
    want = ops.paste_into_frames(step, fr, plan)
    assert torch.equal(got, want)
    g = got.cpu().numpy()
    for i in range(2):
        x0, y0, x1, y1 = plan.paste_boxes[i].tolist()
        outside = np.ones(g.shape[1:3], bool)
        outside[y0:y1, x0:x1] = False
        assert np.array_equal(g[i][outside], frames[i][outside])
        outside = _outside_quad(np.asarray(plan.quads[i], dtype=np.float64), g.shape[1], g.shape[2])
        assert outside[y0:y1, x0:x1].any()                        # the quad is rotated: its bounding box holds pixels outside it
        assert np.array_equal(g[i][outside], frames[i][outside])
        assert (g[i] != frames[i]).any()
    if not recolor:
        video = pipeline.swap_frames(gpu_net3, parser, driven, fr, plan)
        assert not torch.equal(video, got)                        # another paste-back and another style mix than the video caller's
        guards = []
        under = pipeline.swap_images(gpu_net3, parser, driven, fr, plan, guard=guards)
        assert len(guards) == 1
        if not guards[0].tripped():
            assert torch.equal(under, got)
        for k, v in (("mask_surgery", True), ("to_uint8", True), ("ear_interpolation", True), ("comp_indices", (1,))):
            with pytest.raises(TypeError, match="fixed"):
                pipeline.swap_images(gpu_net3, parser, driven, fr, plan, **{k: v})
