"""GPU tests of row f7, the two-image caller's skin colour transfer on the device (``csrc/colortransfer.hip``): ``ops.grey_dilate`` / ``grey_erode``
bit for bit against the reference's outputs (``g19_color_transfer.npz``) and the model, the statistics and the 3 x 3 map against the float64 model,
``ops.skin_color_transfer`` against the reference's bytes, ``ops.soft_expansion_masks``, and ``pipeline.color_transfer`` / ``swap_images(ct_mode=...)``.

Bounds, none of them tuned:

* morphology and the float32 composition are exact;
* the map: the nine raw moments are summed in float64 (relative error <= N 2^-53 = 1.2e-10 at N = 2^20), the covariance is their difference, and the
  square roots amplify an error in it by at most 1 / lambda_min; with lambda_min >= 4e-3 on the fixture pairs (1e-5, lct's regulariser, under an empty
  mask, where the sums are exact zeros) that stays under 1e-7 relative to the norm of the map;
* the quantised output: at most one grey level and at most 1e-3 of the bytes against the reference (the model alone: 1.8e-5 .. 1.4e-4);
* the soft masks: the tolerance and the threshold band of ``test_gpu_softpaste.py`` (the same arithmetic);
* the whole chain: one level, and a share of differing bytes of at most the q step's measured share plus ``paste_back_soft``'s recorded 4.6e-4."""
import numpy as np
import pytest
import torch

import colortransfer_model as CM
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import align, ops, pipeline, seeded
from test_gpu_softpaste import BAND_SHARE, Bars, _capture, _outside_quad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
MAP_REL = 1e-7
MAX_SHARE = 1e-3
PASTE_BACK_SOFT_SHARE = 4.6e-4        # pipeline.paste_back_soft against its restatement


# ------------------------------------------------------------------------------------------------ grey morphology
@pytest.mark.parametrize("shape,radii", CM.MORPH_SHAPES, ids=lambda v: "x".join(str(i) for i in v))
def test_grey_morphology_equals_the_reference_bit_for_bit(shape, radii):
    g = load_golden("g19_color_transfer")
    x = CM.morph_input(shape)
    tag = "x".join(str(v) for v in shape)
    xd = T(x).to(DEV)
    for r in radii:
        for name, fn, model in (("dilate", ops.grey_dilate, CM.grey_dilate), ("erode", ops.grey_erode, CM.grey_erode)):
            got = fn(xd, r)
            assert got.shape == xd.shape and got.dtype == torch.float32
            got = got.cpu().numpy()
            assert np.array_equal(got, g[f"morph.{tag}.r{r}.{name}"]), (tag, r, name)
            assert np.array_equal(got, model(x, r)), (tag, r, name)
    assert torch.equal(xd.cpu(), T(x))                                     # the input is left alone


def test_grey_morphology_at_the_call_site_and_on_odd_layouts():
    """One 1024^2 plane at radius 10 (the vector path: w % 4 == 0), widths that are no multiple of 4 or of the 64 x 32 tile, several planes, every
    radius up to the largest, a non-contiguous input and an empty one."""
    m = CM.face_masks(seeded.facelike_labels(5, 1), (1024, 1024))
    md = T(m).to(DEV)
    for name, fn, model in (("dilate", ops.grey_dilate, CM.grey_dilate), ("erode", ops.grey_erode, CM.grey_erode)):
        assert np.array_equal(fn(md, 10).cpu().numpy(), model(m, 10)), name
    x = CM.morph_input((2, 3, 70, 131), seed=5)
    xd = T(x).to(DEV)
    for r in (3, 16):
        assert np.array_equal(ops.grey_dilate(xd, r).cpu().numpy(), CM.grey_dilate(x, r)), r
        assert np.array_equal(ops.grey_erode(xd, r).cpu().numpy(), CM.grey_erode(x, r)), r
    y = CM.morph_input((1, 1, 40, 68), seed=6)                             # w % 4 == 0 but not a multiple of the tile
    assert np.array_equal(ops.grey_erode(T(y).to(DEV), 5).cpu().numpy(), CM.grey_erode(y, 5))
    assert np.array_equal(ops.grey_dilate(T(y).to(DEV)[..., 4:], 4).cpu().numpy(), CM.grey_dilate(y[..., 4:], 4))       # a strided view
    assert np.array_equal(ops.grey_dilate(T(y[0, 0]).to(DEV), 2).cpu().numpy(), CM.grey_dilate(y[0, 0], 2))             # a bare [H, W] plane
    assert ops.grey_dilate(torch.zeros(0, 1, 8, 8, device=DEV), 2).shape == (0, 1, 8, 8)


# ------------------------------------------------------------------------------------------------ statistics and the map
def _fixture_batch():
    """The three fixture pairs as one batch: uint8 [3, 192, 192, 3] frames, float32 [3, 1, 192, 192] masks."""
    d, t, md, mt = zip(*(CM.ct_pair(i) for i in range(CM.CT_PAIRS)))
    return np.stack(d), np.stack(t), np.stack(md)[:, None, :, :, 0], np.stack(mt)[:, None, :, :, 0]


def _ragged_batch():
    """[2, 37, 53, 3]: a pixel count (1961) that is no multiple of 4 or of a chunk.  Image 0: an all-zero source mask; image 1: all-ones masks."""
    rs = np.random.RandomState(77)
    d, t = rs.randint(0, 256, (2, 37, 53, 3)).astype(np.uint8), rs.randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    md, mt = rs.rand(2, 1, 37, 53).astype(np.float32), rs.rand(2, 1, 37, 53).astype(np.float32)
    md[0], md[1], mt[1] = 0.0, 1.0, 1.0
    return d, t, md, mt


def _model_coefficients(d, t, md, mt, mode):
    out = []
    for b in range(d.shape[0]):
        a, mu0, mu1 = CM.coefficients(CM.inner(d[b], md[b, 0, :, :, None]), CM.inner(t[b], mt[b, 0, :, :, None]), mode)
        out.append(np.concatenate([a.reshape(-1), mu0, mu1]))
    return np.stack(out)


@pytest.mark.parametrize("mode", CM.MODES)
@pytest.mark.parametrize("batch", ["ragged_2x37x53", "fixture_3x192x192"])
def test_moments_and_solve_against_the_float64_model(batch, mode):
    d, t, md, mt = _ragged_batch() if batch.startswith("ragged") else _fixture_batch()
    args = [T(a).to(DEV) for a in (d, t, md, mt)]
    coef = ops.color_transfer_coefficients(*args, mode)
    assert coef.shape == (d.shape[0], 15) and coef.dtype == torch.float64
    again = ops.color_transfer_coefficients(*args, mode)
    assert torch.equal(coef, again)                                        # no atomics: bitwise reproducible
    got, want = coef.cpu().numpy(), _model_coefficients(d, t, md, mt, mode)
    assert np.isfinite(got).all()
    for b in range(d.shape[0]):
        a_err = np.abs(got[b, :9] - want[b, :9]).max() / np.linalg.norm(want[b, :9].reshape(3, 3), 2)
        mu_err = np.abs(got[b, 9:] - want[b, 9:]).max()
        print(f"{batch} image {b} {mode}: map error / |A| = {a_err:.2e}, offsets max-abs {mu_err:.2e}, |A| = {np.linalg.norm(want[b, :9].reshape(3, 3), 2):.3g}")
        record_parity(f"colortransfer.{batch}.{b}.{mode}.map_rel", a_err, MAP_REL)
        record_parity(f"colortransfer.{batch}.{b}.{mode}.offsets_max_abs", mu_err, MAP_REL)
        assert a_err <= MAP_REL and mu_err <= MAP_REL, (batch, b, mode, a_err, mu_err)


@pytest.mark.parametrize("mode", CM.MODES)
def test_empty_masks_give_finite_coefficients(mode):
    d, t, md, mt = _ragged_batch()
    zero = np.zeros_like(md)
    for ms, mtt in ((zero, mt), (md, zero), (zero, zero)):
        coef = ops.color_transfer_coefficients(T(d).to(DEV), T(t).to(DEV), T(ms).to(DEV), T(mtt).to(DEV), mode)
        assert torch.isfinite(coef).all()
        composed, q = ops.skin_color_transfer(T(d).to(DEV), T(t).to(DEV), T(ms).to(DEV), T(mtt).to(DEV), mode)
        assert torch.isfinite(composed).all()
    assert torch.equal(composed, T(d).to(DEV).permute(0, 3, 1, 2).float())     # an empty source mask leaves the face as it is
    e = ops.skin_color_transfer(T(d[:0]).to(DEV), T(t[:0]).to(DEV), T(md[:0]).to(DEV), T(mt[:0]).to(DEV), mode)
    assert e[0].shape == (0, 3, 37, 53) and e[1].shape == (0, 37, 53, 3)


# ------------------------------------------------------------------------------------------------ the quantised transfer and the composition
def _compose_planar(d, q, md):
    return np.stack([CM.compose(d[b], q[b], md[b, 0, :, :, None]) for b in range(d.shape[0])]).transpose(0, 3, 1, 2)


@pytest.fixture(scope="module")
def q_step():
    """``ops.skin_color_transfer`` on the fixture pairs, once per module: mode -> (composed, q, share of bytes that differ from the reference's)."""
    g = load_golden("g19_color_transfer")
    d, t, md, mt = _fixture_batch()
    out = {}
    for mode in CM.MODES:
        composed, q = ops.skin_color_transfer(*(T(a).to(DEV) for a in (d, t, md, mt)), mode)
        ref = np.stack([g[f"ct.p{i}.{mode}.q"] for i in range(CM.CT_PAIRS)])
        diff = np.abs(q.cpu().numpy().astype(np.int32) - ref.astype(np.int32))
        out[mode] = (composed.cpu().numpy(), q.cpu().numpy(), diff, float((diff > 0).mean()))
    return out


@pytest.mark.parametrize("mode", CM.MODES)
def test_skin_color_transfer_against_the_reference_bytes(q_step, mode):
    d, t, md, mt = _fixture_batch()
    composed, q, diff, share = q_step[mode]
    print(f"skin_color_transfer {mode}: max {diff.max()} level, share of differing bytes {share:.2e}")
    record_parity(f"colortransfer.q.{mode}.max_abs_levels", int(diff.max()), 1)
    record_parity(f"colortransfer.q.{mode}.share_differing", share, MAX_SHARE)
    assert q.shape == d.shape and q.dtype == np.uint8 and diff.max() <= 1 and share <= MAX_SHARE, (diff.max(), share)
    want = _compose_planar(d, q, md)
    assert composed.dtype == np.float32 and composed.shape == want.shape and np.array_equal(composed, want)      # numpy's float32 bits
    only = ops.skin_color_transfer(*(T(a).to(DEV) for a in (d, t, md, mt)), mode, with_q=False)
    assert only[1] is None and np.array_equal(only[0].cpu().numpy(), composed)


@pytest.mark.parametrize("mode", CM.MODES)
def test_skin_color_transfer_on_a_ragged_shape(mode):
    """The scalar path (h w % 4 != 0) against the model: q within one level on at most 1e-3 of the bytes, the composition bit for bit."""
    d, t, md, mt = _ragged_batch()
    md[0] = np.random.RandomState(3).rand(1, 37, 53).astype(np.float32)
    composed, q = ops.skin_color_transfer(*(T(a).to(DEV) for a in (d, t, md, mt)), mode)
    q = q.cpu().numpy()
    want = np.stack([CM.skin_color_transfer(d[b], t[b], md[b, 0, :, :, None], mt[b, 0, :, :, None], mode)[1] for b in range(2)])
    diff = np.abs(q.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1 and (diff > 0).mean() <= MAX_SHARE, (diff.max(), (diff > 0).mean())
    assert np.array_equal(composed.cpu().numpy(), _compose_planar(d, q, md))


# ------------------------------------------------------------------------------------------------ masks
def test_soft_expansion_masks_against_the_restatement():
    m = np.concatenate([CM.soft_mask(128, 61), CM.morph_input((1, 1, 128, 128), seed=62)])
    assert ((m > 0) & (m < 1)).any() and (m == 0).any() and (m == 1).any()
    radius = 10
    content, border, full = ops.soft_expansion_masks(T(m).to(DEV), radius)
    dil, ero = CM.grey_dilate(m, radius), CM.grey_erode(m, radius)
    b = Bars(np.concatenate([dil, ero, m], axis=1), 15, 0.6, 1)
    assert b.band_share < BAND_SHARE
    s64, ok = b.soft64, ~b.band
    got = np.concatenate([full.cpu().numpy(), border.cpu().numpy(), content.cpu().numpy()], axis=1)
    want = np.concatenate([s64[:, 0:1], np.clip(s64[:, 0:1] - s64[:, 1:2], 0, 1), s64[:, 2:3]], axis=1)
    keep = np.stack([ok[:, 0], ok[:, 0] & ok[:, 1], ok[:, 2]], axis=1)
    for i, (name, scale) in enumerate((("full", 1), ("border", 2), ("content", 1))):      # border is a difference of two soft masks
        dlt = float(np.abs(got[:, i] - want[:, i])[keep[:, i]].max())
        record_parity(f"colortransfer.masks.r{radius}.{name}_max_abs", dlt, scale * b.tol)
        assert dlt <= scale * b.tol, (name, dlt, b.tol)
    r32 = CM.soft_expansion_masks(m, radius)
    assert max(float(np.abs(a.cpu().numpy() - r)[keep[:, j:j + 1]].max()) for a, r, j in ((content, r32[0], 2), (border, r32[1], 1), (full, r32[2], 0))) <= 2 * b.tol
    empty = ops.soft_expansion_masks(torch.zeros(0, 1, 16, 16, device=DEV), 3)
    assert all(t.shape == (0, 1, 16, 16) for t in empty)


# ------------------------------------------------------------------------------------------------ pipeline
def _chain_inputs():
    d, t, _, _ = CM.ct_pair(0, 1024)
    return d[None], t[None], seeded.facelike_labels(5, 1), seeded.facelike_labels(6, 1)


@pytest.mark.parametrize("mode", CM.MODES)
def test_color_transfer_chain_against_the_restatement(q_step, mode):
    """pipeline.color_transfer = _color_transfer:537-572 against the model chain (face masks -> soft expansion border -> transfer -> composition -> the
    oracle's multi-band blend).  The share of differing bytes is bounded by the q step's measured share plus paste_back_soft's recorded 4.6e-4."""
    d, t, ld, lt = _chain_inputs()
    dd, td, ldd, ltd = (T(a).to(DEV) for a in (d, t, ld, lt))
    out = pipeline.color_transfer(dd, td, ldd, ltd, mode)
    assert out.shape == d.shape and out.dtype == torch.uint8
    if mode == "lct":
        assert torch.equal(out, pipeline.color_transfer(dd, td, ldd, ltd))          # the default mode
    out = out.cpu().numpy()
    ref = CM.color_transfer(d, t, ld, lt, mode)
    diff = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    share, bound = float((diff > 0).mean()), q_step[mode][3] + PASTE_BACK_SOFT_SHARE
    print(f"color_transfer chain {mode}: max {diff.max()} level, share of differing bytes {share:.2e} (bound {bound:.2e} = q step {q_step[mode][3]:.2e} + 4.6e-4)")
    record_parity(f"colortransfer.chain.{mode}.max_abs_levels", int(diff.max()), 1)
    record_parity(f"colortransfer.chain.{mode}.share_differing", share, bound)
    assert diff.max() <= 1, diff.max()
    assert share <= bound, f"share of differing bytes {share:.3e} exceeds the q step's {q_step[mode][3]:.3e} + paste_back_soft's 4.6e-4"
    assert (out != d).any() and (out != t).any()
    if mode == "lct":
        # an empty swapped map: no face to recolour, the swapped face comes back (through the float pyramid of the blend: within one level)
        none = pipeline.color_transfer(dd, td, torch.zeros_like(ldd), ltd, mode).cpu().numpy().astype(np.int32)
        assert np.abs(none - d).max() <= 1


def test_color_transfer_inside_graph_capture():
    """No host synchronisation anywhere in the chain: capture on one stream + replay gives the eager bits."""
    d, t, ld, lt = (T(a).to(DEV) for a in _chain_inputs())
    for mode in CM.MODES:
        eager, out = _capture(lambda: pipeline.color_transfer(d, t, ld, lt, mode))
        assert torch.equal(out, eager), mode


@pytest.fixture(scope="module")
def parser(bisenet_sd):
    install_dropin()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    p = FaceParser(seg_ckpt=None, device=DEV)
    p.seg.load_state_dict(bisenet_sd)
    p.seg.eval()
    return p


def test_swap_images_with_ct_mode_bs2(gpu_net3, parser):
    import align_model as M
    rng = np.random.default_rng(15)
    frames = np.stack([M.make_frame(rng, 1080, 1920) for _ in range(2)])
    quads = np.stack([M.square_quad(960, 540, 300, 0.35), M.square_quad(1800, 120, 380, -0.5)])
    plan = align.crop_plan(quads, (1080, 1920), 1024)
    driven = seeded.seeded_image(16, 2, 1024).to(DEV)
    fr = T(frames).to(DEV)
    got = pipeline.swap_images(gpu_net3, parser, driven, fr, plan, ct_mode="lct")
    assert got.shape == fr.shape and got.dtype == torch.uint8 and torch.equal(fr.cpu(), T(frames))
    g = got.cpu().numpy()
    plain = pipeline.swap_images(gpu_net3, parser, driven, fr, plan).cpu().numpy()
    for i in range(2):
        x0, y0, x1, y1 = plan.paste_boxes[i].tolist()
        outside = _outside_quad(np.asarray(plan.quads[i], dtype=np.float64), g.shape[1], g.shape[2])
        outside[:y0], outside[y1:], outside[:, :x0], outside[:, x1:] = True, True, True, True
        assert np.array_equal(g[i][outside], frames[i][outside])             # every pixel outside the quads untouched
        assert (g[i][~outside] != plain[i][~outside]).any()                  # and another face inside them than without the colour transfer
    # the same chain through recolor_fn, fed the maps swap_batch hands out
    crops = ops.crop_align(fr, plan)
    _, lab, extra = pipeline.swap_batch(gpu_net3, parser, driven, ops.frames_to_tensor(crops), mask_surgery=True, ear_interpolation=False,
                                        comp_indices=pipeline.IMAGE_COMP_INDICES_CT)
    assert extra["target_labels"].shape == lab.shape and extra["target_labels"].dtype == torch.uint8
    via_fn = pipeline.swap_images(gpu_net3, parser, driven, fr, plan,
                                  recolor_fn=lambda s, c: pipeline.color_transfer(s, c, lab, extra["target_labels"], "lct"))
    assert torch.equal(got, via_fn)
    mkl = pipeline.swap_images(gpu_net3, parser, driven, fr, plan, ct_mode="mkl").cpu().numpy()
    assert mkl.shape == g.shape and np.array_equal(mkl[1][outside], frames[1][outside])          # (`outside`: the second image's, from the loop above)
