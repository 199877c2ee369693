"""Row f23 (the tiled Real-ESRGAN x2 step of ``CodeFormerInfer.infer_image``) without a GPU: the restatement ``esrgan_tile_model`` against what the reference's
own ``RealESRGANer`` gave (tests/golden/g33_esrgan_tile.npz), the bars of the GPU tests pinned from the other side by single-change mutants, ``ops.esrgan_tiles``
against the model's geometry, the Lanczos4 resize on properties that need no cv2, the host tables of ``ops_esrgan`` against the model's, the names, and the
argument errors that must raise before any launch.

The bound of a case is ``gpen_sr_model.bound``: ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64; uint8 images follow
``gpen_sr_model.check_u8``."""
import os

import numpy as np
import pytest
import torch

import esrgan_tile_model as M
from conftest import GOLDEN

ENTRY_POINTS = {"e4s_esrt_input", "e4s_esrt_tail", "e4s_cv_resize_lanczos4_u8"}
NAMES = ("ESRGAN_SCALE", "ESRGAN_TILE", "ESRGAN_TILE_PAD", "ESRGAN_PRE_PAD", "esrgan_tiles", "esrgan_enhance", "cv_resize_lanczos4")
OUT_KEYS = {2: "out2", None: "out_none", 1.5: "out1p5"}
HALF_TAPS = (-26, 122, -340, 1267, 1267, -340, 122, -26)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "g33_esrgan_tile.npz")) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ names
def test_names_and_entry_points():
    from e4s2024_amd import _lib, ops, ops_esrgan, pipeline
    assert set(ops_esrgan.__all__) == set(NAMES) and all(getattr(ops, n) is getattr(ops_esrgan, n) for n in NAMES)
    assert ENTRY_POINTS <= set(_lib.declared_symbols())
    assert callable(pipeline.codeformer_enhance) and callable(pipeline.recolor_frames)
    assert (ops.ESRGAN_SCALE, ops.ESRGAN_TILE, ops.ESRGAN_TILE_PAD, ops.ESRGAN_PRE_PAD) == (4, 400, 40, 0)
    with open(_lib.HEADER) as f:
        assert "/* f23:" in f.read()


# ------------------------------------------------------------------------------------------------ the model against the reference
@pytest.mark.parametrize("tag", list(M.GOLDEN_CASES))
def test_model_against_the_reference(golden, tag):
    """The float64 model against the reference's float32 ``post_process`` output within the bound; the reference's uint8 results under the uint8 rule and, for the
    resized ones, bit for bit the model's Lanczos4 of the reference's own x4 image; the model alone is conditioned (why CASE_SEED is what it is)."""
    H, W, tile, tile_pad, pre_pad = M.GOLDEN_CASES[tag]
    c = M.golden_case(tag)
    assert np.array_equal(golden[f"{tag}.img"], c["img"]) and c["img"].shape == (H, W, 3)
    r32 = golden[f"{tag}.r"]
    err, b = M.max_err(r32, c["r"][0]), M.bound(c["e32"], c["r"])
    big = golden[f"{tag}.out_none"]
    strict, clamped, std = M.check_u8(big, c["u"], c["e32"])
    mstrict, mclamped, mstd = M.conditioned(c)
    print(f"{tag}: err {err:.3e} = {err / c['e32']:.2f} e32, bound {b:.3e}; strict {100 * strict:.2f} %, clamped {100 * clamped:.2f} %, std {std:.1f}; "
          f"the model alone: strict {100 * mstrict:.2f} %, clamped {100 * mclamped:.2f} %, std {mstd:.1f}")
    assert r32.shape == (3, 4 * H, 4 * W) and err <= b
    assert strict >= 0.99 and clamped < 0.10 and std > 30
    assert mstrict >= 0.99 and mclamped < 0.10 and mstd > 30
    for outscale in M.GOLDEN_OUTSCALES:
        got, dsize = golden[f"{tag}.{OUT_KEYS[outscale]}"], M.out_size(H, W, outscale)
        want = big if dsize is None else M.resize_lanczos4(big, dsize)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), outscale
        # and the model's own chain, end to end, within one grey level of an x4 pixel spread through eight taps (its positive coefficients sum to under 1.36 per axis)
        mine = M.enhance(c["sd"], c["img"], outscale, tile, tile_pad, pre_pad)
        assert mine.shape == got.shape and np.abs(mine.astype(int) - got.astype(int)).max() <= (1 if dsize is None else 2)


def test_golden_is_small(golden):
    size = os.path.getsize(os.path.join(GOLDEN, "g33_esrgan_tile.npz"))
    assert size < max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz") and not f.startswith("g33_")) and size < 1 << 20
    assert len(golden) == 5 * len(M.GOLDEN_CASES)


# ------------------------------------------------------------------------------------------------ the mutants
@pytest.mark.parametrize("mutant", M.TILE_MUTANTS)
def test_tile_mutants_move_the_model(mutant):
    """Every single-change mutant of the tile path moves the float64 x4 output by at least MUTANT_MARGIN bounds on some golden case (``half_up``: the uint8 image,
    on the float32 values that are exact ties)."""
    if mutant == "half_up":
        ties = M.SM.tie_values()
        r = np.broadcast_to(ties[None, None, None, :], (1, 3, 1, len(ties))).copy()
        assert (M.to_u8(r)[1] != M.to_u8(r, mutant)[1]).any() and len(ties) > 50
        return
    worst = 0.0
    for tag, (H, W, tile, tile_pad, pre_pad) in M.GOLDEN_CASES.items():
        c = M.golden_case(tag)
        moved = M.max_err(M.x4(c["sd"], c["img"], tile, tile_pad, pre_pad, mutant=mutant)[0], c["r"]) / M.bound(c["e32"], c["r"])
        print(f"{mutant} on {tag}: {moved:.1f} bounds")
        worst = max(worst, moved)
    assert worst >= M.MUTANT_MARGIN


@pytest.mark.parametrize("mutant", M.LANCZOS_MUTANTS)
def test_lanczos_mutants_move_the_resize(mutant):
    """Every single-change mutant of the integer resize moves some pixel of some case by at least one grey level."""
    worst = 0
    for H, W, Ho, Wo in M.RESIZE_CASES:
        img = M.resize_image(H, W)
        worst = max(worst, int(np.abs(M.resize_lanczos4(img, (Wo, Ho), mutant).astype(int) - M.resize_lanczos4(img, (Wo, Ho)).astype(int)).max()))
    print(f"{mutant}: {worst} grey levels")
    assert worst >= 1


# ------------------------------------------------------------------------------------------------ the geometry
def test_esrgan_tiles_equals_the_model():
    from e4s2024_amd import ops
    n = 0
    for H in range(1, 14):
        for W in range(1, 14):
            for tile in (0, 1, 4, 5, 400):
                for pad in (0, 1, 2, 40):
                    got = ops.esrgan_tiles(H, W, tile, pad)
                    assert got == M.tiles(H, W, tile, pad), (H, W, tile, pad)
                    # the kept windows tile the x4 image exactly once, and each lies in its tile's output
                    cover = np.zeros((4 * H, 4 * W), int)
                    for (y0, y1, x0, x1), (oy0, oy1, ox0, ox1), (Y0, X0) in got:
                        assert 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W and 0 <= oy0 < oy1 <= 4 * (y1 - y0) and 0 <= ox0 < ox1 <= 4 * (x1 - x0)
                        cover[Y0:Y0 + oy1 - oy0, X0:X0 + ox1 - ox0] += 1
                    assert (cover == 1).all()
                    n += len(got)
    assert n > 10000
    assert ops.esrgan_tiles(512, 512) == ops.esrgan_tiles(512, 512, 400, 40) and len(ops.esrgan_tiles(512, 512)) == 4
    assert ops.esrgan_tiles(512, 512)[3] == ((360, 512, 360, 512), (160, 608, 160, 608), (1600, 1600))
    for bad in (dict(H=0), dict(W=2.0), dict(tile=None), dict(tile_pad=-1), dict(tile_pad=True)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            ops.esrgan_tiles(**{**dict(H=5, W=5, tile=2, tile_pad=1), **bad})


# ------------------------------------------------------------------------------------------------ the Lanczos4 resize
def test_lanczos_taps():
    assert tuple(M.lanczos4_taps(0.5)) == HALF_TAPS and sum(HALF_TAPS) == 2046
    assert M.lanczos4_taps(0.0) == [0, 0, 0, 2048, 0, 0, 0, 0] and M.lanczos4_taps(np.float32(1e-8)) == [0, 0, 0, 2048, 0, 0, 0, 0]
    idx, taps, f = M.lanczos4_axis(2048, 1024)
    assert (f == 0.5).all() and (taps == np.array(HALF_TAPS)).all() and idx[0].tolist() == [0, 0, 0, 0, 1, 2, 3, 4] and idx[-1].tolist() == [2043, 2044, 2045, 2046, 2047, 2047, 2047, 2047]
    # int32 is enough.  With P / N the sums of the positive / negative taps of a fraction, |h| <= 255 max(P, N) and the vertical sum is largest where the positive
    # taps meet 255 P and the negative ones -255 N: 255 (P P' + N N') + 2^21 < 2^31 over a sweep of the fractions (the issue's 255 * 2778^2 counts P alone)
    sums = [(sum(t for t in taps if t > 0), -sum(t for t in taps if t < 0)) for taps in (M.lanczos4_taps(np.float32(k / 2048)) for k in range(2048))]
    P, N = max(p for p, _ in sums), max(n for _, n in sums)
    print(f"positive taps sum to {P} at the most, negative ones to -{N}")
    assert 2700 < P < 2800 and 255 * (P * P + N * N) + (1 << 21) < 2 ** 31
    # an enlargement keeps its fraction at the border (INTER_LINEAR resets it)
    idx, taps, f = M.lanczos4_axis(5, 12)
    assert f[0] > 0.5 and idx[0].tolist() == [0] * 5 + [1, 2, 3]


def test_lanczos_model_properties():
    for H, W, Ho, Wo in M.RESIZE_CASES:
        img = M.resize_image(H, W)
        got = M.resize_lanczos4(img, (Wo, Ho))
        assert got.shape == (2, Ho, Wo, 3) and got.dtype == np.uint8
        if (H, W) == (Ho, Wo):
            assert np.array_equal(got, img)                                                   # equal size is the identity
        want = np.stack([M.resample_lanczos4_f64(i, (Wo, Ho)) for i in img])
        diff = int(np.abs(got.astype(int) - want.astype(int)).max())
        print(f"{H} x {W} -> {Ho} x {Wo}: {diff} grey levels from the float64 resample")
        assert diff <= 2
    white = np.full((12, 10, 3), 255, np.uint8)
    assert (M.resize_lanczos4(white, (5, 6)) == 255).all() and (M.resize_lanczos4(np.zeros_like(white), (5, 6)) == 0).all()
    assert (255 * 2046 * 2046 + (1 << 21)) >> 22 == 255


def test_host_tables_equal_the_model():
    from e4s2024_amd import ops_esrgan
    for src, dst in ((16, 8), (9, 5), (13, 7), (7, 15), (5, 12), (8, 8), (1, 3), (20, 10), (3, 9), (64, 32), (2048, 1024), (100, 9), (2048, 768)):
        ofs, coef = ops_esrgan._lanczos4_axis(src, dst)
        idx, taps, _ = M.lanczos4_axis(src, dst)
        assert ofs.dtype == np.int32 and coef.dtype == np.int16 and coef.shape == (dst, 8)
        assert np.array_equal(np.clip(ofs[:, None].astype(np.int64) + np.arange(8)[None], 0, src - 1), idx) and np.array_equal(coef.astype(np.int64), taps), (src, dst)


# ------------------------------------------------------------------------------------------------ refusals in front of the device check
def _esr(scale=4, nf=64):
    from e4s2024_amd import ops
    return ops.GpenSRNet(1, nf, scale).eval()


def test_esrgan_enhance_refusals():
    from e4s2024_amd import ops
    net, img = _esr(), torch.zeros((1, 6, 7, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="scale 2"):
        ops.esrgan_enhance(img, _esr(2))
    with pytest.raises(RuntimeError, match="training mode"):
        ops.esrgan_enhance(img, _esr().train())
    with pytest.raises(TypeError, match="module or a mapping"):
        ops.esrgan_enhance(img, 5)
    for bad in (img.float(), img[0], torch.zeros((1, 6, 7, 4), dtype=torch.uint8), torch.zeros((1, 6, 7), dtype=torch.uint8), img.to(torch.int16)):
        with pytest.raises(ValueError, match="uint8"):
            ops.esrgan_enhance(bad, net)
    with pytest.raises(ValueError, match="uint8"):
        ops.esrgan_enhance(img, net, chw=True)                                               # [1, 6, 7, 3] is not planar
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.esrgan_enhance(np.zeros((1, 6, 7, 3), np.uint8), net)
    for kw in (dict(tile=4.0), dict(tile=True), dict(tile_pad=-1), dict(tile_pad=1.5), dict(pre_pad=-2), dict(pre_pad="3")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ops.esrgan_enhance(img, net, **kw)
    for outscale in (0, -1, float("nan"), float("inf"), "2", True, 0.1):                      # (0.1 takes 6 x 7 to 0 x 0)
        with pytest.raises(ValueError, match="outscale"):
            ops.esrgan_enhance(img, net, outscale=outscale)
    for pre_pad in (6, 7, 100):
        with pytest.raises(ValueError, match="reflect"):
            ops.esrgan_enhance(img, net, pre_pad=pre_pad)
    with pytest.raises(ValueError, match="16384"):
        ops.esrgan_enhance(torch.zeros((1, 4097, 8, 3), dtype=torch.uint8), net)
    with pytest.raises(ValueError, match="16384"):
        ops.esrgan_enhance(torch.zeros((1, 8, 4090, 3), dtype=torch.uint8), net, pre_pad=7)
    # everything else in order: the one refusal left is the device's
    for kw in (dict(), dict(outscale=2), dict(outscale=4), dict(outscale=1.5, tile=0, pre_pad=5), dict(tile=-3)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            ops.esrgan_enhance(img, net, **kw)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.esrgan_enhance(img.permute(0, 3, 1, 2), net.state_dict(), chw=True)


def test_cv_resize_lanczos4_refusals():
    from e4s2024_amd import ops
    img = torch.zeros((1, 6, 7, 3), dtype=torch.uint8)
    for bad in (img.float(), img[0], torch.zeros((1, 6, 7, 1), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            ops.cv_resize_lanczos4(bad, (3, 3))
    for dsize in (3, (3,), (3, 3, 3), (0, 3), (3, 16385), (3.0, 3), (True, 3), None):
        with pytest.raises(ValueError, match="dsize"):
            ops.cv_resize_lanczos4(img, dsize)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.cv_resize_lanczos4(img, (3, 3))


def test_pipeline_refusals():
    from e4s2024_amd import ops, pipeline
    cf, esr = ops.CodeFormer(64, 2, 1, 40, 256).eval(), _esr()
    faces = torch.zeros((1, 3, 512, 512), dtype=torch.uint8)
    with pytest.raises(TypeError, match="w must be"):
        pipeline.codeformer_enhance(cf, esr, faces, w=torch.tensor(0.8))
    for upscale in (0, float("nan"), "2", True):
        with pytest.raises(ValueError, match="upscale"):
            pipeline.codeformer_enhance(cf, esr, faces, upscale=upscale)
    with pytest.raises(ValueError, match="scale 2"):
        pipeline.codeformer_enhance(cf, _esr(2), faces)
    with pytest.raises(RuntimeError, match="training mode"):
        pipeline.codeformer_enhance(cf, _esr().train(), faces)
    with pytest.raises(ValueError, match="faces_u8"):
        pipeline.codeformer_enhance(cf, esr, faces.float())
    with pytest.raises(ValueError, match="faces_u8"):
        pipeline.codeformer_enhance(cf, esr, faces.permute(0, 2, 3, 1))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        pipeline.codeformer_enhance(cf, esr, faces)

    class Parser:
        def parse_batch(self, x, seg12=True):
            raise AssertionError("a launch before the checks were through")

    sw, tg = torch.zeros((1, 32, 32, 3), dtype=torch.uint8), torch.zeros((1, 20, 24, 3), dtype=torch.uint8)
    for a, b in ((sw.float(), tg), (sw, tg[0]), (sw[..., :2], tg), (sw, tg.permute(0, 3, 1, 2))):
        with pytest.raises(ValueError, match="crops"):
            pipeline.recolor_frames(Parser(), None, cf, esr, a, b)
    with pytest.raises(ValueError, match="square"):
        pipeline.recolor_frames(Parser(), None, cf, esr, tg, tg)
    with pytest.raises(ValueError, match="2 target crops"):
        pipeline.recolor_frames(Parser(), None, cf, esr, sw, torch.cat([tg, tg]))
    with pytest.raises(TypeError, match="parse_batch"):
        pipeline.recolor_frames(object(), None, cf, esr, sw, tg)
    with pytest.raises(TypeError, match="latest_netG"):
        pipeline.recolor_frames(Parser(), 5, cf, esr, sw, tg)
