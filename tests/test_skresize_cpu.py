"""Row f24 (skimage's float64 resize in front of the reenactment, the uint8 frames behind it) without a GPU: the restatement ``skresize_model`` against what
``scipy.ndimage`` gave for skimage's ``resize`` body (tests/golden/g34_skresize.npz), the mutants, the host tables of ``ops.sk_resize_tables`` against the
model's and against the golden, the tap counts and row sums, the names, and the refusals that need no device.

The bound of the model against the golden, 2^-47: an output is at most 24 + 24 taps per axis with non-negative weights of sum 1 on values in [0, 1], under 64
roundings of 2^-53 each whichever way the sums are ordered."""
import os

import numpy as np
import pytest
import torch

import skresize_model as M

BOUND = 2.0 ** -47
TOLD = 1e-6
NAMES = ("SK_MAX_SIDE", "SK_MAX_TAPS", "sk_resize_tables", "sk_resize", "frames_u8")
ENTRY_POINTS = {"e4s_sk_resize_u8": 18, "e4s_frames_u8": 7}
AXES = ((1024, 256), (37, 8), (29, 8), (45, 7), (45, 44), (64, 64), (48, 48), (20, 32), (24, 40), (400, 8), (9, 8), (128, 32), (1, 3), (5, 1), (7, 1), (2, 5), (3, 4))


@pytest.fixture(scope="module")
def golden():
    return M.golden()


def test_names_and_abi():
    from e4s2024_amd import _lib, ops, ops_sk, pipeline
    assert set(ops_sk.__all__) == set(NAMES) and all(getattr(ops, n) is getattr(ops_sk, n) for n in NAMES)
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    lib = _lib.lib()
    assert all(hasattr(lib.cdll, n) for n in ENTRY_POINTS)
    assert {n: len(_lib._PROTOS[n]) for n in ENTRY_POINTS} == ENTRY_POINTS
    with open(_lib.HEADER) as f:
        src = f.read()
    assert "/* f24:" in src and _lib.ABI_VERSION == 1 and ops.SK_MAX_TAPS == _lib._DEFINES["E4S_SK_MAX_TAPS"] == 1024
    assert callable(pipeline.reenact_drivens) and callable(pipeline.reenact_recolor_clip)


def test_the_golden_file_is_small_and_holds_the_cases(golden):
    assert os.path.getsize(M.GOLDEN) < 64 * 1024
    for case in M.GOLDEN_CASES:
        img, out = golden[M.tag(case)]
        assert img.dtype == np.uint8 and img.shape == (case[0], case[1], 3) and np.array_equal(img, M.image_u8(case))
        assert out.dtype == np.float64 and out.shape == (case[2], case[3], 3)


@pytest.mark.parametrize("case", M.GOLDEN_CASES, ids=M.tag)
def test_model_against_scipy(golden, case):
    img, want = golden[M.tag(case)]
    got = M.resize(img, case[2:])
    err = float(np.abs(got - want).max())
    differing = int((got.astype(np.float32) != want.astype(np.float32)).sum())
    print(f"{M.tag(case)}: model - scipy {err:.3e}, float32 values that differ {differing}")
    assert err <= BOUND
    assert differing == 0                                                                     # the seed's condition: the GPU bar is measured against the model
    assert want.min() >= img.min() / 255.0 and want.max() <= img.max() / 255.0


@pytest.mark.parametrize("case", M.GOLDEN_CASES, ids=M.tag)
def test_composed_tables_against_scipy(golden, case):
    """The kernel's form — composite tables, x first, ascending taps — on the model's tables and on ``ops.sk_resize_tables``'s."""
    from e4s2024_amd import ops
    img, want = golden[M.tag(case)]
    H, W, Ho, Wo = case
    for what, ytab, xtab in (("model", None, None), ("ops", ops.sk_resize_tables(H, Ho), ops.sk_resize_tables(W, Wo))):
        err = float(np.abs(M.resize_composed(img, (Ho, Wo), ytab, xtab) - want).max())
        print(f"{M.tag(case)}: composed ({what} tables) - scipy {err:.3e}")
        assert err <= BOUND


def test_identity_is_exact(golden):
    img, want = golden["16x12_16x12"]
    assert np.array_equal(want, img / 255.0) and np.array_equal(M.resize(img, (16, 12)), img / 255.0)


@pytest.mark.parametrize("src,dst", AXES, ids=lambda v: str(v))
def test_tables_of_ops_and_model_agree(src, dst):
    from e4s2024_amd import ops
    start, count, weight = ops.sk_resize_tables(src, dst)
    ms, mc, mw = M.tables(src, dst)
    assert start.dtype == np.int32 and count.dtype == np.int32 and weight.dtype == np.float64 and weight.shape == (dst, int(count.max()))
    assert np.array_equal(start, ms) and np.array_equal(count, mc) and weight.shape == mw.shape
    assert np.abs(weight - mw).max() <= 2.0 ** -50
    assert start.min() >= 0 and (start + count).max() <= src and count.min() >= 1            # no tap leaves the source
    assert np.abs(weight.sum(axis=1) - 1).max() <= 2.0 ** -50 and weight.min() >= 0
    assert all((weight[o, count[o]:] == 0).all() for o in range(dst))
    assert ops.sk_resize_tables(src, dst)[2] is weight and not weight.flags.writeable         # made once, kept


def test_tap_counts():
    from e4s2024_amd import ops
    taps = lambda a, b: ops.sk_resize_tables(a, b)[2].shape[1]                                # noqa: E731
    assert taps(1024, 256) == 14                                                              # sigma 1.5, radius 6: 13 + 1
    assert (taps(37, 8), taps(29, 8)) == (16, 12)
    assert taps(45, 7) == 24
    assert taps(45, 44) == 2 and taps(64, 64) == 1 and taps(20, 32) == 2 and taps(256, 1024) == 2
    assert M.gaussian_weights(1.5)[0] == 6 and M.gaussian_weights((45 / 7 - 1) / 2)[0] == 11
    assert taps(400, 8) == 198                                                                # beyond the LDS plan's 80 rows: the direct form


CLIP_MUTANTS = ("no_clip", "clip_per_channel")


@pytest.mark.parametrize("mutant", [m for m in M.MUTANTS if m not in CLIP_MUTANTS])
def test_mutants_are_told_apart(golden, mutant):
    """Each single change moves some stored case by TOLD = 1e-6 or more, sixteen times the GPU bar of one float32 ulp (6e-8; dropping the outermost tap of a
    Gaussian at 4 sigma moves 4e-5, the smallest of them): none of them passes for the rule on the device."""
    worst = {}
    for case in M.GOLDEN_CASES:
        img, want = golden[M.tag(case)]
        worst[M.tag(case)] = float(np.abs(M.resize(img, case[2:], mutant) - want).max())
    print(mutant, {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) > TOLD
    told = [k for k, v in worst.items() if v > TOLD]
    assert len(told) >= 2 or mutant == "radius_floor", told                                   # (the radius differs only where 4 sigma has a fraction >= 0.5)


def test_mutants_where_each_must_show(golden):
    diff = lambda t, m: float(np.abs(M.resize(golden[t][0], golden[t][1].shape[:2], m) - golden[t][1]).max())      # noqa: E731
    assert diff("10x12_16x20", "reflect") > 1e-3 and diff("37x29_8x8", "reflect") > 1e-4      # the fold at the ends of an enlargement and under the Gaussian
    assert diff("45x45_44x7", "radius_floor") > 1e-5                                          # 4 sigma = 10.86: radius 11, not 10
    assert diff("128x8_32x2", "gauss_unnormalised") > 1e-3
    assert diff("10x12_16x20", "no_half_pixel") > 1e-2 and diff("128x8_32x2", "no_half_pixel") > 1e-2
    assert diff("128x8_32x2", "sigma_half_factor") > 1e-3


def test_clip_mutants_are_told_apart_in_the_bits(golden):
    """The composite weights are non-negative with sum one: without the clip a result leaves the image's range by the roundings of its sums alone, so the two clip
    mutants stay within 2^-47 of the rule everywhere and are told from it by exact float64 comparisons on the two special cases."""
    for case in M.GOLDEN_CASES:
        for mutant in CLIP_MUTANTS:
            assert np.abs(M.resize(golden[M.tag(case)][0], case[2:], mutant) - golden[M.tag(case)][1]).max() <= BOUND
    img, want = golden["flat200"]
    assert np.array_equal(img, M.special_u8("flat200")) and (want == 200 / 255.0).all()       # scipy's sums do not give 200 / 255 back: the clip does
    assert (M.resize(img, (3, 3)) == 200 / 255.0).all()
    assert (M.resize(img, (3, 3), "no_clip") != 200 / 255.0).any()
    assert (M.resize(img, (3, 3), "clip_per_channel") == 200 / 255.0).all()
    img, want = golden["chan100"]
    assert np.array_equal(img, M.special_u8("chan100")) and (img[..., 0] == 100).all() and img[..., 1:].min() < 100 < img[..., 1:].max()
    assert np.abs(M.resize(img, (3, 3)) - want).max() <= BOUND
    assert (want[..., 0] != 100 / 255.0).any() and (M.resize(img, (3, 3))[..., 0] != 100 / 255.0).any()      # the image-wide clip leaves the roundings
    assert (M.resize(img, (3, 3), "clip_per_channel")[..., 0] == 100 / 255.0).all()            # a per-channel clip would not


def test_frames_u8_model():
    v = M.frame_values(2, 5, 7)
    assert v.dtype == np.float32 and v.min() == 0 and v.max() == 1 and np.float32(1 - 2.0 ** -24) in v
    u = M.frames_u8(v)
    assert u.shape == (2, 5, 7, 3) and u.dtype == np.uint8 and np.array_equal(M.frames_u8(v, flip=True), u[..., ::-1])
    assert M.frames_u8(np.float32([[[[1.0]], [[1 - 2.0 ** -24]], [[0.0]]]]))[0, 0, 0].tolist() == [255, 254, 0]
    k = (np.arange(256) / 255).astype(np.float32)
    at = lambda a: M.frames_u8(np.broadcast_to(a, (1, 3, 1, 256)).copy())[0, 0, :, 0].astype(int)          # noqa: E731
    assert np.array_equal(at(k), np.arange(256))                                              # float32(k / 255) * 255 rounds to k in float32 ...
    assert np.array_equal(at(np.nextafter(k, np.float32(-1)))[1:], np.arange(255))            # ... and its neighbour below truncates to k - 1


def test_refusals_that_need_no_device():
    from e4s2024_amd import ops
    with pytest.raises(ValueError, match="1024 at the most"):
        ops.sk_resize_tables(16384, 8)
    for bad in ((0, 4), (4, 0), (4.0, 4), (True, 4), (4, 16385), ("4", 4)):
        with pytest.raises(ValueError, match="is an int in 1..16384"):
            ops.sk_resize_tables(*bad)
    img = torch.zeros((2, 9, 7, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="sk_resize: img_u8 must be a CUDA tensor"):
        ops.sk_resize(img, (4, 4))
    for bad in (img.float(), img[0], img[..., :2], torch.zeros((1, 0, 7, 3), dtype=torch.uint8), img.permute(0, 3, 1, 2)):
        with pytest.raises(ValueError, match="uint8 .bs, H, W, 3. image batch"):
            ops.sk_resize(bad, (4, 4))
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.sk_resize(img.numpy(), (4, 4))
    for bad in (4, (4,), (4, 4, 3), (4.0, 4), (0, 4), (4, 16385), (True, 4), None):
        with pytest.raises(ValueError, match="size is a pair"):
            ops.sk_resize(img, bad)
    with pytest.raises(ValueError, match="sk_resize: 9000 -> 4 needs .* composite taps .* 1024 at the most"):
        ops.sk_resize(torch.zeros((1, 9000, 2, 3), dtype=torch.uint8), (4, 2))
    pred = torch.zeros((2, 3, 5, 7))
    with pytest.raises(RuntimeError, match="frames_u8: pred must be a CUDA tensor"):
        ops.frames_u8(pred)
    for bad in (pred.double(), pred[0], pred[:, :2], pred.permute(0, 2, 3, 1), torch.zeros((1, 3, 0, 7))):
        with pytest.raises(ValueError, match="float32 .n, 3, H, W. frames"):
            ops.frames_u8(bad)


def test_pipeline_refusals_that_need_no_device():
    from e4s2024_amd import pipeline
    src, tgt = torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    call = lambda *a, **kw: pipeline.reenact_drivens(None, None, None, None, None, None, None, *a, **kw)      # noqa: E731
    for kw in (dict(size=0), dict(size=16.0), dict(batch=0), dict(chunk=0), dict(chunk=True)):
        with pytest.raises(ValueError, match="is a positive int"):
            call(src, tgt, **kw)
    with pytest.raises(ValueError, match="channel_order"):
        call(src, tgt, channel_order="bgr")
    with pytest.raises(TypeError, match="unexpected keyword 'relative'"):
        call(src, tgt, relative=True)
    with pytest.raises(TypeError, match="yaw is a number"):
        call(src, tgt, yaw="20")
    with pytest.raises(ValueError, match="uint8 .bs, H, W, 3. image batch"):
        call(src.float(), tgt)
    with pytest.raises(ValueError, match="source_u8 is ONE image"):
        call(tgt, tgt)
    with pytest.raises(RuntimeError, match="reenact_drivens: source_u8 must be a CUDA tensor"):
        call(src, tgt)
    with pytest.raises(TypeError, match="flip_target"):
        pipeline.reenact_recolor_clip(*[None] * 11, src, tgt, flip_target=1)
    with pytest.raises(RuntimeError, match="reenact_recolor_clip: source_u8 must be a CUDA tensor"):
        pipeline.reenact_recolor_clip(*[None] * 11, src, tgt)
