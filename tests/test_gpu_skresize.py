"""Row f24 on the device: ``ops.sk_resize`` against tests/skresize_model.py, ``ops.frames_u8`` bit for bit against numpy, and ``pipeline.reenact_drivens`` /
``reenact_recolor_clip`` against the composition of their public parts on the small seeded networks of the f15 / f16 / f20 / f23 tests.

The bar of the resize against the model's ``float32(...)`` on seeded random bytes.  The kernel and the model both sum float64 products of non-negative weights
of sum one, in different orders: the two float64 values differ by less than 2^-47 (tests/test_skresize_cpu.py holds the model to scipy within that), so they
round to different float32 values only across a rounding boundary: no element differs by more than ONE float32 ulp, and at most 1 element in 10^4 differs at all
(a condition, not a measurement: the model against scipy differs in 0 elements on every case, at the seed of the cases).  On top of it the kernel's own order is
pinned: ``skresize_model.resize_composed`` sums the host tables x first, ascending, one rounding per product and per sum, and the device gives its bits, through
the LDS plan and through the direct form alike."""
import numpy as np
import pytest
import torch

import skresize_model as M
from e4s2024_amd import ops, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
# the issue's table; 400 x 9 -> 8 x 8 needs all 400 source rows for its one tile, over the 80 of the LDS plan: the direct form
CASES = M.GPU_CASES + (M.WORKLOAD_CASE,)
_WANT = {}


def dev(a):
    return T(a).to(DEV)


def _case(case):
    """(img uint8 [2, H, W, 3], the model's float32 [2, Ho, Wo, 3]) of a case, made once."""
    if case not in _WANT:
        img = M.image_u8(case, bs=2)
        _WANT[case] = (img, M.resize(img, case[2:]).astype(np.float32))
    return _WANT[case]


def _ulps(got, want):
    """Distance in float32 steps between two arrays of non-negative floats."""
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ e4s_sk_resize_u8
@pytest.mark.parametrize("case", CASES, ids=M.tag)
def test_sk_resize_against_the_model(case):
    img, want = _case(case)
    x = dev(img)
    hwc = ops.sk_resize(x, case[2:], chw=False)
    chw = ops.sk_resize(x, case[2:])
    assert hwc.dtype == torch.float32 and tuple(hwc.shape) == (2, case[2], case[3], 3) and tuple(chw.shape) == (2, 3, case[2], case[3])
    assert hwc.is_contiguous() and chw.is_contiguous() and torch.equal(chw.permute(0, 2, 3, 1), hwc)                  # both layouts, the same values
    got = hwc.cpu().numpy()
    steps = _ulps(got, want)
    print(f"{M.tag(case)}: {int((steps > 0).sum())} of {steps.size} float32 values differ from the model, the farthest by {int(steps.max())} ulp")
    assert steps.max() <= 1
    assert (steps > 0).sum() <= steps.size * 1e-4
    # a sample of a batch gets the bits it gets alone
    for i in range(2):
        assert torch.equal(ops.sk_resize(x[i:i + 1], case[2:], chw=False), hwc[i:i + 1])
    if case[:2] == case[2:]:
        assert np.array_equal(got, (img / 255.0).astype(np.float32))                          # identity: exactly float32(v / 255.0)


@pytest.mark.parametrize("case", M.GPU_CASES + ((128, 40, 32, 10),), ids=M.tag)
def test_sk_resize_gives_the_bits_of_its_own_order(case):
    """The host tables summed in the kernel's order in numpy: the LDS plan and the direct form (400 x 9) give the same bits as that, so as each other."""
    img, _ = _case(case) if case in M.GPU_CASES else (M.image_u8(case, bs=2), None)
    H, W, Ho, Wo = case
    want = M.resize_composed(img, (Ho, Wo), ops.sk_resize_tables(H, Ho), ops.sk_resize_tables(W, Wo)).astype(np.float32)
    assert np.array_equal(ops.sk_resize(dev(img), (Ho, Wo), chw=False).cpu().numpy(), want)


def test_sk_resize_exact_values_and_the_clip():
    for H, W, Ho, Wo in ((37, 29, 8, 8), (20, 24, 32, 40), (400, 9, 8, 8), (64, 64, 16, 16)):
        ones = ops.sk_resize(torch.full((1, H, W, 3), 255, dtype=torch.uint8, device=DEV), (Ho, Wo))
        zeros = ops.sk_resize(torch.zeros((1, H, W, 3), dtype=torch.uint8, device=DEV), (Ho, Wo))
        assert bool((ones == 1.0).all()) and bool((zeros == 0.0).all()), (H, W, Ho, Wo)
        img = M.image_u8((H, W, Ho, Wo), bs=2, lo=17, hi=200)
        img[:, 0, 0], img[:, -1, -1] = 17, 200
        got = ops.sk_resize(dev(img), (Ho, Wo)).cpu().numpy()
        assert got.min() >= np.float32(17 / 255.0) and got.max() <= np.float32(200 / 255.0)
        flat = ops.sk_resize(torch.full((1, H, W, 3), 200, dtype=torch.uint8, device=DEV), (Ho, Wo)).cpu().numpy()
        assert (flat == np.float32(200 / 255.0)).all()
    # every sample is clipped to its OWN range: a dark and a bright sample in one batch
    pair = np.stack([np.full((12, 12, 3), 3, dtype=np.uint8), np.full((12, 12, 3), 250, dtype=np.uint8)])
    got = ops.sk_resize(dev(pair), (5, 5)).cpu().numpy()
    assert (got[0] == np.float32(3 / 255.0)).all() and (got[1] == np.float32(250 / 255.0)).all()
    assert ops.sk_resize(torch.zeros((0, 9, 9, 3), dtype=torch.uint8, device=DEV), (4, 5)).shape == (0, 3, 4, 5)
    # a non-contiguous view and a batch that starts off a 4-byte boundary (the range pass reads aligned dwords behind a byte head)
    img = M.image_u8((21, 23, 9, 10), bs=3)
    want = ops.sk_resize(dev(img), (9, 10))
    wide = dev(np.concatenate([img, img], axis=2))
    assert torch.equal(ops.sk_resize(wide[:, :, :23], (9, 10)), want)
    flat = torch.empty(img.size + 8, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):
        view = flat[off:off + img.size].view(img.shape)
        view.copy_(dev(img))
        assert view.data_ptr() % 4 == off and torch.equal(ops.sk_resize(view, (9, 10)), want)


def test_sk_resize_graph_replay_equals_the_eager_call():
    case = (37, 29, 8, 8)
    img, _ = _case(case)
    x = dev(img)
    eager = ops.sk_resize(x, case[2:])                                                        # the tables exist from here on
    static = x.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                             # one stream: no parallel branches
        out = ops.sk_resize(static, case[2:])
        u8 = ops.frames_u8(out, flip=True)
    for src in (x, x.flip(0)):
        static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        want = ops.sk_resize(src.contiguous(), case[2:])
        assert torch.equal(out, want) and torch.equal(u8, ops.frames_u8(want, flip=True))
    assert torch.equal(want, eager.flip(0))


def test_refusals_on_the_device():
    img = torch.zeros((1, 9, 7, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8 .bs, H, W, 3. image batch"):
        ops.sk_resize(img.float(), (4, 4))
    with pytest.raises(ValueError, match="uint8 .bs, H, W, 3. image batch"):
        ops.sk_resize(img.permute(0, 3, 1, 2), (4, 4))
    with pytest.raises(ValueError, match="size is a pair"):
        ops.sk_resize(img, (4, 0))
    with pytest.raises(ValueError, match="size is a pair"):
        ops.sk_resize(img, (4.0, 4))
    with pytest.raises(ValueError, match="1024 at the most"):
        ops.sk_resize(torch.zeros((1, 9000, 2, 3), dtype=torch.uint8, device=DEV), (4, 2))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.sk_resize(img.cpu(), (4, 4))
    pred = torch.zeros((1, 3, 5, 7), device=DEV)
    with pytest.raises(ValueError, match="float32 .n, 3, H, W. frames"):
        ops.frames_u8(pred.half())
    with pytest.raises(ValueError, match="float32 .n, 3, H, W. frames"):
        ops.frames_u8(pred.permute(0, 2, 3, 1))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.frames_u8(pred.cpu())


# ------------------------------------------------------------------------------------------------ e4s_frames_u8
@pytest.mark.parametrize("H,W", [(5, 7), (256, 256)])
def test_frames_u8_bit_for_bit(H, W):
    v = M.frame_values(2, H, W)
    x = dev(v)
    for flip in (False, True):
        want = M.frames_u8(v, flip)
        got = ops.frames_u8(x, flip=flip)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, H, W, 3) and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), want), (H, W, flip)
        # a non-contiguous input (a channel-last view, a slice of a wider batch) and one that starts off a 16-byte boundary
        assert torch.equal(ops.frames_u8(dev(v.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2), flip=flip), got)
        wide = dev(np.concatenate([v, v], axis=3))
        assert torch.equal(ops.frames_u8(wide[..., :W], flip=flip), got)
        flat = torch.empty(v.size + 4, dtype=torch.float32, device=DEV)
        off = flat[1:1 + v.size].view(v.shape)
        off.copy_(x)
        assert off.data_ptr() % 16 == 4 and torch.equal(ops.frames_u8(off, flip=flip), got)
    assert ops.frames_u8(x[:0]).shape == (0, H, W, 3)


def test_frames_u8_outside_the_unit_interval():
    """numpy leaves these undefined; the kernel clamps, and a NaN gives 0."""
    v = torch.tensor([-1.0, -0.0, 0.0, 1.0, 1.5, 300.0, float("inf"), float("-inf"), float("nan"), 0.999999, 1 / 255, 254.999 / 255], device=DEV)
    got = ops.frames_u8(v.view(1, 1, 1, -1).expand(1, 3, 1, -1))[0, 0, :, 0].tolist()
    assert got == [0, 0, 0, 255, 255, 255, 255, 0, 0, 254, 1, 254]


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture()
def nets(monkeypatch):
    """The seeded networks of the f15 / f16 / f20 tests at their smallest sizes: the G-E generator with its 16 x 16 detector and head-pose estimator, RetinaFace
    'D', GPEN 's32', ParseNet 'C' with the paste constants that fit a 32 x 32 mask, and the x2 RealESRNet of 32 features and one block."""
    import gpen_sr_model as SRM
    import test_gpu_gpen_paste as TP
    import test_gpu_gpen_sr as TS
    import test_gpu_vid2vid_decoder as VD
    for key in ("ksize", "sigma", "thres", "small_face"):
        monkeypatch.setitem(ops.GPEN_PASTE_DEFAULTS, key, SRM.FE_PASTE[key])
    kp, he, _, _ = VD._clip()
    detector, gpen, parsenet = TP._nets()
    tag = SRM.tag_of(2, 32, 1, 7, 9)
    return VD._net(), kp, he, detector, gpen, parsenet, TS._net(SRM.image_case(tag)["sd"], tag)


def _smooth_u8(rs, n, h, w):
    """Seeded uint8 ``[n, 6 h, 6 w, 3]``: blocks of 6 x 6 in 30 .. 225 with +-12 of noise."""
    blocks = np.kron(rs.randint(30, 226, size=(n, h, w, 3)), np.ones((1, 6, 6, 1), dtype=np.int64))
    return np.clip(blocks + rs.randint(-12, 13, size=blocks.shape), 0, 255).astype(np.uint8)


def _clip_u8(n, seed=3):
    """(source uint8 [1, 42, 36, 3], targets uint8 [n, 30, 48, 3]) on the device."""
    rs = np.random.RandomState(seed)
    return dev(_smooth_u8(rs, 1, 7, 6)), dev(_smooth_u8(rs, n, 5, 8))


def test_reenact_drivens_is_its_pieces(nets):
    gen, kp, he, detector, gpen, parsenet, sr = nets
    source_u8, targets_u8 = _clip_u8(3)
    src, drv = ops.sk_resize(source_u8, (16, 16)), ops.sk_resize(targets_u8, (16, 16))
    pred = pipeline.reenact_clip(gen, kp, he, src, drv, batch=2)
    assert tuple(pred.shape) == (3, 3, 32, 32)
    plain = ops.frames_u8(pred)
    # enhance=False: the uint8 predictions, whatever stands in the GPEN networks' places
    got = pipeline.reenact_drivens(gen, kp, he, None, None, None, None, source_u8, targets_u8, size=16, enhance=False, batch=2)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 32, 32, 3) and torch.equal(got, plain) and 8 < len(got.unique())
    # 'rgb': the frames as they are; 'reference': channel-reversed in, reversed back out
    want_rgb = pipeline.gpen_face_enhancement(detector, gpen, parsenet, sr, plain)
    want_ref = pipeline.gpen_face_enhancement(detector, gpen, parsenet, sr, plain.flip(3).contiguous()).flip(3)
    rgb = pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, sr, source_u8, targets_u8, size=16, channel_order="rgb", batch=2)
    ref = pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, sr, source_u8, targets_u8, size=16, batch=2)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (3, 64, 64, 3) and rgb.is_contiguous() and torch.equal(rgb, want_rgb)
    assert tuple(ref.shape) == (3, 64, 64, 3) and torch.equal(ref, want_ref)
    assert not torch.equal(ref, rgb)                                                          # the channel order reaches the result
    assert torch.equal(ops.frames_u8(pred, flip=True), plain.flip(3))
    # chunks and generator batches smaller than the clip: the same bytes
    for chunk, batch in ((1, 1), (2, 4), (8, 3)):
        assert torch.equal(pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, sr, source_u8, targets_u8, size=16, chunk=chunk, batch=batch), ref)
    # without the RealESRNet pass D has the predictions' size
    assert torch.equal(pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, None, source_u8, targets_u8, size=16, channel_order="rgb"),
                       pipeline.gpen_face_enhancement(detector, gpen, parsenet, None, plain))
    # an empty clip
    assert pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, sr, source_u8, targets_u8[:0], size=16).shape == (0, 64, 64, 3)
    assert pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, None, source_u8, targets_u8[:0], size=16).shape == (0, 32, 32, 3)
    assert pipeline.reenact_drivens(gen, kp, he, None, None, None, None, source_u8, targets_u8[:0], size=16, enhance=False).shape == (0, 32, 32, 3)
    # free-view keywords reach make_animation
    free = pipeline.reenact_drivens(gen, kp, he, None, None, None, None, source_u8, targets_u8, size=16, enhance=False, free_view=True, yaw=20.0, pitch=None, roll=None)
    assert torch.equal(free, ops.frames_u8(pipeline.reenact_clip(gen, kp, he, src, drv, free_view=True, yaw=20.0, pitch=None, roll=None)))


def test_reenact_drivens_refusals_on_the_device(nets):
    gen, kp, he, detector, gpen, parsenet, sr = nets
    source_u8, targets_u8 = _clip_u8(1)
    call = lambda *a, **kw: pipeline.reenact_drivens(*a, source_u8, targets_u8, **{**dict(size=16), **kw})           # noqa: E731
    with pytest.raises(ValueError, match="reenact_drivens: .*multiples of"):
        call(gen, kp, he, detector, gpen, parsenet, sr, size=17)
    with pytest.raises(RuntimeError, match="reenact_drivens: .*device mismatch"):
        call(gen, _cpu_copy(kp), he, detector, gpen, parsenet, sr)
    with pytest.raises(TypeError, match="reenact_drivens"):
        call(gen, kp, he, detector, gpen, None, sr)
    with pytest.raises(RuntimeError, match="device mismatch"):
        call(gen, kp, he, detector, gpen, parsenet, _cpu_copy(sr))
    with pytest.raises(RuntimeError, match="training mode"):
        call(gen, kp, _cpu_copy(he).train().to(DEV), detector, gpen, parsenet, sr)
    with pytest.raises(ValueError, match="targets_u8"):
        pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, sr, source_u8, targets_u8.cpu(), size=16)


def _cpu_copy(module):
    import copy
    return copy.deepcopy(module).cpu()


@pytest.fixture(scope="module")
def recolor_nets(bisenet_sd):
    """The parser, the recolouring network, CodeFormer and the x4 Real-ESRGAN of tests/test_gpu_esrgan_tile.py's ``recolor_frames`` test."""
    import codeformer_model as CM
    import esrgan_tile_model as EM
    from conftest import install_dropin
    from e4s2024_amd import seeded
    install_dropin()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    parser = FaceParser(seg_ckpt=None, device=DEV)
    parser.seg.load_state_dict(bisenet_sd)
    parser.seg.eval()
    blender = ops.BlenderNet().eval()
    blender.referencer.FPN.load_state_dict(seeded.seeded_fpn_state_dict(22))
    blender.unet.load_state_dict(seeded.seeded_resunet_state_dict(21, 64))
    with torch.no_grad():
        blender.referencer.trainable_tao.fill_(7.0)
    codeformer = ops.CodeFormer(*CM.CASES["CF-F"]["cfg"]).eval()
    codeformer.load_state_dict(CM.case_weights("CF-F"), strict=True)
    SM = EM.SM
    sd = SM.base_state_dict(4, 64, 1, EM.CASE_SEED)
    x = SM.images_u8(5, 1, 16, 16).transpose(0, 3, 1, 2).astype(np.float64) / 255.
    esr = ops.GpenSRNet(1, 64, 4).eval()
    esr.load_state_dict(SM.calibrated(sd, SM.network(sd, x)))
    return parser, blender.to(DEV), codeformer.to(DEV), esr.to(DEV)


def test_reenact_recolor_clip_is_drivens_and_recolor_frames(nets, recolor_nets):
    """One frame at size 128 with a x4 RealESRNet: the predictions are 256 x 256 and D is 1024 x 1024, the size the recolor loop's parser takes."""
    import codeformer_gen_model as G
    import gpen_sr_model as SRM
    import test_gpu_gpen_sr as TS
    gen, kp, he, detector, gpen, parsenet, _ = nets
    parser, blender, codeformer, esr = recolor_nets
    tag = SRM.tag_of(4, 32, 2, 7, 9)
    sr4 = TS._net(SRM.image_case(tag)["sd"], tag)
    source_u8, targets_u8 = _clip_u8(1, seed=4)
    D, D_recolor = pipeline.reenact_recolor_clip(gen, kp, he, detector, gpen, parsenet, sr4, parser, blender, codeformer, esr, source_u8, targets_u8, size=128,
                                                 flip_target=True, w=G.W)
    want_D = pipeline.reenact_drivens(gen, kp, he, detector, gpen, parsenet, sr4, source_u8, targets_u8, size=128)
    assert D.dtype == torch.uint8 and tuple(D.shape) == (1, 1024, 1024, 3) and torch.equal(D, want_D) and 8 < len(D.unique())
    want = pipeline.recolor_frames(parser, blender, codeformer, esr, want_D, targets_u8, flip_target=True, w=G.W)
    assert D_recolor.dtype == torch.uint8 and tuple(D_recolor.shape) == (1, 1024, 1024, 3) and torch.equal(D_recolor, want)
    empty = pipeline.reenact_recolor_clip(gen, kp, he, detector, gpen, parsenet, sr4, parser, blender, codeformer, esr, source_u8, targets_u8[:0], size=128)
    assert tuple(empty[0].shape) == (0, 1024, 1024, 3) and tuple(empty[1].shape) == (0, 1024, 1024, 3)
    with pytest.raises(RuntimeError, match="reenact_recolor_clip: .*training mode"):
        pipeline.reenact_recolor_clip(gen, kp, he, detector, gpen, parsenet, sr4, parser, blender, codeformer, ops.GpenSRNet(1, 64, 4).to(DEV), source_u8, targets_u8,
                                      size=128)
    with pytest.raises(TypeError, match="parse_batch"):
        pipeline.reenact_recolor_clip(gen, kp, he, detector, gpen, parsenet, sr4, None, blender, codeformer, esr, source_u8, targets_u8, size=128)
