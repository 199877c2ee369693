"""GPU tests of row f5: ``ops.crop_align`` and ``ops.paste_into_frames`` (csrc/align.hip) byte for byte against the numpy model of Pillow's
warps (``tests/align_model.py``, itself pinned to Pillow by ``tests/test_align_cpu.py``) and against Pillow where it is installed; batch
independence, run-to-run and stream stability; and ``pipeline.swap_frames``, the video pipeline's per-frame loop with ``use_crop=True``."""
import numpy as np
import pytest
import torch

import align_model as M
from conftest import install_dropin, record_parity
from e4s2024_amd import align, ops, pipeline, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731

try:
    from PIL import Image  # noqa: F401
    HAVE_PIL = True
except ImportError:            # the model stands in (it is checked against Pillow on the host)
    HAVE_PIL = False


def _hd_quads():
    return np.stack([M.square_quad(960, 540, 300, 0.35),       # rotated, inside the frame
                     M.square_quad(1800, 120, 380, -0.5),      # partly outside (top right)
                     M.square_quad(150, 1000, 260, 1.2),       # partly outside (bottom left)
                     M.square_quad(1200, 400, 12, 0.2)])       # a tiny face


@pytest.fixture(scope="module")
def hd():
    rng = np.random.default_rng(11)
    frames = np.stack([M.make_frame(rng, 1080, 1920) for _ in range(4)])
    plan = align.crop_plan(_hd_quads(), (1080, 1920), 1024)
    faces = np.stack([M.make_frame(rng, 1024, 1024) for _ in range(4)])
    return frames, plan, faces


def _count(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def test_crop_align_hd_batch_is_bit_exact(hd):
    frames, plan, _ = hd
    got = ops.crop_align(T(frames).to(DEV), plan.to(DEV)).cpu().numpy()
    assert got.shape == (4, 1024, 1024, 3) and int(plan.shrink.max()) == 1
    for i in range(4):
        want = M.crop_align(frames[i], plan, i)
        d = _count(got[i], want)
        record_parity(f"align.crop_1080p.frame{i}.bytes_vs_model", d, 0)
        assert d == 0, i
        if HAVE_PIL:
            d = _count(got[i], M.pil_crop_image(frames[i], plan.quads[i], 1024))
            record_parity(f"align.crop_1080p.frame{i}.bytes_vs_pillow", d, 0)
            assert d == 0, i
    assert (got[1] == 0).all(axis=-1).any() and (got[2] == 0).all(axis=-1).any()      # the overhanging faces have unsampled (0) pixels


def test_crop_align_4k_shrink_branch_is_bit_exact():
    rng = np.random.default_rng(12)
    frame = M.make_frame(rng, 2160, 3840)[None]
    plan = align.crop_plan(M.square_quad(1900, 1000, 1500, 0.15)[None], (2160, 3840), 1024)
    assert int(plan.shrink[0]) == 2 and tuple(plan.resized_wh[0]) == (1920, 1080)
    got = ops.crop_align(T(frame).to(DEV), plan).cpu().numpy()[0]
    d = _count(got, M.crop_align(frame[0], plan, 0))
    record_parity("align.crop_4k_shrink2.bytes_vs_model", d, 0)
    assert d == 0
    if HAVE_PIL:
        d = _count(got, M.pil_crop_image(frame[0], plan.quads[0], 1024))
        record_parity("align.crop_4k_shrink2.bytes_vs_pillow", d, 0)
        assert d == 0


def test_paste_into_frames_is_bit_exact_in_and_out_of_place(hd):
    frames, plan, faces = hd
    fr, fa = T(frames).to(DEV), T(faces).to(DEV)
    out = ops.paste_into_frames(fa, fr, plan)
    assert torch.equal(fr.cpu(), T(frames))                                    # out of place: the input frames are left alone
    buf = torch.full_like(fr, 7)
    out2 = ops.paste_into_frames(fa, fr, plan, out=buf)
    assert out2.data_ptr() == buf.data_ptr()
    inplace = fr.clone()
    out3 = ops.paste_into_frames(fa, inplace, plan, out=inplace)
    assert out3.data_ptr() == inplace.data_ptr()
    got = out.cpu().numpy()
    assert np.array_equal(got, out2.cpu().numpy()) and np.array_equal(got, out3.cpu().numpy())
    for i in range(4):
        d = _count(got[i], M.paste(faces[i], frames[i], plan, i))
        record_parity(f"align.paste_1080p.frame{i}.bytes_vs_model", d, 0)
        assert d == 0, i
        if HAVE_PIL:
            d = _count(got[i], M.pil_paste(faces[i], frames[i], plan.inv_coeffs[i].numpy()))
            record_parity(f"align.paste_1080p.frame{i}.bytes_vs_pillow", d, 0)
            assert d == 0, i
        x0, y0, x1, y1 = plan.paste_boxes[i].tolist()
        outside = np.ones(got.shape[1:3], bool)
        outside[y0:y1, x0:x1] = False
        assert np.array_equal(got[i][outside], frames[i][outside])
        assert _count(got[i], frames[i]) > 0


def test_paste_4k_is_bit_exact():
    rng = np.random.default_rng(13)
    frame, face = M.make_frame(rng, 2160, 3840)[None], M.make_frame(rng, 1024, 1024)[None]
    plan = align.crop_plan(M.square_quad(2500, 900, 700, -0.25)[None], (2160, 3840), 1024)
    got = ops.paste_into_frames(T(face).to(DEV), T(frame).to(DEV), plan).cpu().numpy()[0]
    d = _count(got, M.paste(face[0], frame[0], plan, 0))
    record_parity("align.paste_4k.bytes_vs_model", d, 0)
    assert d == 0


def test_batches_are_independent_stable_and_stream_safe():
    """Frame i of a batch = the frame alone; 40 frames (two launches of the kernels' 32-frame chunks) of odd sizes (the byte-store paths);
    a second run is bit-identical; the batch split over two streams equals one stream."""
    rng = np.random.default_rng(14)
    n, h, w, s = 40, 61, 83, 30
    frames = np.stack([M.make_frame(rng, h, w) for _ in range(n)])
    faces = np.stack([M.make_frame(rng, s, s) for _ in range(n)])
    quads = np.stack([M.square_quad(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(3, 40), rng.uniform(-3, 3)) for _ in range(n)])
    quads[5] = M.square_quad(40, 30, 60, 0.2)                                   # diag 170 > 4 s: a shrink frame inside the batch
    plan = align.crop_plan(quads, (h, w), s)
    assert int(plan.shrink[5]) == 2
    fr, fa = T(frames).to(DEV), T(faces).to(DEV)
    crops = ops.crop_align(fr, plan)
    pasted = ops.paste_into_frames(fa, fr, plan)
    for i in range(n):
        assert _count(crops[i].cpu().numpy(), M.crop_align(frames[i], plan, i)) == 0, i
        assert _count(pasted[i].cpu().numpy(), M.paste(faces[i], frames[i], plan, i)) == 0, i
    for i in (0, 5, 33):
        assert torch.equal(ops.crop_align(fr[i:i + 1], plan[i:i + 1])[0], crops[i])
        assert torch.equal(ops.paste_into_frames(fa[i:i + 1], fr[i:i + 1], plan[i:i + 1])[0], pasted[i])
    assert torch.equal(ops.crop_align(fr, plan), crops) and torch.equal(ops.paste_into_frames(fa, fr, plan), pasted)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(main)
    c2, p2 = torch.empty_like(crops), torch.empty_like(pasted)
    with torch.cuda.stream(side):
        c2[:20] = ops.crop_align(fr[:20], plan[:20])
        ops.paste_into_frames(fa[:20], fr[:20], plan[:20], out=p2[:20])
    c2[20:] = ops.crop_align(fr[20:], plan[20:])
    ops.paste_into_frames(fa[20:], fr[20:], plan[20:], out=p2[20:])
    main.wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(c2, crops) and torch.equal(p2, pasted)


# ------------------------------------------------------------------------------------------------ swap_frames
@pytest.fixture(scope="module")
def parser(bisenet_sd):
    install_dropin()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    p = FaceParser(seg_ckpt=None, device=DEV)
    p.seg.load_state_dict(bisenet_sd)
    p.seg.eval()
    return p


def test_swap_frames_bs2(gpu_net3, parser):
    rng = np.random.default_rng(15)
    frames = np.stack([M.make_frame(rng, 1080, 1920) for _ in range(2)])
    plan = align.crop_plan(_hd_quads()[:2], (1080, 1920), 1024)
    driven = seeded.seeded_image(16, 2, 1024).to(DEV)
    fr = T(frames).to(DEV)
    got = pipeline.swap_frames(gpu_net3, parser, driven, fr, plan)
    assert got.shape == fr.shape and got.dtype == torch.uint8 and torch.equal(fr.cpu(), T(frames))
    # by hand: crop, swap, paste back into the crop, paste into the frame
    crops = ops.crop_align(fr, plan)
    sw, _, extra = pipeline.swap_batch(gpu_net3, parser, driven, ops.frames_to_tensor(crops), mask_surgery=True)
    blended = pipeline.paste_back(sw, crops, extra["content"], extra["border"])
    want = ops.paste_into_frames(blended, fr, plan)
    assert torch.equal(got, want)
    g = got.cpu().numpy()
    for i in range(2):
        x0, y0, x1, y1 = plan.paste_boxes[i].tolist()
        outside = np.ones(g.shape[1:3], bool)
        outside[y0:y1, x0:x1] = False
        assert np.array_equal(g[i][outside], frames[i][outside])
        assert _count(g[i], frames[i]) > 0
    # the host route: the crop and the paste by Pillow (or its model), the swap on the device
    host_crops = np.stack([(M.pil_crop_image(frames[i], plan.quads[i], 1024) if HAVE_PIL else M.crop_align(frames[i], plan, i)) for i in range(2)])
    hc = T(host_crops).to(DEV)
    sw, _, extra = pipeline.swap_batch(gpu_net3, parser, driven, ops.frames_to_tensor(hc), mask_surgery=True)
    bl = pipeline.paste_back(sw, hc, extra["content"], extra["border"]).cpu().numpy()
    for i in range(2):
        ref = M.pil_paste(bl[i], frames[i], plan.inv_coeffs[i].numpy()) if HAVE_PIL else M.paste(bl[i], frames[i], plan, i)
        d = _count(g[i], ref)
        record_parity(f"align.swap_frames.frame{i}.bytes_vs_host_route", d, 0)
        assert d == 0, i
