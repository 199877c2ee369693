"""Row f23 on the device: the three kernels of csrc/esrgan_tile.hip alone, ``ops.esrgan_enhance`` / ``cv_resize_lanczos4`` against tests/esrgan_tile_model.py on
the cases of g33_esrgan_tile.npz, the full depth once, and ``pipeline.codeformer_enhance`` / ``recolor_frames`` against the composition of their public parts.
Small shapes throughout: each test takes seconds.

The bars.  ``e4s_esrt_input`` and the resize: bit for bit the model (a correctly rounded division; integer arithmetic).  ``e4s_esrt_tail``: the uint8 rule of
tests/gpen_sr_model.py against float64, and bit for bit the rounding end on the fused float32 chain in the documented order.  A network case: the uint8 rule
with ``e32`` the model in float32 against itself in float64, never the code under test; the resized image bit for bit the model's Lanczos4 of the device's OWN x4
image, so that a pixel that is not strict cannot spread through eight taps."""
import numpy as np
import pytest
import torch

import codeformer_gen_model as G
import codeformer_model as CM
import esrgan_tile_model as M
from conftest import install_dropin
from e4s2024_amd import ops, pipeline, seeded
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
SM = M.SM
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
_NETS = {}


def dev(a):
    return T(a).to(DEV)


def _net(sd, key):
    """``ops.GpenSRNet`` with ``sd`` on the device, one module per ``key`` (a module caches its prepared weights)."""
    if key not in _NETS:
        net = ops.GpenSRNet(SM.num_blocks(sd), int(sd["conv_first.weight"].shape[0]), 4).eval()
        net.load_state_dict(sd, strict=True)
        _NETS[key] = net.to(DEV)
    return _NETS[key]


def _offset(t):
    """A copy of ``t`` that starts one element past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


# ------------------------------------------------------------------------------------------------ e4s_cv_resize_lanczos4_u8
# the table of the issue; 100 x 90 -> 7 x 9 takes the direct form (a tile's source window is 94 rows, over the 40 of the LDS plan), 64 x 300 -> 32 x 20 takes it for
# its columns alone (293 over 136; its rows fit); 200 x 300 -> 100 x 150 is the 2 : 1 plan over 7 x 3 workgroups with ragged ends; 40 x 30 -> 90 x 100 an
# enlargement over several workgroups
LANCZOS_CASES = M.RESIZE_CASES + ((100, 90, 7, 9), (64, 300, 32, 20), (200, 300, 100, 150), (40, 30, 90, 100))


@pytest.mark.parametrize("H,W,Ho,Wo", LANCZOS_CASES, ids=lambda v: str(v))
def test_cv_resize_lanczos4_bit_for_bit(H, W, Ho, Wo):
    img = M.resize_image(H, W)
    want = M.resize_lanczos4(img, (Wo, Ho))
    got = ops.cv_resize_lanczos4(dev(img), (Wo, Ho))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, Ho, Wo, 3) and got.is_contiguous()
    diff = np.abs(got.cpu().numpy().astype(int) - want.astype(int))
    print(f"{H} x {W} -> {Ho} x {Wo}: {int((diff != 0).sum())} bytes differ, by {int(diff.max())} at the most")
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.cv_resize_lanczos4(_offset(dev(img)), (Wo, Ho)), got)              # rows that start at any address: the same bits
    assert torch.equal(ops.cv_resize_lanczos4(dev(img)[1:], (Wo, Ho)), got[1:])               # a sample alone
    assert ops.cv_resize_lanczos4(dev(img)[:0], (Wo, Ho)).shape == (0, Ho, Wo, 3)
    if (H, W) == (Ho, Wo):
        assert torch.equal(got, dev(img))


def test_cv_resize_lanczos4_refusals_on_the_device():
    img = torch.zeros((1, 6, 7, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="dsize"):
        ops.cv_resize_lanczos4(img, (0, 3))
    with pytest.raises(ValueError, match="uint8"):
        ops.cv_resize_lanczos4(img.float(), (3, 3))
    out = torch.empty(64, dtype=torch.uint8, device=DEV)
    tab = torch.zeros(64, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="bad size"):
        lib().call("e4s_cv_resize_lanczos4_u8", _p(out), _p(img), _p(tab), _p(tab), _p(tab), _p(tab), 1, 6, 7, 0, 3, _stream())
    with pytest.raises(RuntimeError, match="unaligned table"):
        lib().call("e4s_cv_resize_lanczos4_u8", _p(out), _p(img), _p(tab), _p(tab[1:]), _p(tab), _p(tab), 1, 6, 7, 2, 2, _stream())


# ------------------------------------------------------------------------------------------------ e4s_esrt_input
def _esrt_input(img, chw, pre_pad, win):
    bs = img.shape[0]
    H, W = (img.shape[2], img.shape[3]) if chw else (img.shape[1], img.shape[2])
    y0, y1, x0, x1 = win
    out = torch.empty((bs, 3, y1 - y0, x1 - x0), dtype=torch.float32, device=DEV)
    lib().call("e4s_esrt_input", _p(out), _p(img), bs, H, W, H + pre_pad, W + pre_pad, int(chw), y0, x0, y1 - y0, x1 - x0, _stream())
    return out


@pytest.mark.parametrize("H,W,pre_pad", [(11, 14, 0), (9, 9, 3), (6, 7, 5), (5, 8, 4)])
def test_esrt_input_bit_for_bit(H, W, pre_pad):
    """v / 255 and the reflect pre-pad for both layouts: the whole padded image, windows at each border and corner, an interior window, single pixels — among them
    windows that lie in the reflected rows and columns alone."""
    Hp, Wp = H + pre_pad, W + pre_pad
    imgs = SM.images_u8(H * 100 + W + pre_pad, 2, H, W)
    want = np.stack([M.pre_process(i, pre_pad, torch.float32)[0].numpy() for i in imgs])
    assert want.shape == (2, 3, Hp, Wp) and want.dtype == np.float32
    wins = [(0, Hp, 0, Wp), (0, 3, 0, Wp), (Hp - 2, Hp, 0, Wp), (0, Hp, 0, 2), (0, Hp, Wp - 3, Wp), (2, 5, 1, 6), (Hp - 1, Hp, Wp - 1, Wp), (0, 1, 0, 1)]
    if pre_pad:
        wins += [(H, Hp, W, Wp), (H - 1, Hp, 0, 3)]
    hwc, chw = dev(imgs), dev(imgs.transpose(0, 3, 1, 2))
    for win in wins:
        y0, y1, x0, x1 = win
        for layout, src in ((0, hwc), (1, chw)):
            got = _esrt_input(src, layout, pre_pad, win)
            assert np.array_equal(got.cpu().numpy(), want[:, :, y0:y1, x0:x1]), (win, layout)
    assert _esrt_input(hwc[:0], 0, pre_pad, wins[0]).shape[0] == 0


def test_esrt_input_refusals():
    img = torch.zeros((1, 4, 8, 3), dtype=torch.uint8, device=DEV)
    out = torch.empty(3 * 64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="reflect-padded"):
        lib().call("e4s_esrt_input", _p(out), _p(img), 1, 4, 8, 8, 8, 0, 0, 0, 2, 2, _stream())
    for win in ((0, 0, 5, 2), (3, 7, 2, 2), (-1, 0, 2, 2), (0, 0, 0, 2)):
        with pytest.raises(RuntimeError, match="does not lie"):
            lib().call("e4s_esrt_input", _p(out), _p(img), 1, 4, 8, 4, 8, 0, *win, _stream())


# ------------------------------------------------------------------------------------------------ e4s_esrt_tail
def _esrt_tail(x, w, b, win, place, canvas_hw, pitch=None):
    bs, C, H, W = x.shape
    CH, CW = canvas_hw
    pitch = pitch or CW * 3
    canvas = torch.full((bs, CH, pitch), 0x5A, dtype=torch.uint8, device=DEV)
    lib().call("e4s_esrt_tail", _p(canvas), None, _p(x), _p(w), _p(b), bs, C, H, W, win[0], win[1], win[2], win[3], place[0], place[1], CH, CW, pitch, _stream())
    return canvas.cpu().numpy()


@pytest.mark.parametrize("C", [64, 32])
@pytest.mark.parametrize("win,place,canvas_hw,pitch", [((4, 8, 0, 8), (16, 0), (40, 32), None), ((4, 8, 0, 8), (3, 5), (9, 14), 47), ((5, 6, 3, 4), (0, 7), (2, 8), None),
                                                       ((0, 12, 0, 10), (1, 4), (13, 16), 52), ((1, 12, 2, 9), (0, 0), (11, 7), None)], ids=lambda v: str(v))
def test_esrt_tail(C, win, place, canvas_hw, pitch):
    """conv_last on the kept window of a 12 x 10 tile output, placed into a canvas filled with 0x5A: the window by the uint8 rule against float64 and bit for bit
    the rounding end of the fused float32 chain; every byte outside the window (the pitch's slack included) still 0x5A.  Places at and off a 4-pixel boundary
    (the packed and the bytewise store), a one-pixel window, the whole tile, a window with ragged ends."""
    bs, H, W = 2, 12, 10
    x = seeded.seeded_array(SM.TAIL_SEED, "esrt.tail.x", (bs, C, H, W), 0.0, 1.0, "normal")
    w = seeded.seeded_array(SM.TAIL_SEED, "esrt.tail.w", (3, C, 3, 3), 0.0, 0.25 / np.sqrt(C * 9.0), "normal")
    b = np.array([0.5, 0.45, 0.55], dtype=np.float32)
    m = SM.tail(x, w, b)
    oy0, oy1, ox0, ox1 = win
    Y0, X0 = place
    got = _esrt_tail(dev(x), dev(w), dev(b), win, place, canvas_hw, pitch)
    px = got[:, :, :canvas_hw[1] * 3].reshape(bs, canvas_hw[0], canvas_hw[1], 3)
    kept = px[:, Y0:Y0 + oy1 - oy0, X0:X0 + ox1 - ox0]
    u = np.clip(m["r"], 0, 1).transpose(0, 2, 3, 1)[:, oy0:oy1, ox0:ox1] * 255.0
    strict, clamped, std = SM.check_u8(kept, u, m["e32"])
    f32 = np.rint(np.clip(m["f32"], np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)[:, oy0:oy1, ox0:ox1]
    print(f"C {C}, window {win} at {place}: strict {100 * strict:.1f} %, clamped {100 * clamped:.1f} %; {int((kept != f32).sum())} bytes off the float32 chain")
    assert np.array_equal(kept, f32)
    outside = np.ones(got.shape, bool)
    outside[:, Y0:Y0 + oy1 - oy0, X0 * 3:(X0 + ox1 - ox0) * 3] = False
    assert (got[outside] == 0x5A).all() and outside.sum() == got.size - kept.size


def test_esrt_tail_refusals():
    x = torch.zeros((1, 64, 12, 10), dtype=torch.float32, device=DEV)
    w, b = torch.zeros((3, 64, 3, 3), dtype=torch.float32, device=DEV), torch.zeros(3, dtype=torch.float32, device=DEV)
    canvas = torch.zeros((1, 8, 24), dtype=torch.uint8, device=DEV)
    call = lambda *a: lib().call("e4s_esrt_tail", _p(canvas), None, _p(x), _p(w), _p(b), 1, 64, 12, 10, *a, _stream())  # noqa: E731
    for win in ((4, 4, 0, 8), (4, 13, 0, 8), (-1, 4, 0, 8), (4, 8, 0, 11)):
        with pytest.raises(RuntimeError, match="does not lie"):
            call(*win, 0, 0, 8, 8, 24)
    for place in ((5, 0), (0, 1), (-1, 0)):
        with pytest.raises(RuntimeError, match="leaves the"):
            call(4, 8, 0, 8, *place, 8, 8, 24)
    with pytest.raises(RuntimeError, match="bad canvas"):
        call(4, 8, 0, 8, 0, 0, 8, 8, 23)
    with pytest.raises(RuntimeError, match="no float output"):
        lib().call("e4s_esrt_tail", _p(canvas), _p(x), _p(x), _p(w), _p(b), 1, 64, 12, 10, 4, 8, 0, 8, 0, 0, 8, 8, 24, _stream())
    with pytest.raises(RuntimeError, match="multiple of 8"):
        lib().call("e4s_esrt_tail", _p(canvas), None, _p(x), _p(w), _p(b), 1, 60, 12, 10, 4, 8, 0, 8, 0, 0, 8, 8, 24, _stream())


# ------------------------------------------------------------------------------------------------ esrgan_enhance
def _check_x4(tag, c, big):
    strict, clamped, std = M.check_u8(big, c["u"], c["e32"])
    print(f"{tag}: x4 {big.shape}: strict {100 * strict:.2f} %, clamped {100 * clamped:.2f} %, std {std:.1f}, {int((big != c['x4']).sum())} bytes off the float64 model")
    assert strict >= 0.99 and clamped < 0.10 and std > 30


@pytest.mark.parametrize("tag", list(M.GOLDEN_CASES))
def test_esrgan_enhance_on_the_golden_cases(tag):
    H, W, tile, tile_pad, pre_pad = M.GOLDEN_CASES[tag]
    c = M.golden_case(tag)
    net, img = _net(c["sd"], tag), dev(c["img"][None])
    kw = dict(tile=tile, tile_pad=tile_pad, pre_pad=pre_pad)
    x4 = None
    for outscale in M.GOLDEN_OUTSCALES:
        out, big = ops.esrgan_enhance(img, net, outscale=outscale, return_x4=True, **kw)
        assert out.dtype == big.dtype == torch.uint8 and tuple(big.shape) == (1, 4 * H, 4 * W, 3) and out.is_contiguous() and big.is_contiguous()
        if x4 is None:
            x4 = big
            _check_x4(tag, c, big[0].cpu().numpy())
        assert torch.equal(big, x4)                                                           # two calls give equal bits
        dsize = M.out_size(H, W, outscale)
        want = big[0].cpu().numpy() if dsize is None else M.resize_lanczos4(big[0].cpu().numpy(), dsize)
        assert tuple(out.shape[1:]) == want.shape and np.array_equal(out[0].cpu().numpy(), want), outscale
        assert torch.equal(ops.esrgan_enhance(img, net, outscale=outscale, **kw), out)
    assert torch.equal(ops.esrgan_enhance(img, net, outscale=4, **kw), x4) and torch.equal(ops.esrgan_enhance(img, net, outscale=4.0, **kw), x4)
    # the planar layout and a mapping for the weights: the same bits
    planar = img.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(ops.esrgan_enhance(planar, {k: v.to(DEV) for k, v in c["sd"].items()}, chw=True, **kw), x4)
    assert ops.esrgan_enhance(img[:0], net, outscale=2, **kw).shape == (0, 2 * H, 2 * W, 3)


def test_esrgan_enhance_untiled_batch_and_graph():
    tag = "11x14.t5.p2"
    H, W, tile, tile_pad, pre_pad = M.GOLDEN_CASES[tag]
    net = _net(M.golden_case(tag)["sd"], tag)
    imgs = dev(M.image_u8("batch", H, W, bs=3))
    # tile = 0 is one tile, as is any tile that holds the image
    whole = ops.esrgan_enhance(imgs, net, tile=0)
    for t in (14, 15, 400):
        assert torch.equal(ops.esrgan_enhance(imgs, net, tile=t, tile_pad=tile_pad), whole)
    tiled = ops.esrgan_enhance(imgs, net, tile=tile, tile_pad=tile_pad)
    assert not torch.equal(tiled, whole)                                                      # the tile borders change the result
    # a sample of a batch of 3 is itself alone, with and without the pre-pad and the resize
    for kw in (dict(tile=tile, tile_pad=tile_pad), dict(tile=4, tile_pad=1, pre_pad=3, outscale=2), dict(tile=0, outscale=1.5)):
        both = ops.esrgan_enhance(imgs, net, **kw)
        for i in range(3):
            assert torch.equal(ops.esrgan_enhance(imgs[i:i + 1], net, **kw), both[i:i + 1]), (kw, i)
        assert torch.equal(ops.esrgan_enhance(imgs, net, **kw), both)
    # a captured replay equals the eager call (one stream: no parallel branches)
    kw = dict(tile=tile, tile_pad=tile_pad, outscale=2, return_x4=True)
    eager = ops.esrgan_enhance(imgs, net, **kw)
    static = imgs.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.esrgan_enhance(static, net, **kw)
    for src in (imgs, imgs.flip(0)):
        static.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        want = ops.esrgan_enhance(src.contiguous(), net, **kw)
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    assert torch.equal(want[0], eager[0].flip(0))


def test_esrgan_enhance_full_depth():
    """23 blocks at 8 x 8, tile 5, pad 2: 2 x 2 tiles of 7 x 7 (the shape of gpen_sr_model.DEEP_CASE)."""
    tag, nb, H, W, tile, tile_pad, pre_pad = M.DEEP_CASE
    c = M.deep_case()
    out, big = ops.esrgan_enhance(dev(c["img"][None]), _net(c["sd"], tag), outscale=2, tile=tile, tile_pad=tile_pad, pre_pad=pre_pad, return_x4=True)
    _check_x4(tag, c, big[0].cpu().numpy())
    assert np.array_equal(out[0].cpu().numpy(), M.resize_lanczos4(big[0].cpu().numpy(), (2 * W, 2 * H)))


def test_esrgan_enhance_refusals_on_the_device():
    net = _net(M.golden_case("6x7.t0")["sd"], "6x7.t0")
    img = torch.zeros((1, 6, 7, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.esrgan_enhance(img, ops.GpenSRNet(1, 64, 4).eval())
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.esrgan_enhance(img.cpu(), net)
    with pytest.raises(ValueError, match="reflect"):
        ops.esrgan_enhance(img, net, pre_pad=6)
    with pytest.raises(ValueError, match="scale 2"):
        ops.esrgan_enhance(img, ops.GpenSRNet(1, 32, 2).eval().to(DEV))
    with pytest.raises(ValueError, match="uint8"):
        ops.esrgan_enhance(img.float(), net)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.esrgan_enhance(img, ops.GpenSRNet(1, 64, 4).to(DEV))


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def esr():
    """A one-block x4 network with conv_last rescaled on a small seeded input, so that the enhanced image spreads over the grey levels."""
    sd = SM.base_state_dict(4, 64, 1, M.CASE_SEED)
    x = SM.images_u8(5, 1, 16, 16).transpose(0, 3, 1, 2).astype(np.float64) / 255.
    net = ops.GpenSRNet(1, 64, 4).eval()
    net.load_state_dict(SM.calibrated(sd, SM.network(sd, x)))
    return net.to(DEV)


@pytest.fixture(scope="module")
def codeformer():
    net = ops.CodeFormer(*CM.CASES["CF-F"]["cfg"]).eval()
    net.load_state_dict(CM.case_weights("CF-F"), strict=True)
    return net.to(DEV)


def test_codeformer_enhance_is_its_pieces(codeformer, esr):
    u8 = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(1, 3, 512, 512), dtype=np.uint8)).to(DEV)
    got = pipeline.codeformer_enhance(codeformer, esr, u8, w=G.W)
    restored = pipeline.codeformer_restore(codeformer, u8, w=G.W)
    want = ops.esrgan_enhance(restored, esr, chw=True, outscale=2)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 3, 1024, 1024) and got.is_contiguous() and tuple(want.shape) == (1, 1024, 1024, 3)
    assert torch.equal(got, want.permute(0, 3, 1, 2))
    assert 8 < len(got.unique())
    # the tiles are the reference's 2 x 2, and the x4 image behind the resize is the model's Lanczos4 source
    out, big = ops.esrgan_enhance(restored, esr, chw=True, outscale=2, return_x4=True)
    assert tuple(big.shape) == (1, 2048, 2048, 3) and torch.equal(out, want) and len(ops.esrgan_tiles(512, 512)) == 4
    rows = slice(780, 828)                                                                    # a band across the tile seam (x4 row 1600), through the model's resize
    band = M.resize_lanczos4(big[0, 2 * rows.start - 8:2 * rows.stop + 8].cpu().numpy(), (1024, rows.stop - rows.start + 8))
    assert np.array_equal(out[0, rows].cpu().numpy(), band[4:-4])
    with pytest.raises(RuntimeError, match="device mismatch"):
        pipeline.codeformer_enhance(codeformer, ops.GpenSRNet(1, 64, 4).eval(), u8)
    with pytest.raises(ValueError, match="upscale"):
        pipeline.codeformer_enhance(codeformer, esr, u8, upscale=0)


@pytest.fixture(scope="module")
def parser(bisenet_sd):
    install_dropin()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    p = FaceParser(seg_ckpt=None, device=DEV)
    p.seg.load_state_dict(bisenet_sd)
    p.seg.eval()
    return p


@pytest.fixture(scope="module")
def blender():
    net = ops.BlenderNet().eval()
    net.referencer.FPN.load_state_dict(seeded.seeded_fpn_state_dict(22))
    net.unet.load_state_dict(seeded.seeded_resunet_state_dict(21, 64))
    with torch.no_grad():
        net.referencer.trainable_tao.fill_(7.0)
    return net.to(DEV)


def test_recolor_frames_is_its_pieces(parser, blender, codeformer, esr):
    swapped = ops.tensor2im_u8(seeded.seeded_image(31, 1, 1024).to(DEV))
    target = ops.tensor2im_u8(seeded.seeded_image(32, 1, 1024).to(DEV))[:, 40:940, :1000].contiguous()
    got = pipeline.recolor_frames(parser, blender, codeformer, esr, swapped, target, flip_target=True, w=G.W)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 1024, 1024, 3) and got.is_contiguous()
    to01 = lambda u8: u8.permute(0, 3, 1, 2).float() / 255                                    # noqa: E731
    tgt = ops.pil_resize(target, (1024, 1024))
    la, lt = parser.parse_batch(to01(swapped), seg12=False), parser.parse_batch(to01(tgt), seg12=False)
    small = pipeline.blender_infer_image(blender, swapped, tgt, la, lt, True)
    recolor = ops.pil_resize(small, (1024, 1024))
    recolor = pipeline.codeformer_enhance(codeformer, esr, recolor.permute(0, 3, 1, 2), w=G.W).permute(0, 2, 3, 1).contiguous()
    want = ops.pil_resize(ops.pil_resize(recolor, (512, 512)), (1024, 1024))
    assert torch.equal(got, want)
    assert 8 < len(got.unique())
    assert pipeline.recolor_frames(parser, blender, codeformer, esr, swapped[:0], target[:0]).shape == (0, 1024, 1024, 3)
    with pytest.raises(ValueError, match="target crops"):
        pipeline.recolor_frames(parser, blender, codeformer, esr, swapped, target.cpu())
    with pytest.raises(RuntimeError, match="training mode"):
        pipeline.recolor_frames(parser, blender, codeformer, ops.GpenSRNet(1, 64, 4).to(DEV), swapped, target)
