"""Row f11 on the GPU: the four kernels of ``csrc/rrdb.hip`` alone, ``ops.realesr_forward`` against the float64 model ``rrdb_model``, the wrappers
``pipeline.realesr_infer_batch`` / ``realesr_infer_image`` / the drop-in ``RealESRBatchInfer``, and ``color_transfer_blender`` /
``swap_images(ct_mode='blender', recolor_nets=...)`` against the composition of their pieces.

The bound of a network case is ``max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against itself in float64 (never the code under test); the
uint8 images follow ``rrdb_model``'s uint8 rule.  Kernel bounds are rounding counts: see each test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rrdb_model as RM
from conftest import install_dropin, record_parity
from e4s2024_amd import align, ops, pipeline, seeded
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
_WORST = {"ratio": 0.0}
_NETS = {}


def _net(sd, key):
    """``ops.RRDBNet`` with ``sd`` on the device, one module per ``key`` (a module caches its prepared weights)."""
    if key not in _NETS:
        net = ops.RRDBNet(RM.num_blocks(sd)).eval()
        net.load_state_dict(sd, strict=True)
        _NETS[key] = net.to(DEV)
    return _NETS[key]


def _offset(t):
    """A copy of ``t`` that starts 4 bytes (one float; for uint8 one byte) past a 16-byte boundary: the kernels' one-element form."""
    if t is None:
        return None
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


# ------------------------------------------------------------------------------------------------ the kernels alone
def _esr_input(img, oh, ow, out=None):
    bs, H, W, _ = img.shape
    out = torch.empty((bs, 3, oh, ow), dtype=torch.float32, device=DEV) if out is None else out
    lib().call("e4s_esr_input", _p(out), _p(img), bs, H, W, oh, ow, _stream())
    return out


def _torch_input_chain(img, oh, ow):
    x = img.permute(0, 3, 1, 2).float()
    x = (x / 127.5) - 1.
    x = (x * 0.5 + 0.5).clamp(0, 1)
    return F.interpolate(x.contiguous(), size=(oh, ow), mode="bilinear", align_corners=True)


@pytest.mark.parametrize("H,W,oh,ow", [(1, 1, 3, 2), (5, 7, 4, 4), (300, 280, 256, 256), (256, 256, 256, 256)])
def test_esr_input(H, W, oh, ow):
    """Against float64 and against stock PyTorch on the device within 2e-7 of the largest value (three float32 roundings at 1.0: the value, its blend along a
    row, the blend of two rows); at equal sizes, where the resize picks single pixels, bit for bit the torch chain.  The float64 side takes the float32 source
    coordinates every float32 resize uses (``rrdb_model.aten_coords``): the image is rough on purpose, and a float64 coordinate would move a value by the
    coordinate's float32 ulp times the difference of two neighbours, which is no property of this kernel."""
    img = T(RM.images_u8(H * 1000 + W, 2, H, W)).to(DEV)
    got = _esr_input(img, oh, ow)
    stock = _torch_input_chain(img, oh, ow)
    want = RM.esr_input_f32_coords(img.cpu().numpy(), oh, ow)
    err64, err_stock = RM.max_err(got.cpu().numpy(), want), RM.max_err(got.cpu().numpy(), stock.cpu().numpy())
    print(f"{H}x{W} -> {oh}x{ow}: against float64 {err64:.3e}, against stock PyTorch {err_stock:.3e}, largest value {np.abs(want).max():.3f}")
    assert got.min() >= 0 and got.max() <= 1
    assert err64 <= 2e-7 * np.abs(want).max() and err_stock <= 2e-7 * np.abs(want).max()
    if (H, W) == (oh, ow):
        assert torch.equal(got, stock)
    assert torch.equal(_esr_input(img, oh, ow, _offset(got)), got)                            # the one-element form: the same bits
    assert torch.equal(_esr_input(img, oh, ow), got)
    assert _esr_input(img[:0], oh, ow).shape == (0, 3, oh, ow)


@pytest.mark.parametrize("planes,hw", [(1, 1), (3, 35), (64, 63), (64, 1024)])
def test_scale_add_equals_stock_pytorch(planes, hw):
    t = T(seeded.seeded_array(1, "esr.t", (planes, hw), 0.0, 30.0)).to(DEV)
    x = T(seeded.seeded_array(2, "esr.r", (planes, hw), 0.0, 30.0)).to(DEV)
    want = t * 0.2 + x

    def run(y, t, x):
        lib().call("e4s_esr_scale_add", _p(y), _p(t), _p(x), planes, hw, _stream())
        return y

    assert torch.equal(run(torch.empty_like(x), t, x), want)
    assert torch.equal(run(_offset(x), _offset(t), _offset(x)), want)                         # a view at a 4-byte offset
    assert torch.equal(run(torch.empty_like(x), _offset(t), x), want)                         # mixed alignment takes the one-element form too
    y = x.clone()
    assert torch.equal(run(y, t, y), want)                                                    # in place over x, as the network calls it


@pytest.mark.parametrize("planes,h,w", [(1, 1, 1), (3, 5, 7), (2, 6, 8), (64, 9, 12)])
def test_up2_equals_stock_pytorch(planes, h, w):
    x = T(seeded.seeded_array(3, "esr.up", (planes, h, w))).to(DEV)
    want = F.interpolate(x[None], scale_factor=2, mode="nearest")[0]

    def run(out, x):
        lib().call("e4s_esr_up2", _p(out), _p(x), planes, h, w, _stream())
        return out

    assert torch.equal(run(torch.empty_like(want), x), want)
    assert torch.equal(run(_offset(want), _offset(x)), want)
    assert torch.equal(run(torch.empty_like(want), _offset(x)), want)


def _tail(x, w, b, out_f=True, off=False):
    bs, _, H, W = x.shape
    u8 = torch.empty((bs, H, W, 3), dtype=torch.uint8, device=DEV)
    f = torch.empty((bs, 3, H, W), dtype=torch.float32, device=DEV) if out_f else None
    if off:
        x, u8, f = _offset(x), _offset(u8), _offset(f)
    lib().call("e4s_esr_tail", _p(u8), _p(f), _p(x), _p(w), _p(b), bs, H, W, _stream())
    return u8, f


def _tail_inputs(H, W, bs=2):
    # (a 1 x 1 image fills one tap of nine: three times the input for the same spread of the output)
    x = T(seeded.seeded_array(5, "esr.tail.x", (bs, 64, H, W), 0.0, 3.0 if H * W == 1 else 1.0, "normal")).to(DEV)
    w = seeded.seeded_array(5, "esr.tail.w", (3, 64, 3, 3), 0.0, 0.25 / np.sqrt(576.0), "normal")
    return x, w, np.array([0.5, 0.45, 0.55], dtype=np.float32)


@pytest.mark.parametrize("H,W", [(5, 7), (16, 64), (20, 68), (67, 130)])
def test_both_tails_run_one_tile(H, W):
    """``e4s_esr_tail`` and ``e4s_gsr_tail`` at 64 channels without crop or flip: the same float output bit for bit (5 x 7 and 67 x 130 in the one-element form,
    16 x 64 one whole tile, 20 x 68 the vector form with a ragged tile), and two uint8 images, since the two ends differ."""
    x, w, b = _tail_inputs(H, W)
    w, b = T(w).to(DEV), T(b).to(DEV)
    esr_u8, esr_f = _tail(x, w, b)
    gsr_u8, gsr_f = torch.empty_like(esr_u8), torch.empty_like(esr_f)
    lib().call("e4s_gsr_tail", _p(gsr_u8), _p(gsr_f), _p(x), _p(w), _p(b), x.shape[0], 64, H, W, H, W, 0, _stream())
    assert torch.equal(esr_f, gsr_f)
    assert not torch.equal(esr_u8, gsr_u8)


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (67, 130), (16, 64), (20, 68)])
def test_tail_against_float64(H, W):
    """The float output within (577 + 1) 2^-24 max(sum |w x| + |b|) of float64; the uint8 image by the uint8 rule, its ``e32`` the same sum in float32 in the
    kernel's documented order (``rrdb_model.tail_f32``); the form at a 4-byte offset and the call without the float output give the same bits.  67 x 130
    spans tiles in both directions, 16 x 64 is one whole tile, 20 x 68 has a multiple-of-four width that is no multiple of the tile."""
    x, w, b = _tail_inputs(H, W)
    m = RM.tail(x.cpu().numpy(), w, b)
    u8, f = _tail(x, T(w).to(DEV), T(b).to(DEV))
    err = RM.max_err(f.cpu().numpy(), m["r"])
    strict, clamped, std = RM.check_u8(u8.cpu().numpy(), m["u"], m["e32"])
    print(f"{H}x{W}: float output against float64 {err:.3e} = {err / m['e32']:.2f} e32, bound {m['bound']:.3e}; strict {100 * strict:.2f} %, "
          f"clamped {100 * clamped:.2f} %, std {std:.1f}")
    assert err <= m["bound"]
    assert strict >= 0.99 and clamped < 0.10 and std > 30
    u8_off, f_off = _tail(x, T(w).to(DEV), T(b).to(DEV), off=True)
    assert torch.equal(u8_off, u8) and torch.equal(f_off, f)
    assert torch.equal(_tail(x, T(w).to(DEV), T(b).to(DEV), out_f=False)[0], u8)


# ------------------------------------------------------------------------------------------------ realesr_forward
@pytest.mark.parametrize("tag", list(RM.CASES))
def test_network_against_the_float64_model(tag):
    c = RM.case(tag)
    nb, h, w, bs = RM.CASES[tag]
    out = ops.realesr_forward(T(c["x"]).to(DEV), _net(c["sd"], tag))
    assert out.dtype == torch.float32 and tuple(out.shape) == (bs, 3, 4 * h, 4 * w) and out.is_contiguous()
    err, bound = RM.max_err(out.cpu().numpy(), c["want"]), RM.bound(c["e32"], c["want"])
    _WORST["ratio"] = max(_WORST["ratio"], err / c["e32"])
    print(f"{tag}: kernels against float64 {err:.3e} = {err / c['e32']:.2f} e32, e32 {c['e32']:.3e}, bound {bound:.3e}")
    record_parity("rrdb.worst_err_over_e32", _WORST["ratio"], RM.MARGIN, "realesr_forward against the float64 model, in units of the float32 model's own error")
    assert err <= bound


@pytest.mark.parametrize("tag", ["b2.12x20", "b1.5x3"])
def test_realesr_forward_is_gpen_sr_forward_at_width_64_and_scale_4(tag):
    """Rows f11 and f16 run one network: on the same weights the two public calls give the same bits, for one sample and for a batch of two."""
    c = RM.case(tag)
    net = _net(c["sd"], tag)
    for x in (T(c["x"]), T(RM.images01(12, 2, 6, 10))):
        x = x.to(DEV)
        assert torch.equal(ops.realesr_forward(x, net), ops.gpen_sr_forward(x, net))


def test_batch_runs_mappings_and_empty_batches():
    tag = "b23.8x8.bs2"
    c = RM.case(tag)
    x, net = T(c["x"]).to(DEV), _net(c["sd"], tag)
    out = ops.realesr_forward(x, net)
    assert torch.equal(out, ops.realesr_forward(x, net))                                      # two runs: the same bits
    assert torch.equal(out, torch.cat([ops.realesr_forward(x[i:i + 1], net) for i in range(2)]))
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    assert torch.equal(out, ops.realesr_forward(x, sd))                                       # a mapping as weights
    assert torch.equal(out, ops.realesr_forward(x, {"params_ema": sd}))
    assert torch.equal(out, ops.realesr_forward(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), net))         # strides do not matter
    assert ops.realesr_forward(x[:0], net).shape == (0, 3, 32, 32)


def test_graph_replay_gives_the_eager_bits():
    tag = "b2.12x20"
    c = RM.case(tag)
    x, net = T(c["x"]).to(DEV), _net(c["sd"], tag)
    eager = ops.realesr_forward(x, net)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.realesr_forward(x, net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.realesr_forward(x, net)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_prepared_weights_follow_updates():
    tag = "b1.5x3"
    c = RM.case(tag)
    x = T(c["x"]).to(DEV)
    net = ops.RRDBNet(1).eval()
    net.load_state_dict(c["sd"])
    net = net.to(DEV)
    before = ops.realesr_forward(x, net)
    with torch.no_grad():
        net.conv_last.bias.add_(0.5)                                                          # in place: the same storage, a new version
    after = ops.realesr_forward(x, net)
    assert np.abs((after - before).cpu().numpy() - 0.5).max() <= 1e-5
    net.body[0].rdb2.conv5.weight.data.mul_(1.5)                                              # behind autograd's back: no trace to key on
    assert torch.equal(ops.realesr_forward(x, net), after)
    assert ops.invalidate_weight_caches(net) >= 1
    moved = ops.realesr_forward(x, net)
    assert RM.max_err(moved.cpu().numpy(), after.cpu().numpy()) > 1e-3
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    want = RM.network(sd, c["x"]).numpy()
    e32 = RM.max_err(RM.network(sd, c["x"], torch.float32).numpy(), want)
    assert RM.max_err(moved.cpu().numpy(), want) <= RM.bound(e32, want)


# ------------------------------------------------------------------------------------------------ the wrappers
@pytest.mark.parametrize("tag", list(RM.IMAGE_CASES))
def test_infer_image_against_the_float64_model(tag):
    c = RM.image_case(tag)
    img, net = T(c["img"]).to(DEV), _net(c["sd"], tag)
    got = pipeline.realesr_infer_image(net, img, in_size=c["in_size"], out_size=c["out_size"])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (img.shape[0], c["out_size"], c["out_size"], 3) and got.is_contiguous()
    strict, clamped, std = RM.check_u8(got.cpu().numpy(), c["u"], c["e32"])
    print(f"{tag}: e32 {c['e32']:.3e}, strict {100 * strict:.2f} %, clamped {100 * clamped:.2f} %, std {std:.1f} grey levels")
    assert strict >= 0.99 and clamped < 0.10 and std > 30
    # the float route through the same pieces: the network's output inside the bound, and the image it implies
    r = ops.realesr_forward(ops.realesr_input(img, (c["in_size"], c["in_size"])), net)
    err = RM.max_err(r.cpu().numpy(), c["want"])
    _WORST["ratio"] = max(_WORST["ratio"], err / c["e32"])
    record_parity("rrdb.worst_err_over_e32", _WORST["ratio"], RM.MARGIN, "realesr_forward against the float64 model, in units of the float32 model's own error")
    assert err <= RM.bound(c["e32"], c["want"])
    assert torch.equal(got, ((r * 2. - 1.).clamp(-1, 1) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1))
    assert pipeline.realesr_infer_image(net, img[:0], in_size=c["in_size"], out_size=c["out_size"]).shape == (0, c["out_size"], c["out_size"], 3)


def test_infer_image_at_the_reference_sizes():
    """256 -> 1024 with one block, checked on the two corners where the float64 model is evaluated (``rrdb_model.real_case``)."""
    c = RM.real_case()
    img, net = T(c["img"]).to(DEV), _net(c["sd"], "real")
    got = pipeline.realesr_infer_image(net, img)
    assert tuple(got.shape) == (1, pipeline.ESR_OUT, pipeline.ESR_OUT, 3) and (pipeline.ESR_IN, pipeline.ESR_OUT) == (c["in_size"], c["out_size"])
    g = got.cpu().numpy()
    for (ys, xs), u in c["parts"]:
        strict, clamped, std = RM.check_u8(g[:, ys, xs], u, c["e32"])
        print(f"corner {ys}, {xs}: e32 {c['e32']:.3e}, strict {100 * strict:.2f} %, clamped {100 * clamped:.2f} %, std {std:.1f} grey levels")
        assert strict >= 0.99 and clamped < 0.10 and std > 30


def test_whole_frame_at_the_reference_sizes():
    """The corners above leave the inside of the 1024 x 1024 frame unchecked.  Here the float64 model itself runs on the device (stock PyTorch's float64
    convolutions, which no library kernel of the float32 path serves), so every tile of the tail and of the convolutions at 256, 512 and 1024 is held to
    the case's bound and the whole image to the uint8 rule.  ``e32`` is the case's, from the model on the CPU."""
    c = RM.real_case()
    img, net = T(c["img"]).to(DEV), _net(c["sd"], "real")
    want = RM.network(c["sd"], RM.esr_input(c["img"], c["in_size"], c["in_size"]).to(DEV))
    got = ops.realesr_forward(ops.realesr_input(img, (c["in_size"], c["in_size"])), net)
    assert tuple(got.shape) == tuple(want.shape) == (1, 3, pipeline.ESR_OUT, pipeline.ESR_OUT) and want.dtype == torch.float64
    err, bound = float((got.double() - want).abs().max()), RM.bound(c["e32"], want.cpu().numpy())
    _WORST["ratio"] = max(_WORST["ratio"], err / c["e32"])
    print(f"whole frame {tuple(got.shape)}: kernels against float64 {err:.3e} = {err / c['e32']:.2f} e32, e32 {c['e32']:.3e}, bound {bound:.3e}")
    record_parity("rrdb.worst_err_over_e32", _WORST["ratio"], RM.MARGIN, "realesr_forward against the float64 model, in units of the float32 model's own error")
    assert err <= bound
    strict, clamped, std = RM.check_u8(pipeline.realesr_infer_image(net, img).cpu().numpy(), RM.to_u8(want.cpu())[0], c["e32"])
    print(f"whole frame: strict {100 * strict:.2f} %, clamped {100 * clamped:.2f} %, std {std:.1f} grey levels")
    assert strict >= 0.99 and clamped < 0.10 and std > 30


def test_infer_batch_and_the_general_output_size():
    tag = "img.40x36"
    c = RM.image_case(tag)
    net = _net(c["sd"], tag)
    x = T(RM.images01(9, 2, 11, 13) * 2.4 - 1.2).to(DEV)                                       # beyond [-1, 1]: the first clamp works
    for out_hw in (None, (32, 32), (20, 45)):
        got = pipeline.realesr_infer_batch(net, x, out_hw, in_size=8)
        want = RM.infer_batch(c["sd"], x.cpu().numpy(), out_hw, in_size=8)
        w32 = RM.infer_batch(c["sd"], x.cpu().numpy(), out_hw, in_size=8, dtype=torch.float32)
        e32 = RM.max_err(w32.numpy(), want.numpy())
        assert tuple(got.shape) == tuple(want.shape) and got.min() >= -1 and got.max() <= 1
        err = RM.max_err(got.cpu().numpy(), want.numpy())
        print(f"infer_batch to {out_hw}: {err:.3e} = {err / e32:.2f} e32")
        assert err <= RM.bound(e32, want.numpy())
    # realesr_infer_image at an output size that is not four times the input's: through ops.bilinear_resize
    img = T(c["img"]).to(DEV)
    got = pipeline.realesr_infer_image(net, img, in_size=8, out_size=20)
    r = ops.bilinear_resize(ops.realesr_forward(ops.realesr_input(img, (8, 8)), net), (20, 20), align_corners=True)
    assert torch.equal(got, ((r * 2. - 1.).clamp(-1, 1) * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1))


def test_dropin_infer_image_is_realesr_infer_image(tmp_path, monkeypatch):
    """The drop-in at the reference's configuration, 23 blocks from 256 x 256 to 1024 x 1024, once, inside a stand-in for the reference tree with the
    checkpoint where the reference keeps it: a file with ``params_ema`` and an unusable ``params`` loads the former; ``infer_image`` on a PIL image and
    ``infer_batch`` are the pipeline's calls."""
    from PIL import Image
    from test_rrdb_cpu import fake_reference_tree
    install_dropin()
    from swap_face_fine.realesr import image_infer
    sd = RM.base_state_dict(23)
    ckpt = fake_reference_tree(tmp_path, monkeypatch)
    ckpt.parent.mkdir(parents=True)
    torch.save({"params": {}, "params_ema": sd}, str(ckpt))
    esr = image_infer.RealESRBatchInfer()
    assert esr.args.model_path == str(ckpt) and all(torch.equal(v.cpu(), sd[k]) for k, v in esr.model.state_dict().items())
    assert not esr.model.training and next(esr.model.parameters()).is_cuda
    img = RM.images_u8(4, 1, 40, 36)
    out = esr.infer_image(Image.fromarray(img[0]))
    assert isinstance(out, Image.Image) and out.size == (1024, 1024) and out.mode == "RGB"
    assert np.array_equal(np.array(out), pipeline.realesr_infer_image(esr.model, T(img).to(DEV))[0].cpu().numpy())
    x = T(RM.images01(10, 1, 9, 9) * 2 - 1).to(DEV)
    got = esr.infer_batch(x, (64, 48))
    assert tuple(got.shape) == (1, 3, 64, 48) and torch.equal(got, pipeline.realesr_infer_batch(esr.model, x, (64, 48)))
    assert tuple(esr.infer_batch(x).shape) == (1, 3, 9, 9)


# ------------------------------------------------------------------------------------------------ ct_mode 'blender'
@pytest.fixture(scope="module")
def parser(bisenet_sd):
    install_dropin()
    from swap_face_fine.face_parsing.face_parsing_demo import FaceParser
    p = FaceParser(seg_ckpt=None, device=DEV)
    p.seg.load_state_dict(bisenet_sd)
    p.seg.eval()
    return p


@pytest.fixture(scope="module")
def nets():
    """(BlenderNet with seeded weights and tau = 7, a two-block RRDBNet): the depth of the second is pinned above and costs time here.  conv_last is
    rescaled on a small seeded input, so that the enhanced image spreads over the grey levels."""
    blender = ops.BlenderNet().eval()
    blender.referencer.FPN.load_state_dict(seeded.seeded_fpn_state_dict(22))
    blender.unet.load_state_dict(seeded.seeded_resunet_state_dict(21, 64))
    with torch.no_grad():
        blender.referencer.trainable_tao.fill_(7.0)
    esr = ops.RRDBNet(2).eval()
    esr.load_state_dict(RM.calibrated(RM.base_state_dict(2), RM.network(RM.base_state_dict(2), RM.images01(1, 1, 16, 16))))
    return blender.to(DEV), esr.to(DEV)


def test_color_transfer_blender_is_its_pieces(parser, nets):
    blender, esr = nets
    a = seeded.seeded_image(31, 2, 1024).to(DEV)
    t = seeded.seeded_image(32, 2, 1024).to(DEV)
    a_u8, t_u8 = ops.tensor2im_u8(a), ops.tensor2im_u8(t)
    got = pipeline.color_transfer_blender(a_u8, t_u8, parser, blender, esr, flip_target=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 1024, 1024, 3) and got.is_contiguous()
    to01 = lambda u8: u8.permute(0, 3, 1, 2).float() / 255                                    # noqa: E731
    la, lt = parser.parse_batch(to01(a_u8), seg12=False), parser.parse_batch(to01(t_u8), seg12=False)
    small = pipeline.blender_infer_image(blender, a_u8, t_u8, la, lt, True)
    want = pipeline.realesr_infer_image(esr, ops.pil_resize(small, (1024, 1024)))
    assert torch.equal(got, want)
    assert got.float().std() > 30                                                             # (an image over the grey levels, not a constant)
    assert pipeline.color_transfer_blender(a_u8[:0], t_u8[:0], parser, blender, esr).shape == (0, 1024, 1024, 3)


def test_swap_images_with_the_blender_mode_bs2(gpu_net3, parser, nets):
    import align_model as M
    from test_gpu_softpaste import _outside_quad
    rng = np.random.default_rng(15)
    frames = np.stack([M.make_frame(rng, 1080, 1920) for _ in range(2)])
    quads = np.stack([M.square_quad(960, 540, 300, 0.35), M.square_quad(1800, 120, 380, -0.5)])
    plan = align.crop_plan(quads, (1080, 1920), 1024)
    driven = seeded.seeded_image(16, 2, 1024).to(DEV)
    fr = T(frames).to(DEV)
    np.random.seed(3)
    got = pipeline.swap_images(gpu_net3, parser, driven, fr, plan, ct_mode="blender", recolor_nets=nets)
    assert got.shape == fr.shape and got.dtype == torch.uint8 and torch.equal(fr.cpu(), T(frames))
    np.random.seed(3)
    flip = ops.flip_choice(None)                                                              # the one draw the call made
    via_fn = pipeline.swap_images(gpu_net3, parser, driven, fr, plan,
                                  recolor_fn=lambda s, c: pipeline.color_transfer_blender(s, c, parser, *nets, flip_target=flip))
    assert torch.equal(got, via_fn)
    g = got.cpu().numpy()
    plain = pipeline.swap_images(gpu_net3, parser, driven, fr, plan, recolor_fn=lambda s, c: s).cpu().numpy()
    for i in range(2):
        x0, y0, x1, y1 = plan.paste_boxes[i].tolist()
        outside = _outside_quad(np.asarray(plan.quads[i], dtype=np.float64), g.shape[1], g.shape[2])
        outside[:y0], outside[y1:], outside[:, :x0], outside[:, x1:] = True, True, True, True
        assert np.array_equal(g[i][outside], frames[i][outside])             # every pixel outside the quads untouched
        assert (g[i][~outside] != plain[i][~outside]).any()                  # and another face inside them than without the colour transfer
