"""Row f12 on the GPU: the three kernels of ``csrc/gpen.hip`` alone, ``ops.gpen_forward`` in both arithmetics against the float64 model ``gpen_model`` and the
reference's stored outputs (``tests/golden/g23_gpen.npz``), ``ops.gpen_image`` under the uint8 rule, and the bit-equality properties of the host layer.

Bounds: ``ARITH = "f32"`` is held to ``max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against itself in float64 (never the code under test);
the default ``"sb"`` to ``PIXEL_TOL = 1e-3`` max-abs, the project's bar on generated pixels (tests/test_gpu_synthesis.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gpen_model as GM
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import ops, ops_gpen, pipeline
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
SQRT2 = 2 ** 0.5
_NETS = {}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g23_gpen")


@pytest.fixture(autouse=True)
def _default_arith():
    yield
    ops_gpen.ARITH = "sb"


def _net(tag):
    """``ops.GPEN`` of a case with its seeded weights on the device, one module per case (a module caches its prepared weights)."""
    if tag not in _NETS:
        size, narrow, sdim, _ = GM.CASES[tag]
        net = ops.GPEN(size, sdim, GM.N_MLP, 2, narrow).eval()
        net.load_state_dict(GM.case(tag)["sd"], strict=True)
        _NETS[tag] = net.to(DEV)
    return _NETS[tag]


def _offset(t):
    """A copy of ``t`` that starts one element past a 16-byte boundary: the kernels' one-element form."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 4 != 0 or view.data_ptr() % 16 != 0
    return view


# ------------------------------------------------------------------------------------------------ the kernels alone
def _stem(x, x_u8, w, b, out=None):
    src = x if x is not None else x_u8
    bs, (H, W) = src.shape[0], (src.shape[2:] if x is not None else src.shape[1:3])
    out = torch.empty((bs, w.shape[0], H, W), dtype=torch.float32, device=DEV) if out is None else out
    lib().call("e4s_gpen_stem", _p(out), _p(x), _p(x_u8), _p(w), _p(b), bs, w.shape[0], H, W, _stream())
    return out


@pytest.mark.parametrize("bs,H,W,C0", [(2, 5, 7, 5), (1, 16, 16, 32)])
def test_stem_float_and_uint8(bs, H, W, C0):
    rs = np.random.RandomState(H * W + C0)
    img = rs.randint(0, 256, (bs, H, W, 3)).astype(np.uint8)
    x = GM.img2tensor(img)                                                                    # float32, true division: what FaceGAN.img2tensor gives on the CPU
    w = (rs.standard_normal((C0, 3)) / np.sqrt(3)).astype(np.float32)
    b = rs.uniform(-0.3, 0.3, C0).astype(np.float32)
    xd, ud, wd, bd = T(x).to(DEV), T(img).to(DEV), T(w).to(DEV), T(b).to(DEV)
    got = _stem(xd, None, wd, bd)
    # float64: bias + three products; the kernel's chain is three fused multiply-adds, the activation and the scale: at most 5 roundings of a value below mag
    acc = np.einsum("oc,bchw->bohw", w.astype(np.float64), x.astype(np.float64)) + b.astype(np.float64)[None, :, None, None]
    want = np.where(acc > 0, acc, 0.2 * acc) * np.sqrt(2.0)
    mag = (np.einsum("oc,bchw->bohw", np.abs(w).astype(np.float64), np.abs(x).astype(np.float64)) + np.abs(b)[None, :, None, None]).max() * np.sqrt(2.0)
    err = GM.max_err(got.cpu().numpy(), want)
    record_parity(f"gpen.stem.{H}x{W}.c{C0}", err, 5 * 2.0 ** -24 * mag)
    assert err <= 5 * 2.0 ** -24 * mag
    # stock PyTorch on the device, the reference's composition: the same class of error
    ref = F.leaky_relu(F.conv2d(xd, wd.view(C0, 3, 1, 1)) + bd.view(1, -1, 1, 1), 0.2) * SQRT2
    assert GM.max_err(got.cpu().numpy(), ref.cpu().numpy()) <= 8 * 2.0 ** -24 * mag
    # uint8 input: img2tensor's two roundings inside the kernel give the float input's bits; vector and one-element forms agree bit for bit
    assert torch.equal(_stem(None, ud, wd, bd), got)
    assert torch.equal(_stem(_offset(xd), None, wd, bd), got)
    assert torch.equal(_stem(None, _offset(ud), wd, bd), got)
    assert torch.equal(_stem(xd, None, wd, bd, out=_offset(torch.empty_like(got))), got)


def test_stem_img2tensor_on_all_levels():
    """The uint8 end of the stem for all 256 levels: with an identity weight the uint8 path gives the bits of the float path on NumPy's float32
    ``img2tensor`` chain (a true division, each operation rounded on its own)."""
    img = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    w, b = torch.eye(3, device=DEV), torch.zeros(3, device=DEV)
    from_u8 = _stem(None, T(img).to(DEV), w, b)
    from_f = _stem(T(GM.img2tensor(img)).to(DEV), None, w, b)
    assert torch.equal(from_u8, from_f)


def _noise_half(f, layers, C, outs):
    bs, _, h, w = f.shape
    a, b = layers[0], (layers[1] if len(layers) > 1 else None)
    lib().call("e4s_gpen_noise_half", _p(outs[0][:, C:]), _p(outs[1][:, C:]) if b else None, _p(f), _p(a[0]), _p(b[0]) if b else None, _p(a[1][C:]),
               _p(b[1][C:]) if b else None, bs, C, h * w, 2 * C * h * w, _stream())


@pytest.mark.parametrize("bs,C,h,w", [(2, 3, 5, 7), (1, 32, 16, 16)])
@pytest.mark.parametrize("ndst", [1, 2])
def test_noise_half_is_bit_equal_to_pytorch(bs, C, h, w, ndst):
    g = torch.Generator(device="cpu").manual_seed(C * h + ndst)
    f = torch.randn(bs, C, h, w, generator=g).to(DEV)
    layers = [(torch.tensor([0.37 * (-1) ** k + 0.1], device=DEV), (torch.rand(2 * C, generator=g) - 0.5).to(DEV)) for k in range(ndst)]
    firsts = [torch.randn(bs, C, h, w, generator=g).to(DEV) for _ in range(ndst)]
    for offset in (False, True):
        outs = []
        for y in firsts:
            o = torch.full((bs, 2 * C, h, w), float("nan"), device=DEV)
            o = _offset(o) if offset else o
            o[:, :C] = y
            outs.append(o)
        _noise_half(_offset(f) if offset else f, layers, C, outs)
        for (nw, bias), y, o in zip(layers, firsts, outs):
            want = SQRT2 * F.leaky_relu(torch.cat((y, nw * f), 1) + bias.view(1, -1, 1, 1), 0.2)      # gpen_model.py:294-302, fused_act.py:96
            assert torch.equal(o[:, C:], want[:, C:])
            assert torch.equal(o[:, :C], y)                                                   # the first half is not touched


@pytest.mark.parametrize("bs,H,W", [(2, 5, 7), (1, 16, 16)])
def test_to_u8_is_numpys(bs, H, W):
    rs = np.random.RandomState(H)
    x = rs.uniform(-1.3, 1.3, (bs, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    # values exactly on a level boundary and one float32 step (below 1.2e-7) to either side of it; the range gives values below 0 and above 1 of the clip
    levels = rs.randint(1, 255, flat.size // 2)
    edge = ((levels / 255.0 - 0.5) / 0.5).astype(np.float32)
    step = np.float32(rs.randint(-1, 2, edge.size) * 2)                                       # -2, 0 or 2: the direction of the step, 0 for none
    flat[: edge.size] = np.where(step == 0, edge, np.nextafter(edge, step))
    flat[edge.size: edge.size + 8] = np.float32([-1.0, 1.0, -1.0000001, 1.0000001, 0.0, -0.99999994, 0.99999994, 5.0])
    x = flat.reshape(bs, 3, H, W)
    assert (x < -1).any() and (x > 1).any()
    want = GM.tensor2img(x)                                                                   # NumPy in float32, FaceGAN.tensor2img's expressions
    xd = T(x).to(DEV)
    got = ops.gpen_to_u8(xd)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.gpen_to_u8(_offset(xd)).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("tag", list(GM.CASES))
def test_forward_f32_against_the_model_and_the_reference(tag, golden):
    c = GM.case(tag)
    ops_gpen.ARITH = "f32"
    out, latent = ops.gpen_forward(T(c["x"]).to(DEV), _net(tag), return_latents=True)
    got = out.cpu().numpy()
    bar = GM.bound(c["e32"], c["want"])
    err, err_ref = GM.max_err(got, c["want"]), GM.max_err(got, golden[f"{tag}.out"])
    err_lat = GM.max_err(latent.cpu().numpy(), c["latent"])
    print(f"{tag}: f32 against float64 {err:.3e} = {err / c['e32']:.2f} e32, against the reference {err_ref:.3e}, latent {err_lat:.3e} = {err_lat / c['e32_latent']:.2f} e32")
    record_parity(f"gpen.f32.{tag}.err_over_e32", err / c["e32"], GM.MARGIN)
    record_parity(f"gpen.f32.{tag}.maxabs", err, bar)
    record_parity(f"gpen.f32.{tag}.maxabs_reference", err_ref, bar)
    assert err <= bar
    assert err_ref <= bar
    assert latent.shape == c["latent"].shape and err_lat <= GM.bound(c["e32_latent"], c["latent"])
    if tag == GM.LATENT_CASE:
        assert GM.max_err(latent.cpu().numpy(), golden[f"{tag}.latent"]) <= GM.bound(c["e32_latent"], c["latent"])


@pytest.mark.parametrize("tag", list(GM.CASES))
def test_forward_sb_meets_the_pixel_bar(tag, golden):
    c = GM.case(tag)
    assert ops_gpen.ARITH == "sb"
    got = ops.gpen_forward(T(c["x"]).to(DEV), _net(tag))[0].cpu().numpy()
    err, err_ref = GM.max_err(got, c["want"]), GM.max_err(got, golden[f"{tag}.out"])
    print(f"{tag}: sb against float64 {err:.3e} = {err / c['e32']:.1f} e32, against the reference {err_ref:.3e}")
    record_parity(f"gpen.sb.{tag}.err_over_e32", err / c["e32"])
    record_parity(f"gpen.sb.{tag}.maxabs", err, GM.PIXEL_TOL)
    assert err <= GM.PIXEL_TOL and err_ref <= GM.PIXEL_TOL


@pytest.mark.parametrize("tag", ["s16", "s64"])
def test_image_follows_the_uint8_rule(tag):
    c = GM.case(tag)
    img, net = T(c["img"]).to(DEV), _net(tag)
    ops_gpen.ARITH = "f32"
    got = ops.gpen_image(img, net)
    assert got.dtype == torch.uint8 and got.shape == img.shape
    share = GM.check_u8(got.cpu().numpy(), c["u"], c["e32"])
    assert share >= 0.99
    assert torch.equal(pipeline.gpen_enhance(net, img), got)
    ops_gpen.ARITH = "sb"
    sb = ops.gpen_image(img, net).cpu().numpy().astype(np.int32)
    off = np.abs(sb - GM.expected_u8(c["u"]).astype(np.int32))
    record_parity(f"gpen.image.sb.{tag}.levels_off", int(off.max()), 1, note=f"{(off > 0).mean():.4f} of the values differ; f32 strict share {share:.4f}")
    assert off.max() <= 1
    with pytest.raises(ValueError, match=str(GM.CASES[tag][0])):
        ops.gpen_image(img[:, :-1], net)


def test_bit_equalities():
    tag = "s32"
    c = GM.case(tag)
    x, net = T(c["x"]).to(DEV), _net(tag)
    out, latent = ops.gpen_forward(x, net, return_latents=True)
    assert torch.equal(out, ops.gpen_forward(x, net)[0])                                      # two runs
    for b in range(x.shape[0]):                                                               # a batch against its single samples
        one, lat = ops.gpen_forward(x[b:b + 1], net, return_latents=True)
        assert torch.equal(one[0], out[b]) and torch.equal(lat[0], latent[b])
    assert torch.equal(out, ops.gpen_forward(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), net)[0])      # strides do not matter
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    assert torch.equal(out, ops.gpen_forward(x, sd)[0])                                       # a mapping as weights
    assert ops.gpen_forward(x[:0], net)[0].shape == (0, 3, 32, 32)
    install_dropin()
    from swap_face_fine.gpen.face_model.gpen_model import FullGenerator
    size, narrow, sdim, _ = GM.CASES[tag]
    full = FullGenerator(size, sdim, GM.N_MLP, channel_multiplier=2, narrow=narrow, device="cuda").eval()
    full.load_state_dict(c["sd"], strict=True)
    full = full.to(DEV)
    img, none = full(x)
    assert none is None and torch.equal(img, out)
    img, lat = full(x, return_latents=True)
    assert torch.equal(lat, latent)
    with pytest.raises(NotImplementedError, match="truncation"):
        full(x, truncation=0.7)
    with pytest.raises(NotImplementedError, match="eval"):
        full.train()(x)


def test_graph_replay_gives_the_eager_bits():
    tag = "s32"
    x, net = T(GM.case(tag)["x"]).to(DEV), _net(tag)
    eager = ops.gpen_forward(x, net)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gpen_forward(x, net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gpen_forward(x, net)[0]
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_prepared_weights_follow_the_parameters():
    tag = "s16"
    c = GM.case(tag)
    size, narrow, sdim, _ = GM.CASES[tag]
    x = T(c["x"]).to(DEV)
    net = ops.GPEN(size, sdim, GM.N_MLP, 2, narrow).eval()
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.gpen_forward(x, net.to(DEV))
    net.load_state_dict(c["sd"], strict=True)
    net = net.to(DEV)
    before = ops.gpen_forward(x, net)[0]
    with torch.no_grad():
        net.generator.to_rgbs[1].bias.add_(0.25)                                              # in place: the same storage, a new version
    after = ops.gpen_forward(x, net)[0]
    assert np.abs((after - before).cpu().numpy() - 0.25).max() <= 1e-5
    net.ecd1[0][1].weight.data.mul_(-2.0)                                                     # behind autograd's back: no trace to key on (a re-laid-out weight)
    assert torch.equal(ops.gpen_forward(x, net)[0], after)
    assert ops.invalidate_weight_caches(net) >= 1
    assert GM.max_err(ops.gpen_forward(x, net)[0].cpu().numpy(), after.cpu().numpy()) > 1e-2


def test_argument_errors_before_any_launch():
    tag = "s16"
    c = GM.case(tag)
    x, net = T(c["x"]).to(DEV), _net(tag)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.gpen_forward(x.cpu(), net)
    with pytest.raises(ValueError, match="float32"):
        ops.gpen_forward(x.double(), net)
    with pytest.raises(ValueError, match="16"):
        ops.gpen_forward(x[:, :, :8, :8], net)
    net.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            ops.gpen_forward(x, net)
    finally:
        net.eval()
    ops_gpen.ARITH = "bf16"
    with pytest.raises(ValueError, match="ARITH"):
        ops.gpen_forward(x, net)
