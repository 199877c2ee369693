"""Row f18 on the GPU: the 7-tap convolution, the strided 3 x 3 x 3 convolution and pool and the two glue kernels alone, then ``dense_motion_forward`` against
the float64 model ``vid2vid_motion_model`` under its bars (``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64;
test_vid2vid_motion_cpu.py pins those bars from the other side with mutants and holds the reference's stored outputs to them) and against the reference's stored
outputs.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vid2vid_motion_model as M
from conftest import load_golden, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_RTOL = 2e-6                             # the project's bar for the three-way bf16 split, as for e4s_conv3d_sb3
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731

# (cin, cout, D, H, W, kd, sigmoid)
K7_SHAPES = [(21, 6, 2, 5, 9, 7, False),     # every tap partly in the padding, extents below the radius
             (112, 16, 4, 16, 16, 7, False), (16, 1, 3, 8, 40, 7, False), (35, 21, 5, 12, 8, 7, False), (17, 32, 7, 7, 7, 7, False),
             (48, 1, 1, 16, 16, 1, True), (100, 3, 1, 9, 33, 1, False)]


@pytest.fixture(scope="module")
def golden():
    return load_golden("g29_vid2vid_motion")


@pytest.fixture(scope="module")
def ops():
    from e4s2024_amd import ops
    return ops


def _rand(seed, *shape, std=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * np.float32(std))


_K7 = {}


def _k7_case(shape, bs=1):
    """(x, bias, slabs) on the device and the float64 reference of one shape, made once."""
    if (shape, bs) not in _K7:
        from e4s2024_amd import ops
        cin, cout, D, H, W, kd, sig = shape
        seed = sum(shape[:6]) + bs
        x, w = _rand(seed, bs, cin, D, H, W), _rand(seed + 1, cout, cin, kd, 7, 7, std=1.0 / np.sqrt(49 * kd * cin))
        bias = _rand(seed + 2, cout, std=0.5)
        ref = F.conv3d(x.double(), w.double(), bias.double(), padding=(kd // 2, 3, 3))
        _K7[shape, bs] = (x.to(DEV), bias.to(DEV), ops.prep_conv3d_k7(w.to(DEV)), torch.sigmoid(ref) if sig else ref, w)
    return _K7[shape, bs]


@pytest.mark.parametrize("shape", K7_SHAPES, ids=lambda s: "x".join(map(str, s[:6])))
def test_conv3d_k7_against_float64(ops, shape):
    x, bias, slabs, ref, w = _k7_case(shape)
    got = ops.conv3d_k7(x, slabs, bias, sigmoid=shape[6])
    assert got.shape == ref.shape and got.dtype == torch.float32
    err, bar = M.max_err(got.cpu().numpy(), ref.numpy()), FP32_RTOL * float(ref.abs().max())
    record_parity(f"conv3d_k7_sb3.{'x'.join(map(str, shape[:6]))}", err, bar)
    assert err <= bar
    if shape[5] == 1:                            # the Conv2d form: a 4-D weight and a 4-D input, the same bits
        got2 = ops.conv3d_k7(x[:, :, 0], ops.prep_conv3d_k7(w[:, :, 0].contiguous().to(DEV)), bias, sigmoid=shape[6])
        assert got2.shape == got[:, :, 0].shape and torch.equal(got2, got[:, :, 0])
        ref2 = F.conv2d(x[:, :, 0].double().cpu(), w[:, :, 0].double(), bias.double().cpu(), padding=3)
        assert M.max_err(got2.cpu().numpy(), (torch.sigmoid(ref2) if shape[6] else ref2).numpy()) <= bar


@pytest.mark.parametrize("shape", [K7_SHAPES[0], K7_SHAPES[3], K7_SHAPES[6]], ids=lambda s: "x".join(map(str, s[:6])))
def test_conv3d_k7_bit_for_bit_properties(ops, shape):
    x, bias, slabs, _, _ = _k7_case(shape)
    base = ops.conv3d_k7(x, slabs, bias)
    assert torch.equal(base, ops.conv3d_k7(x, slabs, bias))                                   # two runs are equal
    buf = torch.empty(x.numel() + 8, dtype=torch.float32, device=DEV)                         # an input one element past a 16-byte boundary
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + x.numel()].view(x.shape)
    off.copy_(x)
    assert off.data_ptr() % 16 == 4 and torch.equal(base, ops.conv3d_k7(off, slabs, bias))
    x2 = torch.cat((x, x.flip(3))).contiguous()                                               # a batch of two equals two batches of one
    both = ops.conv3d_k7(x2, slabs, bias)
    assert torch.equal(both[:1], base) and torch.equal(both[1:], ops.conv3d_k7(x2[1:].contiguous(), slabs, bias))
    assert ops.conv3d_k7(x[:0], slabs, bias).shape == (0,) + tuple(base.shape[1:])            # bs == 0 returns at once


def test_conv3d_k7_refuses_bad_arguments(ops):
    with pytest.raises(ValueError, match="7, 7"):
        ops.prep_conv3d_k7(torch.zeros((4, 4, 3, 3, 3), device=DEV))
    with pytest.raises(ValueError, match="cout <= 32"):
        ops.prep_conv3d_k7(torch.zeros((33, 4, 7, 7, 7), device=DEV))
    x, bias, slabs, _, _ = _k7_case(K7_SHAPES[0])
    with pytest.raises(ValueError, match="matching the slabs"):
        ops.conv3d_k7(torch.zeros((1, 40, 2, 5, 9), device=DEV), slabs)
    with pytest.raises(ValueError, match="matching the slabs"):
        ops.conv3d_k7(x[:, :, 0], slabs)                                                      # a 4-D input needs kd 1 slabs


def test_strided_conv3d_equals_the_dense_kernel(ops):
    """``e4s_conv3d_sb3_strided`` with dense strides, with a channel-slice destination and with a channel-slice source: the bits of ``e4s_conv3d_sb3``."""
    from e4s2024_amd._lib import lib
    from e4s2024_amd.ops import _p, _stream
    bs, cin, cout, D, H, W = 2, 24, 20, 3, 12, 20
    x, w, bias = _rand(1, bs, cin, D, H // 2, W // 2).to(DEV), _rand(2, cout, cin, 3, 3, 3, std=0.07).to(DEV), _rand(3, cout, std=0.5).to(DEV)
    slabs = ops.prep_conv3d(w)[0]
    for up in (1, 2):
        h, wd = (H // 2) * up, (W // 2) * up
        dense = ops.conv3d_sb3(x, slabs, bias, relu=True, up_hw=up)
        out = torch.empty_like(dense)
        lib().call("e4s_conv3d_sb3_strided", _p(out), _p(x), *[_p(s) for s in slabs], _p(bias), None, 1, up, bs, cin, cout, D, h, wd, x[0].numel(), out[0].numel(),
                   out[0].numel(), _stream())
        assert torch.equal(out, dense)
        wide = torch.full((bs, cout + 7, D, h, wd), -3.0, device=DEV)                         # the destination: the first channels of a wider buffer
        ops.conv3d_sb3(x, slabs, bias, relu=True, up_hw=up, out=wide[:, :cout])
        assert torch.equal(wide[:, :cout], dense) and bool((wide[:, cout:] == -3.0).all())
        back = torch.full((bs, 5 + cout, D, h, wd), -3.0, device=DEV)                         # and the last
        ops.conv3d_sb3(x, slabs, bias, relu=True, up_hw=up, out=back[:, 5:])
        assert torch.equal(back[:, 5:], dense) and bool((back[:, :5] == -3.0).all())
        src = torch.full((bs, 3 + cin, D, H // 2, W // 2), 9.0, device=DEV)                   # the source: the last channels of a wider buffer
        src[:, 3:] = x
        assert torch.equal(ops.conv3d_sb3(src[:, 3:], slabs, bias, relu=True, up_hw=up), dense)
    with pytest.raises(ValueError, match="every sample dense"):
        ops.conv3d_sb3(x, slabs, out=torch.empty((bs, cout, D, H // 2, W), device=DEV)[..., ::2])


def test_strided_avgpool_equals_the_dense_kernel(ops):
    x = _rand(4, 2, 6, 9, 14).to(DEV)
    dense = ops.avgpool2x2(x)
    assert torch.equal(ops.avgpool2x2(x, out=torch.empty_like(dense)), dense)
    wide = torch.full((2, 10, 4, 7), -3.0, device=DEV)
    ops.avgpool2x2(x, out=wide[:, 4:])
    assert torch.equal(wide[:, 4:], dense) and bool((wide[:, :4] == -3.0).all())


def _kp_dev(tag):
    return M.kp_dicts(tag, to=lambda a: T(a).to(DEV))


@pytest.mark.parametrize("tag", list(M.CASES))
def test_motion_input_and_combine_against_the_model(ops, tag):
    """The two glue kernels on the model's own float32 intermediates; ``e32`` is the float32 model of the same piece on the same inputs."""
    c = M.case(tag)
    K = M.CASES[tag][0]["num_kp"]
    f32 = T(c["out64"]["compressed"].astype(np.float32))
    args = [None if c[k] is None else T(c[k]) for k in ("kp_d", "kp_s", "jac_d", "jac_s")]
    want, sparse = M.hourglass_input(f32.double(), *[None if a is None else a.double() for a in args])
    e32 = M.max_err(M.hourglass_input(f32, *args)[0].numpy(), want.numpy())
    kd, ks = _kp_dev(tag)
    got = ops.motion_input(f32.to(DEV), kd, ks)
    err, bar = M.max_err(got.cpu().numpy(), want.numpy()), M.bound(e32, want.numpy())
    record_parity(f"v2v_motion_input.{tag}", err, bar)
    assert got.shape == want.shape and err <= bar
    cc = f32.shape[1] + 1
    assert bool((got[:, 0] == 0).all())                                                       # the background heatmap: exactly 0
    # exactly 0 where all eight taps are outside: the unnormalised coordinate ((m + 1) n - 1) / 2 below -1 or at least n, that is (|m| - 1) n > 1
    d, h, w = f32.shape[2:]
    far = ((sparse.abs() - 1) * torch.tensor([w, h, d], dtype=torch.float64) > 1.0 + 1e-3).any(-1)      # [bs, K + 1, d, h, w]
    feats = got.cpu().view(got.shape[0], K + 1, cc, d, h, w)[:, :, 1:]
    assert int(far.sum()) > 0 and bool((feats.permute(0, 1, 3, 4, 5, 2)[far] == 0).all())
    wide = torch.full((got.shape[0], got.shape[1] + 3, d, h, w), -3.0, device=DEV)            # written through a batch stride: the same bits
    ops.motion_input(f32.to(DEV), kd, ks, out=wide[:, 3:])
    assert torch.equal(wide[:, 3:], got) and bool((wide[:, :3] == -3.0).all())

    lg = T(c["out64"]["logits"].astype(np.float32))
    sp32 = M.hourglass_input(f32, *args)[1]
    m64, d64 = M.combine(lg.double(), sparse)
    m32, d32 = M.combine(lg, sp32)
    mask, deformation = ops.motion_combine(lg.to(DEV), kd, ks)
    for name, g, w64, w32 in (("mask", mask, m64, m32), ("deformation", deformation, d64, d32)):
        err, bar = M.max_err(g.cpu().numpy(), w64.numpy()), M.bound(M.max_err(w32.numpy(), w64.numpy()), w64.numpy())
        record_parity(f"v2v_motion_combine.{tag}.{name}", err, bar)
        assert g.shape == w64.shape and err <= bar, name
    again = ops.motion_combine(lg.to(DEV), kd, ks)
    assert torch.equal(again[0], mask) and torch.equal(again[1], deformation)


_NETS = {}


def _net(tag):
    if tag not in _NETS:
        net = M.make_module(tag)
        net.load_state_dict(M.case(tag)["sd"], strict=True)
        _NETS[tag] = net.to(DEV)
    return _NETS[tag]


@pytest.mark.parametrize("tag", list(M.CASES))
def test_dense_motion_forward_against_the_model_and_the_reference(ops, golden, tag):
    c = M.case(tag)
    kd, ks = _kp_dev(tag)
    before = [{k: v.clone() for k, v in kp.items()} for kp in (kd, ks)]
    x = T(c["feature"]).to(DEV)
    out = ops.dense_motion_forward(x, kd, ks, _net(tag))
    assert list(out) == [k for k in M.OUTPUTS if k in c["out64"]]
    for k, got in out.items():
        bar = M.bound(c["e32"][k], c["out64"][k])
        err, ref_err = M.max_err(got.cpu().numpy(), c["out64"][k]), M.max_err(got.cpu().numpy(), golden[f"{tag}.{k}"])
        record_parity(f"dense_motion_forward.{tag}.{k}", err, bar)
        record_parity(f"dense_motion_forward.{tag}.{k}.against_the_reference", ref_err, 2 * bar)
        assert got.shape == c["out64"][k].shape and got.dtype == torch.float32 and err <= bar, k
        assert ref_err <= 2 * bar, k                                                           # (two float32 results, each within one bar of float64)
    assert all(torch.equal(v, was[k]) for kp, was in zip((kd, ks), before) for k, v in kp.items())      # the caller's dicts are as they were
    again = ops.dense_motion_forward(x, kd, ks, _net(tag))
    assert all(torch.equal(again[k], out[k]) for k in out)                                    # a second call equals the first
    # a mapping, the generator's checkpoint and the file torch.load returns: the same bits
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    gen = {"dense_motion_network." + k: v for k, v in sd.items()}
    gen["first.conv.weight"] = torch.zeros(1, device=DEV)
    for weights in (sd, gen, {"generator": gen, "kp_detector": {}}):
        got = ops.dense_motion_forward(x, kd, ks, weights)
        assert all(torch.equal(got[k], out[k]) for k in out)


def test_batch_equals_singles_and_a_strided_feature_is_accepted(ops):
    c = M.case("D-A")
    kd, ks = _kp_dev("D-A")
    x = T(c["feature"]).to(DEV)
    both = ops.dense_motion_forward(x, kd, ks, _net("D-A"))
    for i in range(2):
        one = ops.dense_motion_forward(x[i:i + 1], {"value": kd["value"][i:i + 1]}, {"value": ks["value"][i:i + 1]}, _net("D-A"))
        assert all(torch.equal(one[k], both[k][i:i + 1]) for k in both)
    strided = x.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)                   # channels last in memory
    assert not strided.is_contiguous()
    got = ops.dense_motion_forward(strided, kd, ks, _net("D-A"))
    assert all(torch.equal(got[k], both[k]) for k in both)
    empty = ops.dense_motion_forward(x[:0], {"value": kd["value"][:0]}, {"value": ks["value"][:0]}, _net("D-A"))
    assert empty["mask"].shape == (0, 6, 4, 16, 16) and empty["deformation"].shape == (0, 4, 16, 16, 3) and empty["occlusion_map"].shape == (0, 1, 16, 16)


def test_graph_replay_gives_the_eager_bits(ops):
    from e4s2024_amd import pipeline
    c = M.case("D-B")
    kd, ks = _kp_dev("D-B")
    x = T(c["feature"]).to(DEV)
    eager = pipeline.reenact_dense_motion(_net("D-B"), x, kd, ks)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.dense_motion_forward(x, kd, ks, _net("D-B"))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.dense_motion_forward(x, kd, ks, _net("D-B"))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in eager)


def test_dropin_forward_runs_the_native_path(ops):
    from conftest import install_dropin
    install_dropin()
    from swap_face_fine.face_vid2vid.modules import dense_motion as dm
    c = M.case("D-D")
    net = dm.DenseMotionNetwork(**M.config("D-D")).eval()
    net.load_state_dict(c["sd"], strict=True)
    kd, ks = _kp_dev("D-D")
    x = T(c["feature"]).to(DEV)
    out, want = net.to(DEV)(x, kd, ks), ops.dense_motion_forward(x, kd, ks, _net("D-D"))
    assert list(out) == list(want) and all(torch.equal(out[k], want[k]) for k in want)
