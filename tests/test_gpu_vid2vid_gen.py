"""Row f19 on the GPU: the three glue kernels alone against float64 and their bit-for-bit properties, then ``appearance_feature``, ``generator_warp`` and
``generator_front_forward`` against the float64 model ``vid2vid_gen_model`` under its bars (``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against
itself in float64; test_vid2vid_gen_cpu.py pins those bars from the other side with mutants and holds the reference's stored outputs to them) and against the
reference's stored outputs.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vid2vid_gen_model as M
from conftest import load_golden, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
DEFORM_SHAPES = [(2, 5, 3, 8, 24), (1, 8, 4, 16, 16), (1, 3, 2, 2, 6)]        # more than one workgroup per channel row, 5 and 3 channels (ragged rows of 4), W = 6
FRONT_TAGS = ["G-A", "G-B", "G-C", "G-D"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("g30_vid2vid_gen")


@pytest.fixture(scope="module")
def ops():
    from e4s2024_amd import ops
    return ops


def _rand(seed, *shape, std=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * np.float32(std))


def _offset(t):
    """A dense copy of the device tensor ``t`` that starts one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + t.numel()].view(t.shape)
    off.copy_(t)
    return off


_DEFORM = {}


def _deform_case(shape):
    """(feature, deformation) on the CPU and the float64 ``F.grid_sample`` of them, made once: about a third of the sample points outside the volume and, in
    the first rows of the last depth slice, a block wholly outside (every tap beyond the border)."""
    if shape not in _DEFORM:
        bs, C, D, H, W = shape
        x = _rand(sum(shape), *shape)
        grid = T(np.random.RandomState(sum(shape) + 1).uniform(-1.15, 1.15, (bs, D, H, W, 3)).astype(np.float32))
        grid[:, -1, :max(H // 4, 1)] = torch.tensor([3.0, -2.5, 1.75])
        grid[:, 0, 0, 0] = torch.tensor([-1.0, 1.0, -1.0])                                    # a corner, and the exact centre
        grid[:, 0, 0, 1] = 0.0
        want = F.grid_sample(x.double(), grid.double(), mode="bilinear", padding_mode="zeros", align_corners=False).reshape(bs, C * D, H, W)
        _DEFORM[shape] = (x, grid, want)
    return _DEFORM[shape]


@pytest.mark.parametrize("shape", DEFORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_deform_feature_against_float64(ops, shape):
    x, grid, want = _deform_case(shape)
    outside = float((grid.abs() > 1).any(-1).float().mean())
    assert 0.2 <= outside <= 0.7, outside
    got = ops.deform_feature(x.to(DEV), grid.to(DEV))
    assert got.shape == want.shape and got.dtype == torch.float32
    # the coordinate ((g + 1) S - 1) / 2 takes two float32 roundings at a magnitude of at most 2.15 S, halved: 1.1 eps S (held to 1.25) per axis, and the trilinear sum moves by
    # at most 2 max|x| per unit of a coordinate; the weights, products and the sum of eight taps add a dozen roundings of values below max|x|
    bs, C, D, H, W = shape
    err, bar = M.max_err(got.cpu().numpy(), want.numpy()), (2.5 * (D + H + W) + 12) * EPS32 * float(x.abs().max())
    record_parity(f"v2v_deform.{'x'.join(map(str, shape))}", err, bar)
    assert err <= bar
    dead = got.view(bs, C, D, H, W)[:, :, -1, :max(H // 4, 1)]                                # all eight taps outside: exactly zero
    assert bool((dead == 0).all()) and bool((want.view(bs, C, D, H, W)[:, :, -1, :max(H // 4, 1)] == 0).all())


@pytest.mark.parametrize("shape", DEFORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_deform_feature_bit_for_bit_properties(ops, shape):
    x, grid, _ = _deform_case(shape)
    x, grid = x.to(DEV), grid.to(DEV)
    bs, C, D, H, W = shape
    base = ops.deform_feature(x, grid)
    assert torch.equal(base, ops.deform_feature(x, grid))                                     # two runs are equal
    for i in range(bs):                                                                       # a batch equals its samples
        assert torch.equal(ops.deform_feature(x[i:i + 1], grid[i:i + 1]), base[i:i + 1])
    buf = torch.empty(base.numel() + 8, dtype=torch.float32, device=DEV)                      # an output one element past a 16-byte boundary: the same bits
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + base.numel()].view(base.shape)
    ops.deform_feature(x, grid, out=off)
    assert off.data_ptr() % 16 == 4 and torch.equal(off, base)
    gbuf = torch.empty(grid.numel() + 8, dtype=torch.float32, device=DEV)                     # and a deformation there
    goff = gbuf[1:1 + grid.numel()].view(grid.shape)
    goff.copy_(grid)
    assert goff.data_ptr() % 16 == 4 and torch.equal(ops.deform_feature(x, goff), base)
    xoff = _offset(x)                                                                         # and a feature
    assert xoff.data_ptr() % 16 == 4 and torch.equal(ops.deform_feature(xoff, grid), base)
    n = 3                                                                                     # one feature for n deformations: batch 1, and expand(n)
    grids = torch.cat([grid[:1], grid[:1].flip(1), grid[:1].flip(2)])
    shared = ops.deform_feature(x[:1], grids)
    assert torch.equal(shared, ops.deform_feature(x[:1].expand(n, -1, -1, -1, -1), grids))
    assert torch.equal(shared, ops.deform_feature(x[:1].repeat(n, 1, 1, 1, 1), grids)) and torch.equal(shared[:1], base[:1])
    wide = torch.full((bs, C * D + 5, H, W), -3.0, device=DEV)                                # out= into a channel slice of a wider buffer
    ops.deform_feature(x, grid, out=wide[:, 2:2 + C * D])
    assert torch.equal(wide[:, 2:2 + C * D], base) and bool((wide[:, :2] == -3.0).all()) and bool((wide[:, 2 + C * D:] == -3.0).all())
    assert ops.deform_feature(x[:0], grid[:0]).shape == (0, C * D, H, W)                      # bs == 0 returns at once


def test_bn_relu_and_occlude_against_float64(ops):
    for shape in [(2, 5, 3, 5, 7), (1, 8, 4, 8, 8)]:                                          # n = 105: n % 4 != 0, the one-element form; n = 256
        x, scale, shift = _rand(1, *shape), _rand(2, shape[1]), _rand(3, shape[1], std=0.5)
        scale[1] = 0.0
        view = (1, -1, 1, 1, 1)
        want = F.relu(x.double() * scale.double().view(view) + shift.double().view(view))
        got = ops.bn_relu(x.to(DEV), scale.to(DEV), shift.to(DEV))
        err, bar = M.max_err(got.cpu().numpy(), want.numpy()), EPS32 * float(want.abs().max())     # one rounding: the fused multiply-add
        record_parity(f"v2v_bn_relu.{'x'.join(map(str, shape))}", err, bar)
        assert got.shape == x.shape and err <= bar and float(got.min()) == 0.0
        assert 0.2 <= float((got == 0).float().mean()) <= 0.8
        xd = x.to(DEV)
        # a pointer one element past alignment takes the one-element form whatever n is: the same bits, for x, for out and for both
        assert torch.equal(ops.bn_relu(_offset(xd), scale.to(DEV), shift.to(DEV)), got)
        assert torch.equal(ops.bn_relu(xd, scale.to(DEV), shift.to(DEV), out=_offset(xd)), got)
        xo = _offset(xd)
        assert ops.bn_relu(xo, scale.to(DEV), shift.to(DEV), out=xo) is xo and torch.equal(xo, got)
        assert ops.bn_relu(xd, scale.to(DEV), shift.to(DEV), out=xd) is xd and torch.equal(xd, got)                  # in place
    for shape in [(2, 5, 5, 7), (1, 20, 8, 24)]:                                              # hw = 35 and 192
        x, occ = _rand(4, *shape), torch.sigmoid(_rand(5, shape[0], 1, *shape[2:], std=2.0))
        want = x.double() * occ.double()
        got = ops.occlude(x.to(DEV), occ.to(DEV))
        err, bar = M.max_err(got.cpu().numpy(), want.numpy()), EPS32 * float(want.abs().max())
        record_parity(f"v2v_occlude.{'x'.join(map(str, shape))}", err, bar)
        assert got.shape == x.shape and err <= bar
        xd, od = x.to(DEV), occ.to(DEV)
        assert torch.equal(ops.occlude(_offset(xd), od), got) and torch.equal(ops.occlude(xd, _offset(od)), got)      # x, then the map alone, past alignment
        assert torch.equal(ops.occlude(xd, od, out=_offset(xd)), got)
        assert ops.occlude(xd, occ.to(DEV), out=xd) is xd and torch.equal(xd, got)            # in place: the same bits
    assert ops.occlude(torch.zeros(0, 4, 3, 3, device=DEV), torch.zeros(0, 1, 3, 3, device=DEV)).shape == (0, 4, 3, 3)


_NETS = {}


def _net(tag):
    if tag not in _NETS:
        net = M.make_module(tag)
        net.load_state_dict(M.case(tag)["sd"], strict=True)
        _NETS[tag] = net.to(DEV)
    return _NETS[tag]


def _kp_dev(tag, rows=slice(None)):
    return M.kp_dicts(tag, to=lambda a: T(a).to(DEV), rows=rows)


def _held(name, tag, out, golden):
    """Every output within the model's bar, and within twice the bar of what the fixture holds of the reference."""
    c = M.case(tag)
    for k, got in out.items():
        bar = M.bound(c["e32"][k], c["out64"][k])
        err = M.max_err(got.cpu().numpy(), c["out64"][k])
        record_parity(f"{name}.{tag}.{k}", err, bar)
        assert got.shape == c["out64"][k].shape and got.dtype == torch.float32 and err <= bar, k
        if f"{tag}.{k}" in golden.files:
            ref_err = M.max_err(got.cpu().numpy(), golden[f"{tag}.{k}"])
            record_parity(f"{name}.{tag}.{k}.against_the_reference", ref_err, 2 * bar)
            assert ref_err <= 2 * bar, k                                                       # (two float32 results, each within one bar of float64)


@pytest.mark.parametrize("tag", FRONT_TAGS)
def test_front_against_the_model_and_the_reference(ops, golden, tag):
    from e4s2024_amd import pipeline
    c = M.case(tag)
    net = _net(tag)
    kd, ks = _kp_dev(tag)
    before = [{k: v.clone() for k, v in kp.items()} for kp in (kd, ks)]
    x = T(c["source"]).to(DEV)
    f3 = ops.appearance_feature(x, net)
    _held("appearance_feature", tag, {"feature_3d": f3}, golden)
    out = ops.generator_warp(f3, kd, ks, net)
    assert list(out) == [k for k in ("mask", "deformation", "occlusion_map", "feature") if k in c["out64"]]
    _held("generator_warp", tag, out, golden)
    whole = ops.generator_front_forward(x, kd, ks, net)                                       # the two in a row: the cached feature path gives the same bits
    assert list(whole) == list(out) and all(torch.equal(whole[k], out[k]) for k in out)
    assert all(torch.equal(v, was[k]) for kp, was in zip((kd, ks), before) for k, v in kp.items())      # the caller's dicts are as they were
    again = pipeline.reenact_warp(net, pipeline.reenact_source_feature(net, x), kd, ks)
    assert all(torch.equal(again[k], out[k]) for k in out)                                    # a second call equals the first
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}                                           # a mapping without decoder keys, and the checkpoint file
    for weights in (sd, {"generator": sd, "kp_detector": {}}, {"generator." + k: v for k, v in sd.items()}, {"module." + k: v for k, v in sd.items()}):
        got = ops.generator_front_forward(x, kd, ks, weights)
        assert all(torch.equal(got[k], out[k]) for k in out)
    strided = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                          # a non-contiguous image is accepted
    assert not strided.is_contiguous() and torch.equal(ops.appearance_feature(strided, net), f3)


def test_shared_feature_equals_single_calls(ops):
    """G-D: one source feature against three driving keypoint sets, bit-equal to three calls with one set each."""
    net = _net("G-D")
    x = T(M.case("G-D")["source"]).to(DEV)
    f3 = ops.appearance_feature(x, net)
    kd, ks = _kp_dev("G-D")
    both = ops.generator_warp(f3, kd, ks, net)
    assert both["feature"].shape[0] == 3
    for i in range(3):
        kdi, ksi = _kp_dev("G-D", slice(i, i + 1))
        one = ops.generator_warp(f3, kdi, ksi, net)
        assert all(torch.equal(one[k], both[k][i:i + 1]) for k in both), i
    rep = ops.generator_warp(f3.repeat(3, 1, 1, 1, 1), kd, ks, net)                           # and to a feature per frame
    assert all(torch.equal(rep[k], both[k]) for k in both)
    empty = ops.generator_warp(f3, {"value": kd["value"][:0]}, {"value": ks["value"][:0]}, net)
    assert empty["feature"].shape == (0, 32, 8, 8) and empty["mask"].shape == (0, 6, 4, 8, 8) and empty["occlusion_map"].shape == (0, 1, 8, 8)
    assert ops.appearance_feature(x[:0], net).shape == (0, 8, 4, 8, 8)


def test_graph_replay_gives_the_eager_bits(ops):
    net = _net("G-B")
    x = T(M.case("G-B")["source"]).to(DEV)
    kd, ks = _kp_dev("G-B")
    eager = ops.generator_front_forward(x, kd, ks, net)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.generator_front_forward(x, kd, ks, net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.generator_front_forward(x, kd, ks, net)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in eager)


def test_mirror_on_the_device_agrees_with_the_native_front(ops):
    """The stock-PyTorch mirror, the parent path of the timings, on the same device and weights: within two bars of the native front."""
    tag = "G-A"
    c = M.case(tag)
    net = _net(tag)
    x = T(c["source"]).to(DEV)
    kd, ks = _kp_dev(tag)
    stock, native = net.front(x, kd, ks), ops.generator_front_forward(x, kd, ks, net)
    for k in native:
        err, bar = M.max_err(stock[k].cpu().numpy(), native[k].cpu().numpy()), 2 * M.bound(c["e32"][k], c["out64"][k])
        record_parity(f"generator_front_forward.{tag}.{k}.against_stock_pytorch", err, bar)
        assert err <= bar, k
