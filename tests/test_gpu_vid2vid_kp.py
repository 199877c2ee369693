"""Row f17 on the GPU: the 3 x 3 x 3 convolution and the glue kernels alone against float64, then ``kp_detector_forward``, ``he_estimator_forward``,
``keypoint_transformation`` and ``reenact_keypoints`` against the float64 model ``vid2vid_kp_model`` under its bars (``max(8 e32, 2e-7 max|want|)``, ``e32`` the
model in float32 against itself in float64; test_vid2vid_kp_cpu.py pins those bars from the other side with mutants and holds the reference's stored outputs to
them).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vid2vid_kp_model as M
from conftest import load_golden, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_RTOL = 2e-6                             # the project's bar for the three-way bf16 split (tests/test_gpu_conv_variants.py)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731

# (bs, cin, cout, D, H, W, up_hw): D, H, W are the output extents
CONV3D_SHAPES = [(1, 5, 3, 2, 3, 5, 1), (2, 24, 15, 3, 6, 10, 2), (1, 32, 45, 4, 16, 16, 2), (1, 16, 135, 2, 33, 17, 1), (2, 64, 32, 16, 8, 8, 2),
                 (1, 48, 16, 5, 1, 7, 1)]
KA_SHAPE = CONV3D_SHAPES[2]                  # UpBlock3d 'up0' of case K-A: 32 channels onto the (4, 16, 16) volume


@pytest.fixture(scope="module")
def golden():
    return load_golden("g28_vid2vid_kp")


@pytest.fixture(scope="module")
def ops():
    from e4s2024_amd import ops
    return ops


def _rand(seed, *shape, std=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * np.float32(std))


_CONV3D = {}


def _conv3d_case(shape):
    """(x, w, bias, residual, slabs) on the device and the float64 references {(with bias + ReLU, with residual): out} of one shape, made once."""
    if shape not in _CONV3D:
        from e4s2024_amd import ops
        bs, cin, cout, D, H, W, up = shape
        seed = sum(shape)
        x, w = _rand(seed, bs, cin, D, H // up, W // up), _rand(seed + 1, cout, cin, 3, 3, 3, std=1.0 / np.sqrt(27 * cin))
        bias, res = _rand(seed + 2, cout, std=0.5), _rand(seed + 3, bs, cout, D, H, W)
        xu = F.interpolate(x.double(), scale_factor=(1, up, up)) if up == 2 else x.double()      # nearest, on the host
        plain = F.conv3d(xu, w.double(), None, padding=1)
        ref = {(False, False): plain, (True, False): F.relu(plain + bias.double().view(1, -1, 1, 1, 1)),
               (True, True): F.relu(plain + bias.double().view(1, -1, 1, 1, 1) + res.double())}
        slabs = ops.prep_conv3d(w.to(DEV))[0]
        _CONV3D[shape] = (x.to(DEV), w, bias.to(DEV), res.to(DEV), slabs, ref)
    return _CONV3D[shape]


def _run3d(ops, shape, act, with_res, x=None):
    xd, _, bias, res, slabs, _ = _conv3d_case(shape)
    return ops.conv3d_sb3(xd if x is None else x, slabs, bias if act else None, relu=act, residual=res if with_res else None, up_hw=shape[6])


@pytest.mark.parametrize("act", [False, True], ids=["plain", "bias_relu"])
@pytest.mark.parametrize("shape", CONV3D_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3d_against_float64(ops, shape, act):
    ref = _conv3d_case(shape)[5][(act, False)]
    got = _run3d(ops, shape, act, False)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err, bar = M.max_err(got.cpu().numpy(), ref.numpy()), FP32_RTOL * float(ref.abs().max())
    record_parity(f"conv3d_sb3.{'x'.join(map(str, shape))}.{'act' if act else 'plain'}", err, bar)
    assert err <= bar


def test_conv3d_with_a_residual_against_float64(ops):
    ref = _conv3d_case(KA_SHAPE)[5][(True, True)]
    got = _run3d(ops, KA_SHAPE, True, True)
    err, bar = M.max_err(got.cpu().numpy(), ref.numpy()), FP32_RTOL * float(ref.abs().max())
    record_parity("conv3d_sb3.K-A.residual", err, bar)
    assert err <= bar
    assert not torch.equal(got, _run3d(ops, KA_SHAPE, True, False))                           # the residual is read


@pytest.mark.parametrize("shape", [CONV3D_SHAPES[1], CONV3D_SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_conv3d_bit_for_bit_properties(ops, shape):
    bs, cin, cout, D, H, W, up = shape
    xd, _, bias, res, slabs, _ = _conv3d_case(shape)
    base = _run3d(ops, shape, True, True)
    assert torch.equal(base, _run3d(ops, shape, True, True))                                  # two runs are equal
    # an input that starts one element past a 16-byte boundary
    buf = torch.empty(xd.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    off = buf[1:1 + xd.numel()].view(xd.shape)
    off.copy_(xd)
    assert off.data_ptr() % 16 == 4 and torch.equal(base, _run3d(ops, shape, True, True, x=off))
    # up_hw = 2 equals up_hw = 1 on the host-upsampled input
    if up == 2:
        xu = F.interpolate(xd, scale_factor=(1, 2, 2)).contiguous()
        assert torch.equal(base, ops.conv3d_sb3(xu, slabs, bias, relu=True, residual=res, up_hw=1))
    # a batch of two equals two batches of one
    x2 = torch.cat((xd, xd.flip(2)))[:2].contiguous()
    r2 = torch.cat((res, res.flip(3)))[:2].contiguous()
    both = ops.conv3d_sb3(x2, slabs, bias, relu=True, residual=r2, up_hw=up)
    for i in range(2):
        assert torch.equal(both[i:i + 1], ops.conv3d_sb3(x2[i:i + 1].contiguous(), slabs, bias, relu=True, residual=r2[i:i + 1].contiguous(), up_hw=up))


def test_conv3d_refuses_bad_arguments(ops):
    xd, _, _, _, slabs, _ = _conv3d_case(CONV3D_SHAPES[0])
    with pytest.raises(ValueError, match="up_hw"):
        ops.conv3d_sb3(xd, slabs, up_hw=3)
    with pytest.raises(ValueError, match="matching the slabs"):
        ops.conv3d_sb3(torch.zeros((1, 17, 2, 3, 5), device=DEV), slabs)
    with pytest.raises(ValueError, match="residual"):
        ops.conv3d_sb3(xd, slabs, residual=torch.zeros((1, 3, 2, 3, 4), device=DEV))
    with pytest.raises(ValueError, match="3, 3, 3"):
        ops.prep_conv3d(torch.zeros((4, 4, 3, 3), device=DEV))


@pytest.mark.parametrize("hw", [(52, 36), (64, 64), (13, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_antialias_down_against_float64(ops, hw):
    """The bar is derived as the stem's: 169 fused multiply-adds, each rounded once: 170 * 2^-24 * max sum |w x|."""
    h, w = hw
    x = T(M.to_float(M.images_u8(h + w, 2, h, w)))
    k = ops.antialias_kernel(0.25)
    pad = F.pad(x.double(), (6,) * 4)
    ref = F.conv2d(pad, k.double().view(1, 1, 13, 13).repeat(3, 1, 1, 1), groups=3)[:, :, ::4, ::4]
    mag = F.conv2d(pad.abs(), k.double().view(1, 1, 13, 13).repeat(3, 1, 1, 1), groups=3)[:, :, ::4, ::4]
    got = ops.antialias_down(x.to(DEV), k.to(DEV), 4)
    assert got.shape == ref.shape == (2, 3, -(-h // 4), -(-w // 4))
    err, bar = M.max_err(got.cpu().numpy(), ref.numpy()), 170 * 2.0 ** -24 * float(mag.max())
    record_parity(f"v2v_antialias_down.{h}x{w}", err, bar)
    assert err <= bar
    assert torch.equal(got, ops.antialias_down(x.to(DEV), k.to(DEV), 4))
    if hw == (13, 13):                                                                        # a single row and column of outputs beside the first: taps in the pad
        assert float(mag[:, :, 0, 0].min()) < 0.5 * float(mag.max())


@pytest.mark.parametrize("hw", [(7, 5), (9, 13), (2, 3), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_avgpool2x2_against_float64(ops, hw):
    x = _rand(sum(hw), 3, 5, *hw)
    ref = F.avg_pool2d(x.double(), 2)
    got = ops.avgpool2x2(x.to(DEV))
    assert got.shape == ref.shape == (3, 5, hw[0] // 2, hw[1] // 2)
    err, bar = M.max_err(got.cpu().numpy(), ref.numpy()), 4 * 2.0 ** -24 * float(x.abs().max())
    record_parity(f"avgpool2x2.{hw[0]}x{hw[1]}", err, bar)
    assert err <= bar
    with pytest.raises(ValueError, match="2 x 2"):
        ops.avgpool2x2(torch.zeros((1, 1, 1, 4), device=DEV))


def _heatmap_check(ops, name, logits, planes):
    """``e4s_v2v_heatmap_kp`` on given logits against the float64 expression; ``e32`` is stock float32 torch on the same logits against float64."""
    h64, v64, j64 = M.heatmap_expectation(logits.double(), None if planes is None else planes.double(), 0.1)
    h32, v32, j32 = M.heatmap_expectation(logits, planes, 0.1)
    value, jac, heat = ops.heatmap_keypoints(logits.to(DEV), None if planes is None else planes.to(DEV), 0.1, want_heatmap=True)
    for k, got, want, f32 in (("value", value, v64, v32), ("jacobian", jac, j64, j32), ("heatmap", heat, h64, h32)):
        if want is None:
            assert got is None
            continue
        err, bar = M.max_err(got.cpu().numpy(), want.numpy()), M.bound(M.max_err(f32.numpy(), want.numpy()), want.numpy())
        record_parity(f"v2v_heatmap_kp.{name}.{k}", err, bar)
        assert got.shape == want.shape and err <= bar, k
    v2, j2, _ = ops.heatmap_keypoints(logits.to(DEV), None if planes is None else planes.to(DEV), 0.1)
    assert torch.equal(v2, value) and (jac is None or torch.equal(j2, jac))                   # two runs give the same bits, with or without the heatmap
    return value


def test_heatmap_kp_on_the_stored_logits(ops, golden):
    logits = T(golden["K-A.prediction"])
    planes = _rand(3, 2, 45, 4, 16, 16)
    value = _heatmap_check(ops, "K-A", logits, planes)
    _heatmap_check(ops, "K-A.no_jacobian", logits, None)
    # against the reference's own keypoints, from its own logits: the model's bar of that case
    c = M.case("K-A")
    err, bar = M.max_err(value.cpu().numpy(), golden["K-A.value"]), M.bound(c["e32"]["value"], c["out64"]["value"])
    record_parity("v2v_heatmap_kp.K-A.against_the_reference", err, 2 * bar)
    assert err <= 2 * bar                                                                      # (two float32 results, each within one bar of float64)


def test_heatmap_kp_with_one_dominant_position(ops):
    logits = _rand(11, 1, 3, 3, 5, 7, std=0.05)
    for k, (z, y, x) in enumerate(((0, 0, 0), (2, 4, 6), (1, 3, 2))):
        logits[0, k, z, y, x] = 5.0                                                            # 50 after the division: every other position is below e^-45
    value = _heatmap_check(ops, "dominant", logits, _rand(12, 1, 27, 3, 5, 7))
    want = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [2 * 2 / 6 - 1, 2 * 3 / 4 - 1, 0.0]])
    assert float((value[0].cpu() - want).abs().max()) < 1e-6
    with pytest.raises(ValueError, match="at least 2"):
        ops.heatmap_keypoints(torch.zeros((1, 1, 1, 4, 4), device=DEV))


_NETS = {}


def _net(tag):
    if tag not in _NETS:
        net = M.make_module(tag)
        net.load_state_dict(M.case(tag)["sd"], strict=True)
        _NETS[tag] = net.to(DEV)
    return _NETS[tag]


@pytest.mark.parametrize("tag", list(M.KP_CASES))
def test_kp_detector_forward_against_the_model(ops, tag):
    c = M.case(tag)
    out = ops.kp_detector_forward(T(c["x"]).to(DEV), _net(tag), want_heatmap=True)
    assert set(out) == {k for k in M.KP_OUTPUTS + ("prediction", "heatmap") if c["out64"][k] is not None}
    for k, got in out.items():
        err, bar = M.max_err(got.cpu().numpy(), c["out64"][k]), M.bound(c["e32"][k], c["out64"][k])
        record_parity(f"kp_detector_forward.{tag}.{k}", err, bar)
        assert got.shape == c["out64"][k].shape and err <= bar, k
    again = ops.kp_detector_forward(T(c["x"]).to(DEV), _net(tag))
    assert set(again) == {k for k in M.KP_OUTPUTS if c["out64"][k] is not None} and all(torch.equal(again[k], out[k]) for k in again)
    # the mapping torch.load returns, bare and as the whole checkpoint: the same bits
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    for weights in (sd, {"kp_detector": sd, "he_estimator": {}}):
        got = ops.kp_detector_forward(T(c["x"]).to(DEV), weights, temperature=0.1)
        assert all(torch.equal(got[k], out[k]) for k in got)


@pytest.mark.parametrize("tag", list(M.HE_CASES))
def test_he_estimator_forward_against_the_model(ops, tag):
    c = M.case(tag)
    out = ops.he_estimator_forward(T(c["x"]).to(DEV), _net(tag))
    assert list(out) == list(M.HE_OUTPUTS)
    for k, got in out.items():
        err, bar = M.max_err(got.cpu().numpy(), c["out64"][k]), M.bound(c["e32"][k], c["out64"][k])
        record_parity(f"he_estimator_forward.{tag}.{k}", err, bar)
        assert got.shape == c["out64"][k].shape and err <= bar, k
    again = ops.he_estimator_forward(T(c["x"]).to(DEV), _net(tag))
    assert all(torch.equal(again[k], out[k]) for k in out)


def _t_inputs(golden, tag):
    """The transformation's inputs of a T case: the reference's stored head outputs and keypoints (the hand-made rows for T-hand), and the model on them."""
    c = M.case(tag)
    he_tag, kp_tag, _ = M.T_CASES[tag]
    n = c["kp"].shape[0]
    he = c["he"] if he_tag == "hand" else {k: golden[f"{he_tag}.{k}"] for k in M.HE_OUTPUTS}
    kp = golden[f"{kp_tag}.value"][:n]
    jac = None if c["jac"] is None else golden[f"{kp_tag}.jacobian"][:n]
    return he, kp, jac, c["fixed"], M.transform_outputs(c, he=he, kp=kp, jac=jac)


@pytest.mark.parametrize("tag", list(M.T_CASES))
def test_keypoint_transformation_against_the_model(ops, golden, tag):
    he, kp, jac, fixed, want = _t_inputs(golden, tag)
    he_d = {k: T(v).to(DEV) for k, v in he.items()}
    kp_d = {"value": T(kp).to(DEV)}
    if jac is not None:
        kp_d["jacobian"] = T(jac).to(DEV)
    kw = {} if fixed is None else dict(free_view=True, yaw=fixed[0], pitch=fixed[1], roll=fixed[2])
    out = ops.keypoint_transformation(kp_d, he_d, estimate_jacobian=jac is not None, **kw)
    assert set(out) == {"value", "jacobian"} and (out["jacobian"] is None) == (jac is None)
    got = dict(out)
    if fixed is None:
        got["deg"], got["rot"] = ops.headpose_degrees(he_d), ops.rotation_matrix(he_d)
    for k in M.T_OUTPUTS:
        if want["out64"][k] is None or k not in got:
            continue
        err, bar = M.max_err(got[k].cpu().numpy(), want["out64"][k]), M.bound(want["e32"][k], want["out64"][k])
        record_parity(f"keypoint_transformation.{tag}.{k}", err, bar)
        assert got[k].shape == want["out64"][k].shape and err <= bar, k
    assert he_d["t"].shape == (he["t"].shape[0], 3)                                           # the caller's he['t'] is left as it was
    three_d = dict(he_d, t=he_d["t"].unsqueeze(1))                                            # what the reference leaves behind is accepted
    assert torch.equal(ops.keypoint_transformation(kp_d, three_d, estimate_jacobian=jac is not None, **kw)["value"], out["value"])


def test_reenact_keypoints_runs_one_head_pose_pass(ops):
    """``reenact_keypoints`` against the float64 model, and bit for bit against the calls made one by one."""
    from e4s2024_amd import pipeline
    kp_net, he_net = _net("K-A"), _net("H-B")                                                 # five keypoints both
    frames = T(M.to_float(M.images_u8(5, 4, 64, 64))).to(DEV)
    source, driving = frames[:1].contiguous(), frames[1:].contiguous()
    calls = []
    orig = ops.he_estimator_forward
    import e4s2024_amd.ops_reenact as R
    R.he_estimator_forward = lambda x, w: (calls.append(tuple(x.shape)), orig(x, w))[1]
    try:
        kp_c, kp_s, kp_d = pipeline.reenact_keypoints(kp_net, he_net, source, driving)
    finally:
        R.he_estimator_forward = orig
    assert calls == [(4, 3, 64, 64)]                                                          # ONE pass over the n + 1 images
    assert kp_d["value"].shape == (3, 5, 3) and kp_d["jacobian"].shape == (3, 5, 3, 3) and kp_s["value"].shape == (1, 5, 3)
    x = frames.cpu().numpy()
    c64 = M.kp_network(M.case("K-A")["sd"], x[:1], M.kp_config("K-A"))
    c32 = M.kp_network(M.case("K-A")["sd"], x[:1], M.kp_config("K-A"), dtype=torch.float32)
    he64, he32 = M.he_network(M.case("H-B")["sd"], x), M.he_network(M.case("H-B")["sd"], x, dtype=torch.float32)
    part = lambda he, a, b: {k: v[a:b] for k, v in he.items()}      # noqa: E731
    for name, got, a, b in (("source", kp_s, 0, 1), ("driving", kp_d, 1, 4)):
        w64 = M.transform(c64["value"], c64["jacobian"], part(he64, a, b))
        w32 = M.transform(c32["value"], c32["jacobian"], part(he32, a, b), dtype=torch.float32)
        for k in ("value", "jacobian"):
            err, bar = M.max_err(got[k].cpu().numpy(), w64[k].numpy()), M.bound(M.max_err(w32[k].numpy(), w64[k].numpy()), w64[k].numpy())
            record_parity(f"reenact_keypoints.{name}.{k}", err, bar)
            assert err <= bar, (name, k)
    one = ops.keypoint_transformation(ops.kp_detector_forward(source, kp_net), ops.he_estimator_forward(driving[1:2].contiguous(), he_net))
    assert torch.equal(one["value"], kp_d["value"][1:2]) and torch.equal(one["jacobian"], kp_d["jacobian"][1:2])
    assert torch.equal(kp_c["value"], ops.kp_detector_forward(source, kp_net)["value"])


def test_dropin_forwards_run_the_native_path(ops):
    from conftest import install_dropin
    install_dropin()
    from swap_face_fine.face_vid2vid.modules import keypoint_detector as kd
    cfg, c = M.kp_config("K-C"), M.case("K-C")
    net = kd.KPDetector(cfg["block_expansion"], 32, cfg["num_kp"], 3, cfg["max_features"], cfg["reshape_channel"], cfg["reshape_depth"], cfg["num_blocks"], 0.1,
                        estimate_jacobian=True, scale_factor=0.25).eval()
    net.load_state_dict(c["sd"], strict=True)
    x = T(c["x"]).to(DEV)
    out, want = net.to(DEV)(x), ops.kp_detector_forward(x, _net("K-C"))
    assert torch.equal(out["value"], want["value"]) and torch.equal(out["jacobian"], want["jacobian"])
    ch = M.case("H-C")
    he = kd.HEEstimator(64, 32, 3, 3, 2048).eval()
    he.load_state_dict(ch["sd"], strict=True)
    xh = T(ch["x"]).to(DEV)
    out, want = he.to(DEV)(xh), ops.he_estimator_forward(xh, _net("H-C"))
    assert all(torch.equal(out[k], want[k]) for k in M.HE_OUTPUTS)


def test_graph_replay_gives_the_eager_bits(ops):
    kp_net, he_net = _net("K-A"), _net("H-B")
    frames = T(M.to_float(M.images_u8(6, 3, 64, 64))).to(DEV)
    source, driving = frames[:1].contiguous(), frames[1:].contiguous()
    eager = ops.reenact_keypoints(source, driving, kp_net, he_net)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.reenact_keypoints(source, driving, kp_net, he_net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.reenact_keypoints(source, driving, kp_net, he_net)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got["value"], want["value"]) and torch.equal(got["jacobian"], want["jacobian"])


def test_prepared_weights_follow_the_parameters(ops):
    c = M.case("K-C")
    net = M.make_module("K-C")
    net.load_state_dict(c["sd"], strict=True)
    net = net.to(DEV)
    x = T(c["x"]).to(DEV)
    before = ops.kp_detector_forward(x, net)["value"].clone()
    with torch.no_grad():
        net.kp.weight.mul_(0.5)
    after = ops.kp_detector_forward(x, net)["value"]
    assert not torch.equal(before, after)
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    sd["kp.weight"] = sd["kp.weight"] * 0.5
    assert torch.equal(after, ops.kp_detector_forward(x, sd)["value"])
