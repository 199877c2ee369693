"""Row f25 on the GPU: the five kernels of ``csrc/gcfsr.hip`` alone, bit for bit against the numpy float32 models of ``inpaint_model``; ``ops.inpaint_forward`` in
both arithmetics and on both up routes against the float64 model and the reference's stored outputs (``tests/golden/g35_inpaint.npz``); ``ops.inpaint_image``
under the uint8 rule; the bit-equality properties of the host layer; ``pipeline.inpaint_faces`` and the refusals.

Bounds: ``ARITH = "f32"`` is held to ``max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against itself in float64 (never the code under test); the
default ``"sb"`` to ``PIXEL_TOL = 1e-3`` max-abs on the raw output, the project's bar on generated pixels."""
import numpy as np
import pytest
import torch

import inpaint_model as M
from conftest import load_golden, record_parity
from e4s2024_amd import ops, ops_inpaint, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
_NETS = {}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g35_inpaint")


@pytest.fixture(autouse=True)
def _defaults():
    yield
    ops_inpaint.ARITH, ops_inpaint.UP_COMPOSED_MAX_WIDTH = "sb", 32


def _net(size):
    """``ops.FaceInpainting`` with the seeded weights on the device, one module per size (a module caches its prepared weights)."""
    if size not in _NETS:
        net = ops.FaceInpainting(size).eval()
        net.load_state_dict(M.state_dict(size), strict=True)
        _NETS[size] = net.to(DEV)
    return _NETS[size]


def _inputs(tag):
    c = M.case(tag)
    return c, T(c["x"]).to(DEV), T(c["in_size"]).to(DEV), [T(n).to(DEV) for n in c["noise"]]


def _offset(t):
    """A copy of ``t`` that starts one element past a 16-byte boundary: the kernels' one-element form."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


# ------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (1, 8, 16, 32)])
def test_scale_shift_act_is_bit_equal_to_the_model(shape):
    bs, C, h, w = shape
    rs = np.random.RandomState(sum(shape))
    y, shift = rs.standard_normal(shape).astype(np.float32), rs.standard_normal(shape).astype(np.float32)
    table1, table2 = (rs.uniform(-1, 1, (bs, C + 3)).astype(np.float32) for _ in (0, 1))             # the level's columns of a wider table
    bias = rs.uniform(-0.5, 0.5, C).astype(np.float32)
    want = M.scale_shift_act_model(y, shift, table1[:, 2:2 + C], table2[:, 2:2 + C], bias)
    assert (want < 0).any() and (want > 0).any()
    t1, t2, b = T(table1).to(DEV), T(table2).to(DEV), T(bias).to(DEV)
    yd = T(y).to(DEV)
    assert (h * w) % 4 != 0 or yd.data_ptr() % 16 == 0                                                # (1, 8, 16, 32): the 16-byte path
    got = ops.scale_shift_act(yd, T(shift).to(DEV), t1[:, 2:2 + C], t2[:, 2:2 + C], b)
    assert got is yd and np.array_equal(yd.cpu().numpy(), want)                                       # in place
    yo = _offset(T(y).to(DEV))                                                                        # single elements: the same bits
    ops.scale_shift_act(yo, _offset(T(shift).to(DEV)), t1[:, 2:2 + C].contiguous(), t2[:, 2:2 + C].contiguous(), b)
    assert np.array_equal(yo.cpu().numpy(), want)


def _masks(S):
    yy, xx = np.mgrid[0:S, 0:S]
    ragged = ((yy * 7 + xx * 3) % 5 < 2) & (yy > 0)
    return np.stack([np.zeros((S, S), bool), np.ones((S, S), bool), ragged]).astype(np.uint8)


@pytest.mark.parametrize("S", [5, 32])
def test_input_and_tail_are_bit_equal_to_the_model(S):
    rs = np.random.RandomState(S)
    hole = _masks(S)                                                                                  # empty, full, ragged
    faces = rs.randint(0, 256, (3, S, S, 3)).astype(np.uint8)
    faces[0, 0, :, 0] = np.arange(S) * 255 // max(S - 1, 1)                                           # both ends of the range
    x_want, in_want, count_want = M.input_model(faces, hole)
    fd, hd = T(faces).to(DEV), T(hole).to(DEV)
    x, in_size, count = ops.inpaint_input(fd, hd)
    assert x.dtype == torch.float32 and in_size.dtype == torch.float32 and count.dtype == torch.int32
    assert np.array_equal(x.cpu().numpy(), x_want) and np.array_equal(count.cpu().numpy(), count_want)
    assert np.array_equal(in_size.cpu().numpy(), in_want) and count_want[0] == 0 and count_want[1] == S * S and in_want[1] == 1
    img = rs.uniform(-0.5, 1.5, (3, 3, S, S)).astype(np.float32)
    img[2, 0, :2] = (np.arange(2 * S).reshape(2, S) % 256 + 0.5) / 255.0                              # ties: half to even
    want = M.tail_model(img, faces, hole)
    got = ops.inpaint_tail(T(img).to(DEV), fd, hd)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(got.cpu().numpy()[hole == 0], faces[hole == 0])                             # outside the hole: the input bytes exactly
    assert np.array_equal(got[0].cpu().numpy(), faces[0]) and {0, 255} <= set(want[1].ravel().tolist())
    if S % 2 == 0:                                                                                    # one-element form of both: the same bits
        x2, in2, count2 = ops.inpaint_input(_offset(fd), _offset(hd))
        assert torch.equal(x2, x) and torch.equal(in2, in_size) and torch.equal(count2, count)
        assert np.array_equal(ops.inpaint_tail(_offset(T(img).to(DEV)), fd, hd).cpu().numpy(), want)
    assert ops.inpaint_input(fd[:0], hd[:0])[0].shape == (0, 4, S, S) and ops.inpaint_tail(T(img).to(DEV)[:0], fd[:0], hd[:0]).shape == (0, S, S, 3)


def test_condition_is_bit_equal_to_the_model():
    rs = np.random.RandomState(11)
    levels = [tuple(rs.uniform(-1, 1, s).astype(np.float32) for s in ((c, 1), (c,), (c, 1), (c,))) for c in (37, 300)]      # two levels, more than one block
    in_size = np.float32([0, 1, 0.37])
    want1, want2 = M.condition_model(in_size, levels)
    dl = [tuple(T(t).to(DEV) for t in lv) for lv in levels]
    s1n, s2n = ops.inpaint_condition(T(in_size).to(DEV), [(lv[0], lv[1]) for lv in dl], [(lv[2], lv[3]) for lv in dl])
    assert s1n.shape == s2n.shape == (3, 337)
    assert np.array_equal(s1n.cpu().numpy(), want1) and np.array_equal(s2n.cpu().numpy(), want2)
    assert ops.inpaint_condition(T(in_size).to(DEV)[:0], [(lv[0], lv[1]) for lv in dl], [(lv[2], lv[3]) for lv in dl])[0].shape == (0, 337)


@pytest.mark.parametrize("H,W,S", M.MASK_PAIRS)
def test_mask_support_is_the_models(H, W, S):
    for soft in (False, True):
        mask = M.mask_case(H * 1000 + W + soft, H, W, soft)
        got = ops.cv_mask_support(T(mask).to(DEV), S)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), M.mask_support_model(mask, S))
    assert ops.cv_mask_support(T(mask).to(DEV)[:0], S).shape == (0, S, S)


# ------------------------------------------------------------------------------------------------ the network
def _check_forward(tag, golden, arith, width=32):
    c, x, in_size, noise = _inputs(tag)
    ops_inpaint.ARITH, ops_inpaint.UP_COMPOSED_MAX_WIDTH = arith, width
    out, latent = ops.inpaint_forward(x, in_size, _net(M.CASES[tag][0]), noise, return_latents=True)
    got = out.cpu().numpy()
    assert got.shape == c["want"].shape and latent.shape == c["latent"].shape
    err, err_ref = M.max_err(got, c["want"]), M.max_err(M.sampled(got), golden[f"{tag}.out"])
    err_lat = M.max_err(latent.cpu().numpy(), c["latent"])
    bar = M.bound(c["e32"], c["want"]) if arith == "f32" else M.PIXEL_TOL
    name = f"inpaint.{arith}.{tag}" + ("" if width == 32 else f".w{width}")
    print(f"{name}: against float64 {err:.3e} = {err / c['e32']:.2f} e32, against the reference {err_ref:.3e}, latent {err_lat:.3e} = "
          f"{err_lat / c['e32_latent']:.2f} e32; bar {bar:.3e}")
    record_parity(f"{name}.maxabs", err, bar)
    record_parity(f"{name}.maxabs_reference", err_ref, bar)
    assert err <= bar and err_ref <= bar
    if arith == "f32":
        assert err_lat <= M.bound(c["e32_latent"], c["latent"])
    else:
        assert err_lat <= M.PIXEL_TOL


@pytest.mark.parametrize("tag", ["i32", "i64"])
def test_forward_f32_against_the_model_and_the_reference(tag, golden):
    _check_forward(tag, golden, "f32")


@pytest.mark.parametrize("tag", ["i32", "i64", "i256"])
def test_forward_sb_meets_the_pixel_bar(tag, golden):
    _check_forward(tag, golden, "sb")


def test_forward_on_the_fused_up_route(golden):
    """``UP_COMPOSED_MAX_WIDTH = 8``: the 16 -> 32 up layer leaves the parity-composed form for ``e4s_modconv_up_fused_sb``; the prepared weights follow the knob."""
    c, x, in_size, noise = _inputs("i32")
    net = _net(32)
    composed = ops.inpaint_forward(x, in_size, net, noise)[0]
    _check_forward("i32", golden, "sb", width=8)
    fused = ops.inpaint_forward(x, in_size, net, noise)[0]
    assert not torch.equal(fused, composed) and M.max_err(fused.cpu().numpy(), composed.cpu().numpy()) <= 2 * M.PIXEL_TOL
    _check_forward("i32", golden, "f32", width=8)                                                    # (f32 keeps the composed exact-fp32 entry)


def test_image_follows_the_uint8_rule():
    c = M.case("i32")
    faces, hole, net = T(c["faces"]).to(DEV), T(c["hole"]).to(DEV), _net(32)
    noise = [T(n).to(DEV) for n in c["noise"]]
    ops_inpaint.ARITH = "f32"
    got = ops.inpaint_image(faces, hole, net, noise)
    assert got.dtype == torch.uint8 and got.shape == faces.shape
    share = M.check_u8(got.cpu().numpy(), c["want"], c["faces"], c["hole"], c["e32"])
    assert share >= 0.99
    assert torch.equal(got[1], faces[1])                                                              # an empty hole: the face comes back
    ops_inpaint.ARITH = "sb"
    sb = ops.inpaint_image(faces, hole, net, noise).cpu().numpy().astype(np.int32)
    off = np.abs(sb - np.rint(M.composite(c["want"], c["faces"], c["hole"]) * 255.0).astype(np.int32))
    record_parity("inpaint.image.sb.i32.levels_off", int(off.max()), 1, note=f"{(off > 0).mean():.4f} of the values differ; f32 strict share {share:.4f}")
    assert off.max() <= 1
    with pytest.raises(ValueError, match="32, 32, 3"):
        ops.inpaint_image(faces[:, :-1, :-1], hole[:, :-1, :-1], net, noise)


def test_bit_equalities_and_generators():
    c, x, in_size, noise = _inputs("i32")
    net = _net(32)
    out, latent = ops.inpaint_forward(x, in_size, net, noise, return_latents=True)
    assert torch.equal(out, ops.inpaint_forward(x, in_size.view(-1, 1), net, noise)[0])               # two runs; in_size [bs, 1]
    for b in range(x.shape[0]):                                                                       # a batch against its single samples
        one, lat = ops.inpaint_forward(x[b:b + 1], in_size[b:b + 1], net, [n[b:b + 1] for n in noise], return_latents=True)
        assert torch.equal(one[0], out[b]) and torch.equal(lat[0], latent[b])
    shared = [n[:1] for n in noise]                                                                   # one noise map for the whole batch
    assert torch.equal(ops.inpaint_forward(x, in_size, net, shared)[0], ops.inpaint_forward(x, in_size, net, [n.expand(2, -1, -1, -1) for n in shared])[0])
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    assert torch.equal(out, ops.inpaint_forward(x, in_size, sd, noise)[0])                            # a mapping as weights
    assert torch.equal(out, ops.inpaint_forward(x, in_size, {"params_ema": sd}, noise)[0])            # the checkpoint file as torch.load gives it
    assert ops.inpaint_forward(x[:0], in_size[:0], net, [n[:0] for n in noise])[0].shape == (0, 3, 32, 32)
    g1, g2, g3 = (torch.Generator(device=DEV).manual_seed(s) for s in (5, 5, 6))
    a, b, d = (ops.inpaint_forward(x, in_size, net, generator=g)[0] for g in (g1, g2, g3))
    assert torch.equal(a, b) and not torch.equal(a, d) and not torch.equal(a, out)
    assert not torch.equal(ops.inpaint_forward(x, in_size, net)[0], ops.inpaint_forward(x, in_size, net)[0])      # fresh draws per call, as the reference's


def test_graph_replay_gives_the_eager_bits():
    c, x, in_size, noise = _inputs("i32")
    net = _net(32)
    eager = ops.inpaint_forward(x, in_size, net, noise)[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.inpaint_forward(x, in_size, net, noise)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.inpaint_forward(x, in_size, net, noise)[0]
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------ the pipeline and the refusals
def test_inpaint_faces_is_the_chain_of_its_parts():
    c = M.case("i32")
    net = _net(32)
    faces = T(M.GM.images_u8(77, 2, 64)).to(DEV)
    mask = T(M.mask_case(9, 64, 64, True)).to(DEV)
    noise = [T(n).to(DEV) for n in c["noise"]]
    got = pipeline.inpaint_faces(net, faces, mask, noise=noise)
    small, hole = ops.pil_resize(faces, (32, 32)), ops.cv_mask_support(mask, 32)
    assert got.dtype == torch.uint8 and got.shape == (2, 32, 32, 3) and 0 < float(hole.float().mean()) < 1
    assert torch.equal(got, ops.inpaint_image(small, hole, net, noise))
    assert torch.equal(got[hole == 0], small[hole == 0]) and not torch.equal(got, small)
    assert torch.equal(pipeline.inpaint_faces(net, faces, (mask > 0).to(torch.uint8), noise=noise), got)      # a uint8 mask with the same support
    ragged = pipeline.inpaint_faces(net, faces[:, :50, :37].contiguous(), mask[:, :23, :29].contiguous(), noise=noise)
    assert ragged.shape == (2, 32, 32, 3)
    assert pipeline.inpaint_faces(net, faces[:0], mask[:0]).shape == (0, 32, 32, 3)
    g1, g2 = (torch.Generator(device=DEV).manual_seed(3) for _ in (0, 1))
    assert torch.equal(pipeline.inpaint_faces(net, faces, mask, generator=g1), pipeline.inpaint_faces(net, faces, mask, generator=g2))


def test_argument_errors_before_any_launch():
    c, x, in_size, noise = _inputs("i32")
    net = _net(32)
    faces, hole = T(c["faces"]).to(DEV), T(c["hole"]).to(DEV)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.inpaint_forward(x.cpu(), in_size.cpu(), net, [n.cpu() for n in noise])
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.inpaint_forward(x, in_size.cpu(), net, noise)
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.inpaint_forward(x, in_size, net, [noise[0].cpu()] + noise[1:])
    with pytest.raises(ValueError, match="generator"):
        ops.inpaint_forward(x, in_size, net, generator=torch.Generator())
    with pytest.raises(ValueError, match="float32"):
        ops.inpaint_forward(x.double(), in_size, net, noise)
    with pytest.raises(ValueError, match="size is 32"):
        ops.inpaint_forward(x[:, :, :16, :16], in_size, net, noise)
    with pytest.raises(ValueError, match="list of 3"):
        ops.inpaint_forward(x, in_size, net, noise[:2])
    with pytest.raises(ValueError, match=r"noise\[2\]"):
        ops.inpaint_forward(x, in_size, net, noise[:2] + [noise[2][:, :, :16]])
    with pytest.raises(ValueError, match="another batch"):
        ops.inpaint_image(faces, hole[:1], net)
    with pytest.raises(ValueError, match="another batch"):
        pipeline.inpaint_faces(net, faces, hole[:1])
    with pytest.raises(ValueError, match="contiguous"):
        ops.scale_shift_act(x.permute(0, 1, 3, 2), x, in_size.view(2, 1).expand(2, 4), in_size.view(2, 1).expand(2, 4), in_size[:1].expand(4))
    never = ops.FaceInpainting(32).eval().to(DEV)
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.inpaint_forward(x, in_size, never, noise)
    net.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            ops.inpaint_forward(x, in_size, net, noise)
        with pytest.raises(RuntimeError, match="training mode"):
            pipeline.inpaint_faces(net, faces, hole)
    finally:
        net.eval()
    ops_inpaint.ARITH = "bf16"
    with pytest.raises(ValueError, match="ARITH"):
        ops.inpaint_forward(x, in_size, net, noise)
    with pytest.raises(ValueError, match="ARITH"):
        ops.inpaint_image(faces, hole, net, noise)
