"""Row f13 on the GPU: the two kernels of ``csrc/parsenet.hip`` alone, ``e4s_bilinear_argmax`` at equal size, ``ops.parsenet_forward`` against the float64 model
``parsenet_model`` and the reference's stored outputs (``tests/golden/g24_parsenet.npz``), the masks under the strict-pixel rule, and the bit-equality
properties of the host layer.

Bounds: a case's logits and image are held to ``max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against itself in float64 (never the code under
test); labels and masks must be equal on every pixel whose float64 top-two margin exceeds twice the logit bar, and at most 1 % of a case's pixels may fall
outside that rule.  The stem is exact float32: bias and 27 fused multiply-adds are 28 roundings of partial sums below ``sum|w x| + |b|``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parsenet_model as PM
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import ops, pipeline
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
_NETS = {}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g24_parsenet")


def _net(tag):
    """``ops.ParseNet`` of a case with its seeded weights on the device, one module per network (a module caches its prepared weights)."""
    tag = "A" if tag == "E" else tag
    if tag not in _NETS:
        net = PM.make_module(tag)
        net.load_state_dict(PM.case(tag)["sd"], strict=True)
        _NETS[tag] = net.to(DEV)
    return _NETS[tag]


def _offset(t):
    """A copy of ``t`` that starts one element past a 16-byte boundary: the kernels' one-element form."""
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


# ------------------------------------------------------------------------------------------------ the kernels alone
def _stem(x, x_u8, w, b, bgr=True, out=None):
    src = x if x is not None else x_u8
    bs, (H, W) = src.shape[0], (src.shape[2:] if x is not None else src.shape[1:3])
    C0 = w.shape[0]
    out = torch.empty((bs, C0, H, W), dtype=torch.float32, device=DEV) if out is None else out
    lut = T(ops.img2tensor_table()).to(DEV)
    lib().call("e4s_parsenet_stem", _p(out), _p(x), _p(x_u8), _p(lut), 1 if bgr else 0, _p(w.reshape(C0, 27)), _p(b), bs, C0, H, W, _stream())
    return out


@pytest.mark.parametrize("bs,H,W,C0", [(2, 2, 2, 5), (2, 5, 7, 5), (1, 16, 16, 64)])
def test_stem_against_float64_and_its_forms(bs, H, W, C0):
    rs = np.random.RandomState(H * W + C0)
    img = rs.randint(0, 256, (bs, H, W, 3)).astype(np.uint8)
    x = PM.img2tensor(img)                                                                    # float32 of numpy's float64 expression, BGR flipped
    w = (rs.standard_normal((C0, 3, 3, 3)) / np.sqrt(27)).astype(np.float32)
    b = rs.uniform(-0.3, 0.3, C0).astype(np.float32)
    xd, ud, wd, bd = T(x).to(DEV), T(img).to(DEV), T(w).to(DEV), T(b).to(DEV)
    got = _stem(xd, None, wd, bd)
    xp = F.pad(T(x).double(), (1, 1, 1, 1), mode="reflect")
    want = F.conv2d(xp, T(w).double(), T(b).double()).numpy()
    mag = float((F.conv2d(xp.abs(), T(w).double().abs()) + T(b).double().abs().view(1, -1, 1, 1)).max())
    tol = 28 * 2.0 ** -24 * mag
    err = PM.max_err(got.cpu().numpy(), want)
    record_parity(f"parsenet.stem.{H}x{W}.c{C0}", err, tol)
    assert got.shape == want.shape and err <= tol
    # the uint8 form gives the float form's bits; BGR of an image is RGB of its flip; the vector and the one-element forms agree bit for bit
    assert torch.equal(_stem(None, ud, wd, bd), got)
    assert torch.equal(_stem(None, ud.flip(3).contiguous(), wd, bd, bgr=False), got)
    assert torch.equal(_stem(_offset(xd), None, wd, bd), got)
    assert torch.equal(_stem(None, _offset(ud), wd, bd), got)
    assert torch.equal(_stem(None, _offset(ud.flip(3).contiguous()), wd, bd, bgr=False), got)
    assert torch.equal(_stem(xd, None, wd, bd, out=_offset(torch.empty_like(got))), got)


def test_stem_img2tensor_on_all_levels():
    img = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    w = torch.zeros(3, 3, 3, 3, device=DEV)
    w[0, 0, 1, 1] = w[1, 1, 1, 1] = w[2, 2, 1, 1] = 1.0                                       # the centre tap: the input itself
    got = _stem(None, T(img).to(DEV), w, torch.zeros(3, device=DEV))
    assert np.array_equal(got.cpu().numpy(), PM.img2tensor(img))


def _pad(x, add, u, out=None):
    planes, h, w = x.shape
    out = torch.full((planes, u * h + 2, u * w + 2), float("nan"), device=DEV) if out is None else out
    lib().call("e4s_parsenet_pad", _p(out), _p(x), _p(add), planes, h, w, u, _stream())
    return out


@pytest.mark.parametrize("planes,h,w", [(3, 2, 2), (5, 3, 5), (4, 6, 6), (2, 1, 1), (2, 14, 8)])
def test_pad_is_bit_equal_to_pytorch(planes, h, w):
    g = torch.Generator(device="cpu").manual_seed(planes * h + w)
    x, add = torch.randn(planes, h, w, generator=g).to(DEV), torch.randn(planes, h, w, generator=g).to(DEV)
    for u in ((2,) if min(h, w) < 2 else (1, 2)):
        for a in (add, None):
            v = (x + a if a is not None else x)[None]
            if u == 2:
                v = F.interpolate(v, scale_factor=2, mode="nearest")
            want = F.pad(v, (1, 1, 1, 1), mode="reflect")[0]
            got = _pad(x, a, u)
            assert got.shape == want.shape and torch.equal(got, want), (u, a is not None)
            assert torch.equal(_pad(_offset(x), None if a is None else _offset(a), u), want)
            assert torch.equal(_pad(x, a, u, out=_offset(torch.full_like(want, float("nan")))), want)
    with pytest.raises(RuntimeError, match="2 x 2"):
        _pad(torch.zeros(1, 1, 4, device=DEV), None, 1)
    with pytest.raises(RuntimeError, match="u is 1 or 2"):
        _pad(x, None, 3)
    _pad(x[:0], None, 2)                                                                      # no planes: returns at once


@pytest.mark.parametrize("h,w", [(7, 9), (64, 64)])
def test_equal_size_bilinear_argmax_is_argmax_and_table(h, w):
    g = torch.Generator(device="cpu").manual_seed(h)
    logits = (torch.randn(2, 19, h, w, generator=g) * 4).to(DEV)
    table = torch.tensor(PM.MASK_COLORMAP, dtype=torch.uint8, device=DEV)
    out = torch.empty((2, h, w), dtype=torch.uint8, device=DEV)
    lib().call("e4s_bilinear_argmax", _p(out), _p(logits), _p(table), 2, 19, h, w, h, w, _stream())
    labels = torch.argmax(logits, dim=1)
    assert torch.equal(out, table[labels])
    lib().call("e4s_bilinear_argmax", _p(out), _p(logits), None, 2, 19, h, w, h, w, _stream())
    assert torch.equal(out.long(), labels)


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("tag", list(PM.CASES))
def test_forward_against_the_model_and_the_reference(tag, golden):
    c = PM.case(tag)
    n = PM.STORED[tag]
    mask, img = ops.parsenet_forward(T(c["x"]).to(DEV), _net(tag), with_image=True)
    got_m, got_i = mask.cpu().numpy(), img.cpu().numpy()
    bar_m, bar_i = PM.bound(c["e32_mask"], c["mask64"]), PM.bound(c["e32_img"], c["img64"])
    err_m, err_i = PM.max_err(got_m, c["mask64"]), PM.max_err(got_i, c["img64"])
    ref_m, ref_i = PM.max_err(got_m[:n], golden[f"{tag}.out_mask"]), PM.max_err(got_i[:n], golden[f"{tag}.out_img"])
    print(f"{tag}: logits against float64 {err_m:.3e} = {err_m / c['e32_mask']:.2f} e32, against the reference {ref_m:.3e}; image {err_i:.3e} = "
          f"{err_i / c['e32_img']:.2f} e32, against the reference {ref_i:.3e}")
    record_parity(f"parsenet.{tag}.logits.err_over_e32", err_m / c["e32_mask"], PM.MARGIN)
    record_parity(f"parsenet.{tag}.image.err_over_e32", err_i / c["e32_img"], PM.MARGIN)
    record_parity(f"parsenet.{tag}.logits.maxabs", err_m, bar_m)
    record_parity(f"parsenet.{tag}.logits.maxabs_reference", ref_m, 2 * bar_m)
    assert got_m.shape == c["mask64"].shape and got_i.shape == c["img64"].shape
    assert err_m <= bar_m and err_i <= bar_i
    # the reference's float32 output is itself within one bar of the model (test_parsenet_cpu.py), so two outputs inside the bar are within two of each other
    assert ref_m <= 2 * bar_m and ref_i <= 2 * bar_i


@pytest.mark.parametrize("tag", list(PM.CASES))
def test_labels_and_masks_on_strict_pixels(tag):
    c = PM.case(tag)
    net = _net(tag)
    logits = ops.parsenet_forward(T(c["x"]).to(DEV), net)[0]
    labels = logits.argmax(1).cpu().numpy()
    share = PM.check_labels(labels, c)
    off = int((labels != c["labels"]).sum())
    record_parity(f"parsenet.{tag}.nonstrict_share", share, PM.NONSTRICT_CAP, note=f"{off} of {labels.size} labels differ from the float64 model's, none of them strict")
    img = T(c["img"]).to(DEV)
    if tag == "E":                                                                            # a ragged input is not at in_size: the mask entry refuses it
        with pytest.raises(ValueError, match="in_size is 16"):
            ops.parsenet_mask(img, net)
        return
    mask = ops.parsenet_mask(img, net)
    assert mask.dtype == torch.uint8 and mask.is_cuda
    PM.check_mask(mask.cpu().numpy(), c)
    assert torch.equal(mask, T(PM.mask_of(labels)).to(DEV))                                   # the uint8 stem gives the float stem's bits, so the same labels
    assert torch.equal(pipeline.gpen_face_mask(net, img.flip(3).contiguous()), mask)          # RGB in: the flip and bgr=False cancel
    assert torch.equal(ops.parsenet_mask(img.flip(3).contiguous(), net, bgr=False), mask)


def test_mask_from_tensor():
    c = PM.case("A")
    net = _net("A")
    imt = (T(c["img"]).permute(0, 3, 1, 2).float() / 255).contiguous()                        # BGR planes in [0, 1], as process_tensor takes them
    x = imt.flip(1) * 2 - 1                                                                   # each operation rounded on its own
    m64 = PM.network(c["sd"], x)[0].numpy()
    m32 = PM.network(c["sd"], x, dtype=torch.float32)[0].numpy()
    top2 = np.sort(m64, axis=1)[:, -2:]
    own = dict(labels=m64.argmax(1), strict=(top2[:, 1] - top2[:, 0]) > 2 * PM.bound(PM.max_err(m32, m64), m64))
    own["mask"] = PM.mask_of(own["labels"])
    got = ops.parsenet_mask_from_tensor(imt.to(DEV), net)
    assert got.dtype == torch.int64 and got.shape == (1, 2, 16, 16)
    PM.check_mask(got[0].cpu().numpy().astype(np.uint8), own)
    logits = ops.parsenet_forward(x.to(DEV), net)[0]
    assert torch.equal(got[0], T(np.asarray(PM.MASK_COLORMAP)).to(DEV)[logits.argmax(1)])
    with pytest.raises(ValueError, match="in_size is 16"):
        ops.parsenet_mask_from_tensor(imt[:, :, :8].to(DEV), net)


def test_bit_equalities():
    tag = "B"
    c = PM.case(tag)
    x, net = T(c["x"]).to(DEV), _net(tag)
    mask, none = ops.parsenet_forward(x, net)
    assert none is None and mask.is_contiguous()
    assert torch.equal(mask, ops.parsenet_forward(x, net)[0])                                 # two runs
    for b in range(x.shape[0]):                                                               # a batch against its single samples
        assert torch.equal(ops.parsenet_forward(x[b:b + 1], net)[0][0], mask[b])
    assert torch.equal(mask, ops.parsenet_forward(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), net)[0])      # strides do not matter
    both, img = ops.parsenet_forward(x, net, with_image=True)                                 # the 22-output head gives the 19-output head's logits
    assert torch.equal(both, mask) and img.shape == (2, 3, 64, 64)
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    assert torch.equal(mask, ops.parsenet_forward(x, sd)[0])                                  # a mapping as weights
    empty = ops.parsenet_forward(x[:0], net, with_image=True)
    assert empty[0].shape == (0, 19, 64, 64) and empty[1].shape == (0, 3, 64, 64)
    e = PM.case("E")                                                                          # the ragged case too: batch against single samples
    xe = T(e["x"]).to(DEV)
    me = ops.parsenet_forward(xe, _net("E"))[0]
    assert me.shape == (2, 19, 20, 12) and all(torch.equal(ops.parsenet_forward(xe[b:b + 1], _net("E"))[0][0], me[b]) for b in range(2))
    install_dropin()
    from swap_face_fine.gpen.face_parse.parse_model import ParseNet
    cfg = PM.config(tag)
    full = ParseNet(cfg["in_size"], cfg["out_size"], cfg["min_feat_size"], cfg["base_ch"], 19, cfg["res_depth"], norm_type="bn", relu_type="LeakyReLU",
                    ch_range=list(cfg["ch_range"])).eval()
    full.load_state_dict(c["sd"], strict=True)
    full = full.to(DEV)
    out_mask, out_img = full(x)
    assert torch.equal(out_mask, mask) and torch.equal(out_img, img)
    with pytest.raises(NotImplementedError, match="eval"):
        full.train()(x)


def test_graph_replay_gives_the_eager_bits():
    c = PM.case("A")
    img, net = T(c["img"]).to(DEV), _net("A")
    x = T(c["x"]).to(DEV)
    eager_mask, eager_logits = ops.parsenet_mask(img, net), ops.parsenet_forward(x, net, with_image=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.parsenet_mask(img, net)
        ops.parsenet_forward(x, net, with_image=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mask = ops.parsenet_mask(img, net)
        logits = ops.parsenet_forward(x, net, with_image=True)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mask, eager_mask) and torch.equal(logits[0], eager_logits[0]) and torch.equal(logits[1], eager_logits[1])


def test_prepared_weights_follow_the_parameters():
    c = PM.case("A")
    x = T(c["x"]).to(DEV)
    net = PM.make_module("A")
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.parsenet_forward(x, net.to(DEV))
    net.load_state_dict(c["sd"], strict=True)
    net = net.to(DEV)
    before = ops.parsenet_forward(x, net)[0]
    with torch.no_grad():
        net.out_mask_conv.conv2d.bias.add_(0.25)                                              # in place: the same storage, a new version
    after = ops.parsenet_forward(x, net)[0]
    assert np.abs((after - before).cpu().numpy() - 0.25).max() <= 1e-5
    assert ops.invalidate_weight_caches(net) >= 1
    assert torch.equal(ops.parsenet_forward(x, net)[0], after)


def test_argument_errors_before_any_launch():
    c = PM.case("A")
    x, img, net = T(c["x"]).to(DEV), T(c["img"]).to(DEV), _net("A")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.parsenet_forward(x.cpu(), net)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.parsenet_mask(img.cpu(), net)
    with pytest.raises(ValueError, match="float32"):
        ops.parsenet_forward(x.double(), net)
    with pytest.raises(ValueError, match="in_size is 16"):
        ops.parsenet_mask(img[:, :8, :8], net)
    with pytest.raises(ValueError, match="2 x 2"):
        ops.parsenet_forward(x[:, :, :4, :4], net)
    net.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            ops.parsenet_forward(x, net)
    finally:
        net.eval()
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.parsenet_mask(img, PM.make_module("A").to(DEV))
