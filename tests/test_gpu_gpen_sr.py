"""Row f16 on the device: its three kernels (csrc/gpen_sr.hip, the tail on csrc/rrdb.hip) alone, ``ops.gpen_sr_forward`` / ``gpen_sr_image`` / ``cv_resize_linear`` against
tests/gpen_sr_model.py on the cases of g27_gpen_sr.npz, and ``pipeline.gpen_face_enhancement`` with the drop-in ``FaceEnhancement`` against the composition of
their pieces and against what the reference's ``process`` gave.  Small shapes throughout: each test takes seconds.

The bars.  ``e4s_gsr_input``, the float output of ``e4s_gsr_tail`` and the resize: bit for bit the model (a correctly rounded division; one fused multiply-add
per tap in a fixed order; integer arithmetic).  A network case: ``max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against itself in float64,
never the code under test.  uint8 images: the model's uint8 rule."""
import os

import numpy as np
import pytest
import torch

import gpen_paste_model as PM
import gpen_sr_model as M
import test_gpu_gpen_paste as TP
from conftest import GOLDEN, install_dropin, record_parity
from e4s2024_amd import ops, pipeline
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
_NETS = {}
_WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "g27_gpen_sr.npz")) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return T(a).to(DEV)


def _net(sd, key):
    """``ops.GpenSRNet`` with ``sd`` on the device, one module per ``key`` (a module caches its prepared weights)."""
    if key not in _NETS:
        net = ops.GpenSRNet(M.num_blocks(sd), int(sd["conv_first.weight"].shape[0]), M.scale_of(sd)).eval()
        net.load_state_dict(sd, strict=True)
        _NETS[key] = net.to(DEV)
    return _NETS[key]


def _offset(t):
    """A copy of ``t`` that starts one element past a 16-byte boundary: the kernels' one-element form."""
    if t is None:
        return None
    flat = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _conditioned(strict, clamped, std):
    return strict >= 0.99 and clamped < 0.10 and std > 30


# ------------------------------------------------------------------------------------------------ e4s_gsr_input
def _gsr_input(img, r, bgr, off=False):
    bs, H, W, _ = img.shape
    out = torch.empty((bs, 3 * r * r, (H + -H % r) // r, (W + -W % r) // r), dtype=torch.float32, device=DEV)
    out = _offset(out) if off else out
    lib().call("e4s_gsr_input", _p(out), _p(img), bs, H, W, r, int(bgr), _stream())
    return out


@pytest.mark.parametrize("H,W", [(5, 3), (7, 9), (12, 20), (6, 17), (7, 15)])
@pytest.mark.parametrize("r", [1, 2, 4])
def test_gsr_input_bit_for_bit(r, H, W):
    """v / 255, the flip, the reflect pad and the unshuffle: the sizes cover a pad of 0 - 3 on each axis.  Output rows that are whole 16-byte groups: 12 x 20 at
    r 1, 7 x 15 at r 2 and r 4 (rows of 8 and 4, with a reflected column inside the last group); every other pair takes single elements, as does the form at an
    offset, with the same bits."""
    for bs in (1, 2):
        img = M.images_u8(H * 100 + W + r, bs, H, W)
        for bgr in (False, True):
            want = M.sr_input_unshuffled_f32(img, r, bgr)
            got = _gsr_input(dev(img), r, bgr)
            assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), (bs, bgr)
            assert torch.equal(_gsr_input(dev(img), r, bgr, off=True), got)
    assert _gsr_input(dev(img)[:0], r, True).shape[0] == 0
    vec = ((W + -W % r) // r) % 4 == 0
    print(f"r {r}, {H} x {W}: pad {-H % r} x {-W % r}, output rows of {(W + -W % r) // r}: the {'16-byte' if vec else 'one-element'} form")


def test_gsr_input_refuses_what_cannot_be_padded():
    img = torch.zeros((1, 1, 8, 3), dtype=torch.uint8, device=DEV)
    out = torch.empty(64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="reflect-padded"):
        lib().call("e4s_gsr_input", _p(out), _p(img), 1, 1, 8, 2, 1, _stream())
    with pytest.raises(RuntimeError, match="r is 1, 2 or 4"):
        lib().call("e4s_gsr_input", _p(out), _p(img), 1, 1, 8, 3, 1, _stream())


# ------------------------------------------------------------------------------------------------ e4s_gsr_tail
def _tail(x, w, b, crop, bgr, out_f=True, off=False):
    bs, C, H, W = x.shape
    Ho, Wo = H - crop[0], W - crop[1]
    u8 = torch.empty((bs, Ho, Wo, 3), dtype=torch.uint8, device=DEV)
    f = torch.empty((bs, 3, H, W), dtype=torch.float32, device=DEV) if out_f else None
    if off:
        x, u8, f = _offset(x), _offset(u8), _offset(f)
    lib().call("e4s_gsr_tail", _p(u8), _p(f), _p(x), _p(w), _p(b), bs, C, H, W, Ho, Wo, int(bgr), _stream())
    return u8, f


@pytest.mark.parametrize("C,H,W", M.TAIL_CASES)
def test_gsr_tail(C, H, W):
    """The float output bit for bit the fused float32 chain in the documented order (``gpen_sr_model.tail_f32``); the uint8 image by the uint8 rule against
    float64, and bit for bit the rounding end applied to the kernel's own float output; crops of 0 and 1 - 3 (and 4 columns: the packed form with a crop), both
    channel orders; the form at an offset and the call without the float output give the same bits.  20 x 20 spans two tiles down."""
    m = M.tail_case(C, H, W)
    x, w, b, bs = m["x"], m["w"], m["b"], 2
    xd, wd, bd = dev(x), dev(w), dev(b)
    for crop in M.TAIL_CROPS:
        for bgr in (False, True):
            u8, f = _tail(xd, wd, bd, crop, bgr)
            assert np.array_equal(f.cpu().numpy(), m["f32"]), "the float output is not the fused float32 chain"
            u = M.to_u8(m["r"], crop, bgr=bgr)[0]
            stats = M.check_u8(u8.cpu().numpy(), u, m["e32"])
            assert _conditioned(*stats), stats
            assert np.array_equal(u8.cpu().numpy(), M.to_u8(m["f32"], crop, bgr=bgr)[1])
            u8_off, f_off = _tail(xd, wd, bd, crop, bgr, off=True)
            assert torch.equal(u8_off, u8) and torch.equal(f_off, f)
            assert torch.equal(_tail(xd, wd, bd, crop, bgr, out_f=False)[0], u8)
    print(f"C {C}, {H} x {W}: e32 {m['e32']:.3e}; strict {100 * stats[0]:.2f} %, clamped {100 * stats[1]:.2f} %, std {stats[2]:.1f}")
    with pytest.raises(RuntimeError, match="multiple of 8"):
        lib().call("e4s_gsr_tail", _p(u8), None, _p(xd), _p(wd), _p(bd), bs, 12, H, W, H, W, 0, _stream())
    with pytest.raises(RuntimeError, match="crop"):
        lib().call("e4s_gsr_tail", _p(u8), None, _p(xd), _p(wd), _p(bd), bs, C, H, W, H + 1, W, 0, _stream())


def test_gsr_tail_rounds_half_to_even():
    """Values whose float32 product with 255 is exactly k + 0.5, through conv_last as the identity on one channel: the even neighbour, never half-up."""
    ties = M.tie_values()
    n = len(ties)
    x = np.zeros((1, 8, 1, n), np.float32)
    x[0, 0, 0] = ties
    w = np.zeros((3, 8, 3, 3), np.float32)
    w[:, 0, 1, 1] = 1.0
    u8, f = _tail(dev(x), dev(w), dev(np.zeros(3, np.float32)), (0, 0), False)
    assert np.array_equal(f.cpu().numpy()[0, 0, 0], ties)
    want = M.to_u8(f.cpu().numpy(), (0, 0), bgr=False)[1]
    assert np.array_equal(u8.cpu().numpy(), want) and (want % 2 == 0).all()
    assert (M.to_u8(f.cpu().numpy(), (0, 0), bgr=False, mutant="half_up")[1] != want).sum() >= 100


# ------------------------------------------------------------------------------------------------ cv_resize_linear
@pytest.mark.parametrize("H,W,Ho,Wo", [(5, 7, 11, 15), (8, 8, 32, 32), (9, 6, 18, 12), (40, 36, 17, 23), (1, 5, 3, 10)])
def test_cv_resize_linear_bit_for_bit(H, W, Ho, Wo):
    img = M.images_u8(H * 1000 + Wo, 2, H, W)
    got = ops.cv_resize_linear(dev(img), (Wo, Ho))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, Ho, Wo, 3) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), M.resize_linear(img, (Wo, Ho)))
    assert torch.equal(ops.cv_resize_linear(dev(img)[1:], (Wo, Ho)), got[1:])
    wide = torch.zeros((2, H, W + 3, 3), dtype=torch.uint8, device=DEV)
    wide[:, :, :W] = dev(img)
    assert torch.equal(ops.cv_resize_linear(wide[:, :, :W], (Wo, Ho)), got)                   # a non-contiguous view is accepted
    assert ops.cv_resize_linear(dev(img)[:0], (Wo, Ho)).shape == (0, Ho, Wo, 3)


def test_cv_resize_linear_edges():
    img = dev(M.images_u8(9, 1, 6, 8))
    assert torch.equal(ops.cv_resize_linear(img, (8, 6)), img)                                # the identity
    assert np.array_equal(ops.cv_resize_linear(img, (4, 4)).cpu().numpy(), M.resize_linear(img.cpu().numpy(), (4, 4)))      # 2 : 1 on one axis alone
    with pytest.raises(ValueError, match="INTER_AREA"):
        ops.cv_resize_linear(img, (4, 3))
    with pytest.raises(RuntimeError, match="INTER_AREA"):
        lib().call("e4s_cv_resize_linear_u8", _p(torch.empty(36, dtype=torch.uint8, device=DEV)), _p(img), 1, 6, 8, 3, 4, _stream())
    ramp = dev(np.tile(np.array([0, 64, 128, 192], np.uint8)[None, None, :, None], (1, 2, 1, 3)))
    assert ops.cv_resize_linear(ramp, (8, 2))[0, 0, :, 0].tolist() == [0, 16, 48, 80, 112, 144, 176, 192]


# ------------------------------------------------------------------------------------------------ the network and the image
@pytest.mark.parametrize("tag", list(M.IMAGE_CASES))
def test_network_and_image_on_the_golden_cases(tag, golden):
    c = M.image_case(tag)
    scale, nf, nb, H, W = M.IMAGE_CASES[tag]
    net = _net(c["sd"], tag)
    x = M.sr_input(c["img"], scale, True, torch.float32).to(DEV)                              # the padded float32 image: what the reference's network sees
    out = ops.gpen_sr_forward(x, net)
    assert out.dtype == torch.float32 and tuple(out.shape) == c["r"].shape and out.is_contiguous()
    err, bound = M.max_err(out.cpu().numpy(), c["r"]), M.bound(c["e32"], c["r"])
    _WORST["ratio"] = max(_WORST["ratio"], err / c["e32"])
    print(f"{tag}: kernels against float64 {err:.3e} = {err / c['e32']:.2f} e32, e32 {c['e32']:.3e}, bound {bound:.3e}")
    record_parity("gpen_sr.worst_err_over_e32", _WORST["ratio"], M.MARGIN, "gpen_sr_forward against the float64 model, in units of the float32 model's own error")
    assert err <= bound
    img = ops.gpen_sr_image(dev(c["img"]), net)
    assert img.dtype == torch.uint8 and tuple(img.shape) == (1,) + M.output_size(H, W, scale) + (3,) and img.is_contiguous()
    stats = M.check_u8(img.cpu().numpy(), c["u"], c["e32"])
    print(f"{tag}: uint8 strict {100 * stats[0]:.2f} %, clamped {100 * stats[1]:.2f} %, std {stats[2]:.1f}")
    assert _conditioned(*stats)
    assert np.abs(img[0].cpu().numpy().astype(int) - golden[f"{tag}.out"].astype(int)).max() <= 1          # the reference's own image
    rgb = ops.gpen_sr_image(dev(c["img"][..., ::-1]), net, bgr=False)                         # RGB in and out: the same network input, the same image flipped
    assert torch.equal(rgb.flip(-1), img)
    assert torch.equal(pipeline.gpen_super_resolve(net, dev(c["img"][..., ::-1])), rgb)


def test_full_depth_batches_views_and_mappings():
    c = M.deep_case()
    tag, scale, nf, nb, h, w, bs = M.DEEP_CASE
    x, net = dev(c["x"]), _net(c["sd"], tag)
    out = ops.gpen_sr_forward(x, net)
    err, bound = M.max_err(out.cpu().numpy(), c["want"]), M.bound(c["e32"], c["want"])
    print(f"{tag}: kernels against float64 {err:.3e} = {err / c['e32']:.2f} e32, e32 {c['e32']:.3e}, bound {bound:.3e}")
    assert tuple(out.shape) == (bs, 3, scale * h, scale * w) and err <= bound
    assert torch.equal(out, ops.gpen_sr_forward(x, net))                                      # two runs: the same bits
    assert torch.equal(out, torch.cat([ops.gpen_sr_forward(x[i:i + 1], net) for i in range(bs)]))
    assert torch.equal(out, ops.gpen_sr_forward(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), net))         # strides do not matter
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    assert torch.equal(out, ops.gpen_sr_forward(x, {"params_ema": sd}))                       # a mapping as weights
    assert ops.gpen_sr_forward(x[:0], net).shape == (0, 3, scale * h, scale * w)
    img = dev(M.images_u8(77, bs, 7, 9))
    u8 = ops.gpen_sr_image(img, net)
    assert tuple(u8.shape) == (bs, 15, 19, 3) and torch.equal(u8, ops.gpen_sr_image(img, net))
    assert torch.equal(u8, torch.cat([ops.gpen_sr_image(img[i:i + 1], net) for i in range(bs)]))
    wide = torch.zeros((bs, 7, 12, 3), dtype=torch.uint8, device=DEV)
    wide[:, :, :9] = img
    assert torch.equal(ops.gpen_sr_image(wide[:, :, :9], net), u8)
    assert ops.gpen_sr_image(img[:0], net).shape == (0, 15, 19, 3)


def test_graph_replay_gives_the_eager_bits():
    tag = M.tag_of(2, 32, 1, 7, 9)
    c = M.image_case(tag)
    img, net = dev(c["img"]), _net(c["sd"], tag)
    eager = ops.gpen_sr_image(img, net)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gpen_sr_image(img, net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                             # single stream: no parallel branches
        out = ops.gpen_sr_image(img, net)
        small = ops.cv_resize_linear(out, (9, 7))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(small, ops.cv_resize_linear(eager, (9, 7)))


# ------------------------------------------------------------------------------------------------ end to end
def _paste_constants(monkeypatch):
    """The production constants (101 taps) do not fit a 32 x 32 mask: the cases' own, as tests/test_gpu_gpen_paste.py sets them."""
    P = M.FE_PASTE
    for key in ("ksize", "sigma", "thres", "small_face"):
        monkeypatch.setitem(ops.GPEN_PASTE_DEFAULTS, key, P[key])


def _fe_sr(tag, img_bgr):
    return _net(M.fe_solved(tag, img_bgr)["sd"], tag)


def test_face_enhancement_is_the_composition_of_its_pieces(monkeypatch):
    """With the seeded detector, generator and ParseNet of tests/test_gpu_gpen_paste.py: bit for bit the steps written out; ``sr=None`` is
    ``gpen_enhance_frames``; the aligned branch; a batch equals its single frames; the drop-in ``FaceEnhancement`` returns the same arrays."""
    detector, gpen, parsenet = TP._nets()
    _paste_constants(monkeypatch)
    bgr = np.stack([M.fe_frame("fe.full"), M.fe_frame("fe.full")[::-1, ::-1]])
    sr = _fe_sr("fe.full", bgr[0])
    frames = dev(bgr[..., ::-1])
    out, orig, enh = pipeline.gpen_face_enhancement(detector, gpen, parsenet, sr, frames, return_faces=True)
    img_sr = ops.gpen_sr_image(frames, sr, bgr=False)
    resized = ops.cv_resize_linear(frames, (96, 80))
    per_frame = pipeline.gpen_detect_faces(detector, resized, bgr=False)
    print("faces per frame:", [len(d) for d, _ in per_frame])
    want, of, ef, flags = TP._composition(gpen, parsenet, resized, img_sr, per_frame)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 80, 96, 3) and torch.equal(out, want)
    assert torch.equal(torch.cat(orig), of[(flags & 1) == 0]) and torch.equal(torch.cat(enh), ef[(flags & 1) == 0])
    assert torch.equal(pipeline.gpen_face_enhancement(detector, gpen, parsenet, sr, frames), out)
    singles = torch.cat([pipeline.gpen_face_enhancement(detector, gpen, parsenet, sr, frames[b:b + 1]) for b in range(2)])
    assert torch.equal(singles, out)
    # without the RealESRNet pass: gpen_enhance_frames, nothing else
    big = dev(np.stack([M.resize_linear(b, (96, 80)) for b in bgr])[..., ::-1])
    assert torch.equal(pipeline.gpen_face_enhancement(detector, gpen, parsenet, None, big), pipeline.gpen_enhance_frames(detector, gpen, parsenet, big))
    # aligned: the generator, then the RealESRNet pass, the results in the reference's order
    faces = dev(M.images_u8(5, 2, 32, 32, noise=10))
    ef = pipeline.gpen_enhance(gpen, faces)
    a_out, a_orig, a_enh = pipeline.gpen_face_enhancement(None, gpen, None, sr, faces, aligned=True, return_faces=True)
    assert torch.equal(a_out, ops.gpen_sr_image(ef, sr, bgr=False)) and tuple(a_out.shape) == (2, 64, 64, 3)
    assert len(a_orig) == len(a_enh) == 1 and a_orig[0] is faces and torch.equal(a_enh[0], ef)
    assert torch.equal(pipeline.gpen_face_enhancement(None, gpen, None, None, faces, aligned=True), ef)
    with pytest.raises(ValueError, match="aligned faces are 32 x 32"):
        pipeline.gpen_face_enhancement(None, gpen, None, sr, frames, aligned=True)
    # the drop-in: numpy BGR in and out
    install_dropin()
    import e4s2024_amd
    try:
        from swap_face_fine.gpen.face_enhancement import FaceEnhancement
        from swap_face_fine.gpen.sr_model.real_esrnet import RealESRNet
        fe = FaceEnhancement.from_networks(detector, gpen, parsenet, sr, use_sr=True, device=DEV)
        d_out, d_orig, d_enh = fe.process(bgr[0])
        assert d_out.dtype == np.uint8 and np.array_equal(d_out, out[0].flip(-1).cpu().numpy())
        assert len(d_orig) == len(orig[0]) == len(d_enh) and all(np.array_equal(a, b.flip(-1).cpu().numpy()) for a, b in zip(d_enh, enh[0]))
        face_bgr = faces[0].flip(-1).cpu().numpy()
        d_out, d_orig, d_enh = fe.process(face_bgr, aligned=True)
        assert np.array_equal(d_out, a_out[0].flip(-1).cpu().numpy()) and d_orig[0] is face_bgr and np.array_equal(d_enh[0], ef[0].flip(-1).cpu().numpy())
        plain = FaceEnhancement.from_networks(detector, gpen, parsenet, sr, use_sr=False, device=DEV)
        assert np.array_equal(plain.process(face_bgr, aligned=True)[0], d_enh[0])
        resr = object.__new__(RealESRNet)
        resr.base_dir, resr.scale, resr.device, resr.srmodel = "./", 2, DEV, sr
        assert np.array_equal(resr.process(bgr[0]), img_sr[0].flip(-1).cpu().numpy())
        with pytest.raises(ValueError, match="reflect pad"):
            resr.process(np.zeros((1, 8, 3), np.uint8))
    finally:
        e4s2024_amd.uninstall()


@pytest.mark.parametrize("tag", ["fe.full", "fe.odd"])
def test_face_enhancement_against_the_reference_process(tag, golden, monkeypatch):
    """The reference's ``process`` with ``use_sr`` on the golden's cases: its stub networks' detections, faces and masks are fed to the chain here too (the
    detector, the generator and the ParseNet replaced by the recorded results), the RealESRNet pass, the resize, the crops and the paste run on the device.
    ``img_sr`` by the uint8 rule; the resized frame bit for bit; outside the faces' reach the result IS ``img_sr``; inside, a pixel may leave the reference's
    only where the model says it may: where ``img_sr`` is not strict, where the paste is not strict (gpen_paste_model.strict_pixels), or — the device forms its
    transforms in float64, the reference in float32 — on a fixed-point coordinate's rounding edge, 2e-3 of the pixels (row f15's figure)."""
    rec = M.fe_record(golden, tag)
    detector, gpen, parsenet = TP._nets()
    _paste_constants(monkeypatch)
    monkeypatch.setattr(pipeline, "gpen_detect_faces", lambda net, frames, bgr=True: [(dev(rec["dets"]), dev(rec["landms"]))] * frames.shape[0])
    monkeypatch.setattr(pipeline, "gpen_enhance", lambda weights, faces: dev(rec["ef"][..., ::-1]))
    monkeypatch.setattr(pipeline, "gpen_face_mask", lambda net, faces: dev(rec["pm"]))
    c = M.fe_solved(tag, rec["input"])
    sr = _fe_sr(tag, rec["input"])
    frames = dev(rec["input"][..., ::-1])[None]
    out, orig, enh = pipeline.gpen_face_enhancement(detector, gpen, parsenet, sr, frames, return_faces=True)
    out = out[0].flip(-1).cpu().numpy()
    Ho, Wo = rec["out"].shape[:2]
    img_sr = pipeline.gpen_super_resolve(sr, frames)[0].flip(-1).cpu().numpy()
    stats = M.check_u8(img_sr[None], c["u"], c["e32"])
    assert _conditioned(*stats)
    assert np.array_equal(ops.cv_resize_linear(frames, (Wo, Ho))[0].flip(-1).cpu().numpy(), rec["frame"])
    mout, morig, fm, pre, flags, faces, masks = PM.model_outputs(rec)
    assert np.array_equal(mout, rec["out"])
    outside = fm == 0
    assert outside.any() and (~outside).any() and np.array_equal(out[outside], img_sr[outside])
    sr_loose = (~M.strict_pixels(c["u"][0], c["e32"])).any(-1)
    paste_loose = ~PM.strict_pixels(rec["base"], faces, masks, rec["T"], flags)
    differs = (out != rec["out"]).any(-1)
    allowed = int((sr_loose | paste_loose).sum()) + int(2e-3 * Ho * Wo)
    print(f"{tag}: {int(differs.sum())} of {Ho * Wo} pixels leave the reference's result; {int(sr_loose.sum())} are not strict in img_sr, "
          f"{int(paste_loose.sum())} in the paste, allowed {allowed}; largest difference {int(np.abs(out.astype(int) - rec['out'].astype(int)).max())}")
    record_parity(f"gpen_sr.process_pixels_off.{tag}", int(differs.sum()), allowed)
    assert int(differs.sum()) <= allowed
    kept = (flags & 1) == 0
    assert len(orig[0]) == int(kept.sum()) == len(rec["orig"])
    assert (orig[0].flip(-1).cpu().numpy() != rec["orig"]).mean() < 2e-3
    assert np.array_equal(enh[0].flip(-1).cpu().numpy(), rec["ef"][kept])


def test_aligned_branch_against_the_reference_process(golden, monkeypatch):
    ef = golden["fe.aligned.ef"]
    detector, gpen, parsenet = TP._nets()
    monkeypatch.setattr(pipeline, "gpen_enhance", lambda weights, faces: dev(ef[..., ::-1])[None])
    c = M.fe_solved("fe.aligned", ef)
    out = pipeline.gpen_face_enhancement(None, gpen, None, _fe_sr("fe.aligned", ef), torch.zeros((1, 32, 32, 3), dtype=torch.uint8, device=DEV), aligned=True)
    out = out.flip(-1).cpu().numpy()
    assert _conditioned(*M.check_u8(out, c["u"], c["e32"]))
    assert np.abs(out[0].astype(int) - golden["fe.aligned.out"].astype(int)).max() <= 1
