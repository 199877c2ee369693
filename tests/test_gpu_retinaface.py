"""Row f14 on the GPU: the kernels of ``csrc/retinaface.hip`` alone, ``ops.retinaface_forward`` against the float64 model ``retinaface_model`` and the
reference's stored outputs (``tests/golden/g25_retinaface.npz``), ``ops.retinaface_detect`` against the reference's stored ``detect`` output, and the
bit-equality properties of the host layer.

Bounds: a case's loc, conf and landms are held to ``max(8 e32, 2e-7 max|want|)`` with ``e32`` the model in float32 against itself in float64 (never the code
under test); decoded coordinates to the bar of the normalised boxes and landmarks times ``max(H, W)``.  ``ARITH = "sb"`` is held to ``SB_TOL = 1e-3`` max-abs,
the bar tests/test_gpu_gpen.py uses for that arithmetic.  The cases meet the admission conditions of ``retinaface_model.admission``, so counts and order must
be the reference's with no exclusion rule."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import retinaface_model as RM
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import ops, ops_retinaface, pipeline
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SB_TOL = 1e-3
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
_NETS = {}


@pytest.fixture(scope="module")
def golden():
    return load_golden("g25_retinaface")


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A fault on the device ends the module: nothing more is launched on a GPU that has reported one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported a fault, stopping: {e}", returncode=3)


def _net(tag):
    """``ops.RetinaFace`` of a case with its seeded weights on the device, made once (a module caches its prepared weights)."""
    if tag not in _NETS:
        net = RM.make_module(tag)
        net.load_state_dict(RM.case(tag)["sd"], strict=True)
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
def _input(img, bgr, out=None):
    bs, H, W, _ = img.shape
    out = torch.full((bs, 3, H, W), float("nan"), device=DEV) if out is None else out
    lib().call("e4s_retina_input", _p(out), _p(img), 1 if bgr else 0, bs, H, W, _stream())
    return out


def test_input_is_exact_on_all_levels_and_in_both_orders():
    levels = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3).copy()
    levels[..., 1] = levels[:, ::-1, :, 1]
    levels[..., 2] = levels[:, :, ::-1, 2]
    ragged = np.random.RandomState(3).randint(0, 256, (2, 5, 7, 3)).astype(np.uint8)          # 35 pixels an image: the one-element form
    for img in (levels, ragged):
        want = T(RM.to_input(img)).to(DEV)
        d = T(img).to(DEV)
        assert torch.equal(_input(d, True), want)
        assert torch.equal(_input(d.flip(3).contiguous(), False), want)                       # RGB of the flipped image
        assert torch.equal(_input(_offset(d), True), want)
        assert torch.equal(_input(d, True, out=_offset(torch.empty_like(want))), want)
    out = _input(T(levels).to(DEV), True)
    assert float(out.min()) == -123.0 and float(out.max()) == 151.0                            # level 0 minus the largest mean, level 255 minus the smallest
    _input(T(levels[:0]).to(DEV), True, out=torch.empty((0, 3, 16, 16), device=DEV))            # an empty batch returns at once


def _up_add(a, b, out=None):
    planes, h, w = a.shape
    out = torch.full_like(a, float("nan")) if out is None else out
    lib().call("e4s_retina_up_add", _p(out), _p(a), _p(b), planes, h, w, b.shape[1], b.shape[2], _stream())
    return out


@pytest.mark.parametrize("big,small", [((13, 7), (7, 4)), ((7, 12), (4, 6)), ((2, 2), (1, 1)), ((6, 8), (6, 8)), ((9, 16), (5, 8)), ((40, 40), (20, 20))])
def test_up_add_is_bit_equal_to_pytorch(big, small):
    g = torch.Generator(device="cpu").manual_seed(big[0] * 100 + big[1])
    a, b = torch.randn(5, *big, generator=g).to(DEV), torch.randn(5, *small, generator=g).to(DEV)
    want = a + F.interpolate(b[None], size=list(big), mode="nearest")[0]
    assert torch.equal(_up_add(a, b), want)
    assert torch.equal(_up_add(_offset(a), _offset(b)), want)
    assert torch.equal(_up_add(a, b, out=_offset(torch.empty_like(a))), want)
    # the float64 model's index rule is the same one
    assert torch.equal(RM._nearest(b.cpu()[None], big, None)[0] + a.cpu(), want.cpu())
    _up_add(a[:0], b[:0])                                                                     # no planes: returns at once


@pytest.mark.parametrize("bs,c,hw", [(2, 64, 35), (1, 16, 64), (3, 8, 1)])
def test_cat_relu(bs, c, hw):
    g = torch.Generator(device="cpu").manual_seed(c + hw)
    a, b, d = (torch.randn(bs, n, hw, generator=g).to(DEV) for n in (c // 2, c // 4, c // 4))
    want = F.relu(torch.cat([a, b, d], dim=1))

    def run(a, b, d, out=None):
        out = torch.full((bs, c, hw), float("nan"), device=DEV) if out is None else out
        lib().call("e4s_retina_cat_relu", _p(out), _p(a), _p(b), _p(d), bs, c // 2, c // 4, c // 4, hw, _stream())
        return out

    assert torch.equal(run(a, b, d), want)
    assert torch.equal(run(_offset(a), b, _offset(d)), want)
    assert torch.equal(run(a, b, d, out=_offset(torch.empty_like(want))), want)


def _seeded_heads(bs, H, W, seed):
    """Head maps with the statistics the seeded network gives: loc and landmarks of order 1, class logits with a difference of a few units."""
    rs = np.random.RandomState(seed)
    heads = []
    for h, w in RM.level_sizes(H, W):
        m = rs.standard_normal((bs, 32, h, w))
        m[:, 8:12] *= 2.5
        heads.append(m.astype(np.float32))
    return heads


def _anchor_major(heads, lo, hi, n):
    """The reference's layout of a head family, float64: channels lo..hi of every level as [bs, N, n]."""
    return np.concatenate([h[:, lo:hi].astype(np.float64).transpose(0, 2, 3, 1).reshape(h.shape[0], -1, n) for h in heads], 1)


def _decode(heads, H, W, offset=False):
    bs = heads[0].shape[0]
    N = ops.retinaface_level_sizes(H, W)[1]
    outs = [torch.full(s, float("nan"), device=DEV) for s in ((bs, N, 4), (bs, N, 2), (bs, N, 10), (bs, N), (bs, N, 4), (bs, N, 10))]
    if offset:
        outs = [_offset(t) for t in outs]
    lib().call("e4s_retina_decode", *[_p(t) for t in outs], *[_p(h) for h in heads], bs, H, W, _stream())
    return outs


@pytest.mark.parametrize("bs,H,W", [(2, 50, 91), (1, 64, 64), (1, 33, 100)])
def test_decode_against_float64_and_its_forms(bs, H, W, golden):
    heads = _seeded_heads(bs, H, W, H + W)
    dh = [T(h).to(DEV) for h in heads]
    pri = ops.retinaface_priors(H, W, DEV)
    assert np.array_equal(pri.cpu().numpy(), RM.priors(H, W))                                  # PriorBox.forward(), bit for bit
    loc, conf, lm, score, boxes, lmk = _decode(dh, H, W)
    loc64, cls64, lm64 = _anchor_major(heads, 0, 8, 4), _anchor_major(heads, 8, 12, 2), _anchor_major(heads, 12, 32, 10)
    conf64 = torch.softmax(T(cls64), -1).numpy()
    assert np.array_equal(loc.cpu().numpy(), loc64.astype(np.float32)) and np.array_equal(lm.cpu().numpy(), lm64.astype(np.float32))      # copies in anchor order
    # bars from the float32 restatement against the float64 one, never from the kernel
    conf32 = torch.softmax(T(cls64.astype(np.float32)), -1).numpy()
    bar_conf = RM.bound(RM.max_err(conf32, conf64), conf64)
    err_conf = RM.max_err(conf.cpu().numpy(), conf64)
    record_parity(f"retinaface.decode.{H}x{W}.conf", err_conf, bar_conf)
    assert err_conf <= bar_conf
    assert torch.equal(score, conf[:, :, 1])
    band = 0
    for b in range(bs):
        b64, l64 = RM.decode_all(loc64[b], lm64[b], H, W)
        b32, l32 = RM.decode_all(loc64[b].astype(np.float32), lm64[b].astype(np.float32), H, W, dtype=np.float32)
        e32 = max(RM.max_err(b32, b64), RM.max_err(l32, l64))
        bar = RM.bound(e32, max(np.abs(b64).max(), np.abs(l64).max())) * max(H, W)
        err = max(RM.max_err(boxes[b].cpu().numpy(), b64 * np.array([W, H, W, H])), RM.max_err(lmk[b].cpu().numpy(), l64 * np.array([W, H] * 5)))
        record_parity(f"retinaface.decode.{H}x{W}.{b}.xy", err, bar)
        assert err <= bar
        # the candidate set: equal on every anchor outside twice the score bar around the threshold, and few anchors inside
        keys, counts = _compact(score[b:b + 1], RM.CONF_T, 5000)
        got = np.zeros(score.shape[1], dtype=bool)
        n = int(counts[0, 1])
        got[(0xFFFFFFFF - (keys[0, :n].cpu().numpy() & 0xFFFFFFFF)).astype(np.int64)] = True
        clear = np.abs(conf64[b, :, 1] - RM.CONF_T) > 2 * bar_conf
        band = max(band, 1.0 - clear.mean())
        assert np.array_equal(got[clear], (conf64[b, :, 1] > RM.CONF_T)[clear]) and int(counts[0, 0]) == n == int(got.sum())
        idx = 0xFFFFFFFF - (keys[0, :n].cpu().numpy() & 0xFFFFFFFF)
        assert np.all(np.diff(idx) > 0)                                                       # anchor order: deterministic
    record_parity(f"retinaface.decode.{H}x{W}.threshold_band_share", band, 0.01)
    assert band <= 0.01
    for got, want in zip(_decode([_offset(h) for h in dh], H, W, offset=True), (loc, conf, lm, score, boxes, lmk)):
        assert torch.equal(got, want)                                                          # the one-element form: the same bits


def _compact(score, thr, cap):
    bs, N = score.shape
    keys = torch.full((bs, cap), 7, dtype=torch.int64, device=DEV)
    counts = torch.full((bs, 2), -1, dtype=torch.int32, device=DEV)
    lib().call("e4s_retina_compact", _p(keys), _p(counts), _p(score.contiguous()), bs, N, cap, float(thr), _stream())
    return keys, counts


TIE = np.float32(0.95)
TIED = np.arange(900, 2900, 50)                  # forty anchors with one score, in the first, second and third round of 1024 anchors
TOP = np.array([10, 1030, 2050, 2999, 5])        # five anchors with the highest score there is


def test_compact_overflow_and_empty():
    """Beyond the capacity the highest scores survive and equal scores at the cut go to the lower anchors.  Image 1 holds forty anchors at 0.95 (above the
    threshold) spread over three rounds of the compaction, and the capacities are chosen from the INPUT so that the cut falls on the first, inside and on the
    last of them; image 0 holds five anchors at 1.0, cut at 1 and 3."""
    rs = np.random.RandomState(5)
    s = rs.uniform(0.5, 1.0, (2, 3000)).astype(np.float32)
    s[0][s[0] >= 1.0] = np.float32(0.75)
    s[0, TOP] = np.float32(1.0)
    s[1][s[1] == TIE] = np.float32(0.75)
    s[1, TIED] = TIE
    hi = int((s[1] > TIE).sum())                                                               # anchors of image 1 that beat the tied forty
    assert hi > 64 and int((s[1] > np.float32(0.9)).sum()) > hi + 40 and int((s[0] > np.float32(0.9)).sum()) > hi + 40
    sd = T(s).to(DEV)
    for cap in (5000, hi + 41, hi + 40, hi + 39, hi + 23, hi + 17, hi + 1, hi, 64, 3, 1):
        keys, counts = _compact(sd, 0.9, cap)
        for b in range(2):
            above = np.where(s[b] > np.float32(0.9))[0]
            order = above[np.lexsort((above, -s[b][above].astype(np.float64)))][:cap]        # score descending, equal scores by anchor
            n = int(counts[b, 1])
            assert int(counts[b, 0]) == len(above) and n == min(len(above), cap)
            k = keys[b].cpu().numpy()
            idx = (0xFFFFFFFF - (k[:n] & 0xFFFFFFFF)).astype(np.int64)
            assert np.array_equal(np.sort(idx), np.sort(order)) and np.all(np.diff(idx) > 0) and np.all(k[n:] == -1), (cap, b)
            assert np.array_equal((k[:n] >> 32).astype(np.uint32).view(np.float32), s[b][idx])
        # said once more without the sort: of the tied anchors exactly the lowest survive, as many as the capacity leaves room for
        idx1 = 0xFFFFFFFF - (keys[1, :int(counts[1, 1])].cpu().numpy() & 0xFFFFFFFF)
        assert np.array_equal(np.intersect1d(idx1, TIED), TIED[:min(max(cap - hi, 0), 40)]), cap
        idx0 = 0xFFFFFFFF - (keys[0, :int(counts[0, 1])].cpu().numpy() & 0xFFFFFFFF)
        assert np.array_equal(np.intersect1d(idx0, TOP), np.sort(TOP)[:min(cap, 5)]), cap
    keys, counts = _compact(sd, 1.0, 64)                                                       # nothing above the threshold
    assert counts.cpu().tolist() == [[0, 0], [0, 0]] and bool((keys == -1).all())
    dets, lm, keep, nkeep, _ = ops.retinaface_detection_tail(sd, torch.zeros(2, 3000, 4, device=DEV), torch.zeros(2, 3000, 10, device=DEV), confidence_threshold=1.0)
    assert nkeep.cpu().tolist() == [0, 0] and dets.shape == (2, 750, 5) and float(dets.abs().max()) == 0.0


def test_nms_equals_the_reference_keep_lists(golden):
    for name, (_, thresh) in RM.NMS_SETS.items():
        boxes, scores = golden[name + ".boxes"], golden[name + ".scores"]
        n = len(boxes)
        shuffle = np.random.RandomState(n).permutation(n)                                      # anchors in any order: the sort puts them back
        lm = np.arange(n * 10, dtype=np.float32).reshape(n, 10)
        args = [T(a[shuffle][None]).to(DEV) for a in (scores, boxes, lm)]
        want = golden[name + ".keep"]
        for keep_top_k in (750, 10):
            dets, lms, keep, nkeep, counts = ops.retinaface_detection_tail(*args, confidence_threshold=0.0, nms_threshold=thresh, top_k=max(n, 1), keep_top_k=keep_top_k)
            k = int(nkeep[0])
            cut = want[:keep_top_k]
            assert counts.cpu().tolist() == [[n, n]] and k == len(cut) and np.array_equal(keep[0, :k].cpu().numpy(), cut), name
            assert np.array_equal(dets[0, :k, :4].cpu().numpy(), boxes[cut]) and np.array_equal(dets[0, :k, 4].cpu().numpy(), scores[cut])
            assert np.array_equal(lms[0, :k].cpu().numpy(), lm[cut].reshape(-1, 5, 2).transpose(0, 2, 1).reshape(-1, 10))      # (x0..x4, y0..y4)
            assert float(dets[0, k:].abs().max() if k < keep_top_k else 0.0) == 0.0
    one = [T(a[:1][None]).to(DEV) for a in (golden["nms.0.scores"], golden["nms.0.boxes"], np.zeros((1, 10), dtype=np.float32))]
    assert ops.retinaface_detection_tail(*one, confidence_threshold=0.0, top_k=1)[3].cpu().tolist() == [1]                              # one candidate


# ------------------------------------------------------------------------------------------------ the whole path
@pytest.mark.parametrize("tag", list(RM.CASES))
def test_forward_against_the_model_and_the_reference(tag, golden):
    c = RM.case(tag)
    got = [t.cpu().numpy() for t in ops.retinaface_forward(T(c["x"]).to(DEV), _net(tag))]
    for g, n in zip(got, ("loc", "conf", "landms")):
        err, ref = RM.max_err(g, c[n + "64"]), RM.max_err(g, golden[f"{tag}.{n}"])
        print(f"{tag}.{n}: against float64 {err:.3e} = {err / c['e32_' + n]:.2f} e32 (bar {c['bar_' + n]:.3e}), against the reference {ref:.3e}")
        record_parity(f"retinaface.{tag}.{n}.err_over_e32", err / c["e32_" + n], RM.MARGIN)
        record_parity(f"retinaface.{tag}.{n}.maxabs", err, c["bar_" + n])
        record_parity(f"retinaface.{tag}.{n}.maxabs_reference", ref, c["bar_" + n])
        assert g.shape == c[n + "64"].shape and err <= c["bar_" + n]
        assert ref <= c["bar_" + n]                    # the same bound against the reference's own float32 output


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_detect_against_the_reference(tag, golden):
    c = RM.case(tag)
    img, net = T(c["img"]).to(DEV), _net(tag)
    out = ops.retinaface_detect(img, net)
    assert len(out) == img.shape[0]
    for b, (dets, lm) in enumerate(out):
        ref = (golden[f"{tag}.{b}.dets"], golden[f"{tag}.{b}.landms"])
        assert dets.is_cuda and dets.dtype == torch.float32 and dets.shape == ref[0].shape and lm.shape == ref[1].shape      # the same count
        dist = RM.detect_distance((dets.cpu().numpy(), lm.cpu().numpy()), ref, c["bar_xy"], c["bar_conf"])
        d64 = c["det"][b]
        dist64 = RM.detect_distance((dets.cpu().numpy(), lm.cpu().numpy()), (d64["dets"], d64["landms"]), c["bar_xy"], c["bar_conf"])
        print(f"{tag}.{b}: {len(dets)} detections; {dist64:.3f} bars from the float64 model, {dist:.3f} bars from the reference")
        record_parity(f"retinaface.{tag}.{b}.detect.bars", dist64, 1.0, note=f"{len(dets)} detections of {len(d64['cand'])} candidates")
        record_parity(f"retinaface.{tag}.{b}.detect.bars_reference", dist, 1.0)
        assert dist64 <= 1.0 and dist <= 1.0                                                   # same order: row i is the reference's row i
    # image i of a batch == the single-image call, bit for bit; BGR of an image == RGB of its flip; the pipeline entry
    for b, (dets, lm) in enumerate(out):
        one = ops.retinaface_detect(img[b:b + 1], net)[0]
        assert torch.equal(one[0], dets) and torch.equal(one[1], lm)
    rgb = pipeline.gpen_detect_faces(net, img.flip(3).contiguous(), bgr=False)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(rgb, out))


def test_forward_batch_graph_and_dropins_are_bit_equal():
    tag = "B"
    c = RM.case(tag)
    x, img, net = T(c["x"]).to(DEV), T(c["img"]).to(DEV), _net(tag)
    eager = ops.retinaface_forward(x, net)
    assert all(t.is_contiguous() for t in eager)
    for b in range(x.shape[0]):                                                               # a batch against its single samples
        assert all(torch.equal(s[0], e[b]) for s, e in zip(ops.retinaface_forward(x[b:b + 1], net), eager))
    sd = {k: v.to(DEV) for k, v in c["sd"].items()}
    assert all(torch.equal(a, b) for a, b in zip(ops.retinaface_forward(x, {"module." + k: v for k, v in sd.items()}), eager))      # a checkpoint mapping
    empty = ops.retinaface_forward(x[:0], net)
    assert empty[0].shape == (0, c["N"], 4) and empty[2].shape == (0, c["N"], 10)
    eager_det = ops.retinaface_detect_padded(img, net)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.retinaface_forward(x, net)
        ops.retinaface_detect_padded(img, net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fwd = ops.retinaface_forward(x, net)
        det = ops.retinaface_detect_padded(img, net)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(fwd, eager)) and all(torch.equal(a, b) for a, b in zip(det, eager_det))
    # the drop-ins: the network class and the detector class give the ops' bits
    install_dropin()
    from swap_face_fine.gpen.face_detect.facemodels.retinaface import RetinaFace
    from swap_face_fine.gpen.face_detect.retinaface_detection import RetinaFaceDetection
    full = RetinaFace(cfg=dict(ops.RETINAFACE_CFG_RE50), phase="test").eval()
    full.load_state_dict(c["sd"], strict=True)
    full = full.to(DEV)
    assert all(torch.equal(a, b) for a, b in zip(full(x), eager))
    det = object.__new__(RetinaFaceDetection)
    det.net, det.device, det.cfg = full, DEV, dict(ops.RETINAFACE_CFG_RE50)
    want = ops.retinaface_detect(img[1:2], net)[0]
    dets, lm = det.detect(c["img"][1])
    assert isinstance(dets, np.ndarray) and np.array_equal(dets, want[0].cpu().numpy()) and np.array_equal(lm, want[1].cpu().numpy())


@pytest.mark.parametrize("tag", ["A", "D"])
def test_forward_sb_meets_its_bar(tag):
    c = RM.case(tag)
    net = RM.make_module(tag)                                                                 # a module of its own: the prepared weights follow ARITH
    net.load_state_dict(c["sd"], strict=True)
    net = net.to(DEV)
    ops_retinaface.ARITH = "sb"
    try:
        got = [t.cpu().numpy() for t in ops.retinaface_forward(T(c["x"]).to(DEV), net)]
    finally:
        ops_retinaface.ARITH = "sb3"
    for g, n in zip(got, ("loc", "conf", "landms")):
        err = RM.max_err(g, c[n + "64"])
        record_parity(f"retinaface.sb.{tag}.{n}.maxabs", err, SB_TOL, note=f"{err / c['e32_' + n]:.1f} e32")
        assert err <= SB_TOL
    ops_retinaface.ARITH = "bf16"
    try:
        with pytest.raises(ValueError, match="ARITH"):
            ops.retinaface_forward(T(c["x"]).to(DEV), net)
    finally:
        ops_retinaface.ARITH = "sb3"


def test_prepared_weights_follow_the_parameters():
    c = RM.case("D")
    x = T(c["x"]).to(DEV)
    net = RM.make_module("D")
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.retinaface_forward(x, net.to(DEV))
    net.load_state_dict(c["sd"], strict=True)
    net = net.to(DEV)
    before = ops.retinaface_forward(x, net)[0]
    with torch.no_grad():
        for h in net.BboxHead:
            h.conv1x1.bias.add_(0.25)                                                          # in place: the same storage, a new version
    after = ops.retinaface_forward(x, net)[0]
    assert np.abs((after - before).cpu().numpy() - 0.25).max() <= 1e-5
    assert ops.invalidate_weight_caches(net) >= 1
    assert torch.equal(ops.retinaface_forward(x, net)[0], after)
