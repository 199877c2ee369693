"""Row f15 on the device: csrc/gpen_paste.hip through ``ops.gpen_*`` and ``pipeline.gpen_enhance_frames`` against tests/gpen_paste_model.py on the cases of
g26_gpen_paste.npz (small sizes, so that each test takes seconds) and once at the production sizes.

The bars.  Transforms: 1e-12 relative to the matrix's largest entry (float64 both sides; the sums differ in order by a few ulp).  uint8 sampling (warp-crop,
smooth): bit-equal — integer arithmetic on identical fixed-point coordinates.  Feather: 2^-23 absolute on masks in [0, 1] — float64 accumulation on both sides
leaves the final rounding to float32, half an ulp below 1 being 2^-25, and a last-bit disagreement of the float64 sums moves the rounded value by at most one
float32 ulp, 2^-23 at 1.  Paste, given the device's own masks and transforms: ``full_mask`` within 8 * 2^-24; the image exact on strict pixels (tests/
gpen_paste_model.py: strict_pixels) and within 1 elsewhere, at most 1 % of a case's pixels not strict."""
import os

import numpy as np
import pytest
import torch

import gpen_model as GM
import gpen_paste_model as PM
import parsenet_model as PNM
import retinaface_model as RM
from conftest import GOLDEN, record_parity
from e4s2024_amd import graphs, ops, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NETS = {}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "g26_gpen_paste.npz")) as z:
        return {k: z[k] for k in z.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _offset(t):
    """A copy of ``t`` that starts one byte past an aligned address: the kernels' byte-wise form."""
    flat = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    return view


def _device_case(rec, T=None):
    """The individual ops on a stored case with the stored matrices: (crops of all faces, smoothed faces, feathered masks, T, flags, frame_of_face, face_begin)."""
    S, H, W, k, sigma, thres, small = PM.config(rec)
    n = len(rec["dets"])
    T = dev(rec["T"] if T is None else T)
    fl = dev(PM.flags_of(rec["dets"], 0.9, small))
    fof = torch.zeros(n, dtype=torch.int32, device=DEV)
    crops = ops.gpen_warp_crop(dev(rec["frame"])[None], fof, T, S)
    faces = ops.gpen_smooth_small(dev(rec["ef"]), fl)
    masks = ops.gpen_mask_feather(dev(rec["pm"]), k, sigma, thres)
    return crops, faces, masks, T, fl, fof, torch.tensor([0, n], dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ transforms
def test_transforms_against_the_model(golden):
    sets = golden["sets.landms"]
    n = len(sets)
    dets = np.tile(np.array([[10, 20, 210, 260, 0.99]], np.float32), (n, 1))
    T, flags = ops.gpen_face_transforms(dev(dets), dev(sets), golden["ref.512"])
    Tm, fm = PM.transforms(dets, sets, golden["ref.512"], 0.9, 100)
    assert T.dtype == torch.float64 and tuple(T.shape) == (n, 2, 2, 3) and flags.dtype == torch.int32
    got = T.cpu().numpy()
    rel = max(np.abs(got[i, j] - Tm[i, j]).max() / np.abs(Tm[i, j]).max() for i in range(n) for j in range(2))
    record_parity("gpen_paste.transforms_rel", rel, 1e-12)
    assert rel <= 1e-12 and np.array_equal(flags.cpu().numpy(), fm)
    with pytest.raises(ValueError, match=r"ref_points.*\(5, 3\)"):
        ops.gpen_face_transforms(dev(dets), dev(sets), np.zeros((5, 3)))


def test_flags_at_their_edges():
    t, lim = np.float32(0.9), np.float32(100)
    below = np.nextafter(t, np.float32(0))
    dets = np.array([[0, 0, 100, 150, t],                       # the score exactly at the threshold: kept; a side exactly at the limit: not small
                     [0, 0, 150, np.nextafter(lim, np.float32(0)), 0.95],          # a height just below the limit: small
                     [0, 0, 99, 150, below],                    # just below the threshold: skipped; width 99: small
                     [5.5, 0.25, 105.5, 200.25, 1.0],           # 100 after a float32 subtraction
                     [0, 0, 300, 300, 0.99], [0, 0, 300, 300, 0.99], [0, 0, 300, 300, np.nan]], np.float32)
    landms = np.tile(PM.reference_points(64).T.reshape(1, 10).astype(np.float32), (len(dets), 1))
    landms[4] = 7.0                                             # the landmarks coincide
    landms[5, 3] = np.inf
    T, flags = ops.gpen_face_transforms(dev(dets), dev(landms), PM.reference_points(64))
    Tm, fm = PM.transforms(dets, landms, PM.reference_points(64), 0.9, 100)
    assert fm.tolist() == [0, 2, 3, 0, 1, 1, 0] and flags.cpu().tolist() == fm.tolist()
    assert not T[4:6].any() and np.abs(T[6].cpu().numpy() - Tm[6]).max() <= 1e-12
    e = ops.gpen_face_transforms(torch.zeros(0, 5, device=DEV), torch.zeros(0, 10, device=DEV), PM.reference_points(64))
    assert tuple(e[0].shape) == (0, 2, 2, 3) and tuple(e[1].shape) == (0,)


# ------------------------------------------------------------------------------------------------ uint8 sampling
@pytest.mark.parametrize("tag", ["A", "B"])
def test_warp_crop_and_smooth_are_bit_equal(tag, golden):
    rec = PM.load_case(golden, tag)
    S, H, W, k, sigma, thres, small = PM.config(rec)
    out, orig, fm, pre, flags, faces_m, masks_m = PM.model_outputs(rec)
    crops, faces, masks, T, fl, fof, fb = _device_case(rec)
    kept = [i for i in range(len(flags)) if not flags[i] & PM.FACE_SKIP]
    assert np.array_equal(crops[kept].cpu().numpy(), orig) and np.array_equal(crops[kept].cpu().numpy(), rec["orig"])
    assert np.array_equal(faces.cpu().numpy(), faces_m)
    # pointers one byte past alignment (the byte-wise loads) and a size whose rows are not dword aligned (the byte-wise stores, a ragged last quadruple)
    frames_o, ef_o = _offset(dev(rec["frame"])[None]), _offset(dev(rec["ef"]))
    assert torch.equal(ops.gpen_warp_crop(frames_o, fof, T, S), crops) and torch.equal(ops.gpen_smooth_small(ef_o, fl), faces)
    for size in (S - 3, S + 1):
        got = ops.gpen_warp_crop(frames_o, fof, T, size).cpu().numpy()
        assert all(np.array_equal(got[i], PM.warp_affine(rec["frame"], rec["T"][i, 0], (size, size))) for i in kept)
    odd = np.random.default_rng(3).integers(0, 256, (3, 13, 13, 3)).astype(np.uint8)
    got = ops.gpen_smooth_small(dev(odd), torch.tensor([2, 0, 3], dtype=torch.int32, device=DEV)).cpu().numpy()
    assert np.array_equal(got[0], PM.filter2d_smooth(odd[0])) and np.array_equal(got[1], odd[1]) and np.array_equal(got[2], PM.filter2d_smooth(odd[2]))
    one = ops.gpen_smooth_small(dev(odd[:1, :1, :1]), torch.tensor([2], dtype=torch.int32, device=DEV))
    assert np.array_equal(one.cpu().numpy(), odd[:1, :1, :1])           # a 1 x 1 face reflects onto itself


def test_a_face_outside_the_frame_and_a_batch_of_frames(golden):
    rec = PM.load_case(golden, "A")
    S = PM.config(rec)[0]
    frames = np.stack([rec["frame"], rec["frame"][::-1, ::-1].copy()])
    far = rec["landms"][:1].copy()
    far[0, :5] -= 500
    landms = np.concatenate([rec["landms"], far, rec["landms"][:1]])
    dets = np.concatenate([rec["dets"], rec["dets"][:2]])
    T, flags = ops.gpen_face_transforms(dev(dets), dev(landms), PM.reference_points(S))
    fof = torch.tensor([0, 1, 0, 1, 7], dtype=torch.int32, device=DEV)          # the last names no frame of the batch
    crops = ops.gpen_warp_crop(dev(frames), fof, T, S).cpu().numpy()
    Tn = T.cpu().numpy()
    for i, b in enumerate([0, 1, 0]):
        assert np.array_equal(crops[i], PM.warp_affine(frames[b], Tn[i, 0], (S, S))) and crops[i].any()
    assert not crops[3].any() and not crops[4].any()
    assert tuple(ops.gpen_warp_crop(dev(frames), fof[:0], T[:0], S).shape) == (0, S, S, 3)


# ------------------------------------------------------------------------------------------------ feather
@pytest.mark.parametrize("tag", ["A", "B"])
def test_feather_against_the_model(tag, golden):
    rec = PM.load_case(golden, tag)
    S, H, W, k, sigma, thres, small = PM.config(rec)
    pm = np.concatenate([rec["pm"], np.full((1, S, S), 255, np.uint8), np.zeros((1, S, S), np.uint8)])
    want = np.array([PM.feather(m, thres, k, sigma) for m in pm])
    got = ops.gpen_mask_feather(dev(pm), k, sigma, thres).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    record_parity(f"gpen_paste.feather_abs.{tag}", err, 2.0 ** -23)
    assert got.dtype == np.float32 and err <= 2.0 ** -23
    assert (got[want == 0] == 0).all() and (want == 0).any() and not got[-1].any()
    assert abs(float(got[-2][S // 2, S // 2]) - 1) <= 2.0 ** -23 and got[-2][0, 0] < 0.5
    assert torch.equal(ops.gpen_mask_feather(_offset(dev(pm)), k, sigma, thres), dev(got))
    assert tuple(ops.gpen_mask_feather(dev(pm[:0]), k, sigma, thres).shape) == (0, S, S)


def test_feather_where_the_taps_span_the_mask():
    """k // 2 = S - 1, the widest reflection; a mask narrower than a tile; thres beyond the middle zeroes everything."""
    pm = (np.random.default_rng(5).random((2, 7, 7)) < 0.7).astype(np.uint8) * np.uint8(255)
    want = np.array([PM.feather(m, 1, 13, 2.5) for m in pm])
    got = ops.gpen_mask_feather(dev(pm), 13, 2.5, 1).cpu().numpy()
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 and want.max() > 0.3
    assert not ops.gpen_mask_feather(dev(pm), 3, 1.0, 4).any()


# ------------------------------------------------------------------------------------------------ paste
def _paste_check(name, base, faces, masks, T, flags, out, full_mask, rows=None, max_loose=0.01):
    """The device's ``out`` / ``full_mask`` against the model fed with the same faces, masks and transforms."""
    want, fm, pre, _ = PM.paste(base, faces, masks, T, flags, rows)
    strict = PM.strict_pixels(base, faces, masks, T, flags, rows=rows)
    if rows is not None:
        out, full_mask = out[rows[0]:rows[1]], full_mask[rows[0]:rows[1]]
    err = float(np.abs(full_mask.astype(np.float64) - fm).max())
    diff = np.abs(out.astype(np.int32) - want.astype(np.int32)).max(-1)
    loose = 1 - float(strict.mean())
    record_parity(f"gpen_paste.full_mask_abs.{name}", err, 8 * 2.0 ** -24)
    print(f"paste {name}: full_mask err {err:.3e}, non-strict pixels {loose:.4f}, differing pixels {int((diff != 0).sum())}, max diff {int(diff.max())}")
    assert err <= 8 * 2.0 ** -24
    assert (diff[strict] == 0).all() and diff.max() <= 1 and loose <= max_loose


@pytest.mark.parametrize("tag", ["A", "B", "C", "D", "E"])
def test_paste_against_the_model(tag, golden):
    rec = PM.load_case(golden, tag)
    S, H, W, k, sigma, thres, small = PM.config(rec)
    base = rec["base"] if "base" in rec else rec["frame"]
    T, flags = ops.gpen_face_transforms(dev(rec["dets"]), dev(rec["landms"]), golden[f"ref.{S}"], 0.9, small)         # the device's own transforms
    crops, faces, masks, _, fl, fof, fb = _device_case(rec, T.cpu().numpy())
    assert torch.equal(fl, flags)
    out, full_mask = ops.gpen_paste(dev(base)[None], faces, masks, T, flags, fb, return_mask=True)
    assert tuple(out.shape) == (1, H, W, 3) and tuple(full_mask.shape) == (1, H, W)
    # E is the tie (every pixel both faces reach is non-strict by construction); the tie is exact on the device too: same inputs, same sample
    _paste_check(tag, base, faces.cpu().numpy(), masks.cpu().numpy(), T.cpu().numpy(), flags.cpu().numpy(), out[0].cpu().numpy(), full_mask[0].cpu().numpy(),
                 max_loose=1.0 if tag == "E" else 0.01)
    if tag == "E":
        want = PM.paste(base, faces.cpu().numpy(), masks.cpu().numpy(), T.cpu().numpy(), flags.cpu().numpy())[0]
        assert np.array_equal(out[0].cpu().numpy(), want)
    if tag == "D":
        assert np.array_equal(out[0].cpu().numpy(), base) and not full_mask.any()
    # in place (out is base), and an output one byte past alignment: the same bits
    b2 = dev(base)[None].clone()
    assert ops.gpen_paste(b2, faces, masks, T, flags, fb, out=b2) is b2 and torch.equal(b2, out)
    o3 = _offset(torch.zeros_like(out))
    ops.gpen_paste(_offset(dev(base)[None]), faces, masks, T, flags, fb, out=o3)
    assert torch.equal(o3, out)
    with pytest.raises(ValueError, match="overlaps"):
        flat = torch.zeros(out.numel() + 8, dtype=torch.uint8, device=DEV)
        ops.gpen_paste(flat[:out.numel()].view(out.shape), faces, masks, T, flags, fb, out=flat[4:4 + out.numel()].view(out.shape))


def test_paste_batch_graph_and_noncontiguous(golden):
    a, c = PM.load_case(golden, "A"), PM.load_case(golden, "C")
    S, H, W, k, sigma, thres, small = PM.config(a)
    T, flags = ops.gpen_face_transforms(dev(a["dets"]), dev(a["landms"]), golden["ref.32"], 0.9, small)
    _, faces, masks, _, _, _, _ = _device_case(a, T.cpu().numpy())
    # three frames: A's faces over A's frame, none over C's base, the first two of A's in reverse order over the flipped frame
    bases = dev(np.stack([a["frame"], c["base"], a["frame"][::-1].copy()]))
    sel = torch.tensor([0, 1, 2, 1, 0], device=DEV)
    F, M, TT, FL = faces[sel], masks[sel], T[sel], flags[sel]
    fb = torch.tensor([0, 3, 3, 5], dtype=torch.int32, device=DEV)
    out, fm = ops.gpen_paste(bases, F, M, TT, FL, fb, return_mask=True)
    singles = [ops.gpen_paste(bases[b:b + 1], F[lo:hi], M[lo:hi], TT[lo:hi], FL[lo:hi], torch.tensor([0, hi - lo], dtype=torch.int32, device=DEV))
               for b, (lo, hi) in enumerate([(0, 3), (3, 3), (3, 5)])]
    assert torch.equal(out, torch.cat(singles)) and torch.equal(out[1], bases[1]) and not fm[1].any()
    assert torch.equal(ops.gpen_paste(bases, F, M, TT, FL, fb), out)                             # a second run: the same bits
    g = graphs.GraphedCall(lambda *t: ops.gpen_paste(*t), [bases, F, M, TT, FL, fb])
    assert torch.equal(g(bases, F, M, TT, FL, fb), out)
    assert torch.equal(g(bases.flip(0).contiguous(), F, M, TT, FL, fb), ops.gpen_paste(bases.flip(0).contiguous(), F, M, TT, FL, fb))
    # non-contiguous views are accepted (and copied)
    wide = torch.zeros((3, H, W + 5, 3), dtype=torch.uint8, device=DEV)
    wide[:, :, :W] = bases
    assert not wide[:, :, :W].is_contiguous() and torch.equal(ops.gpen_paste(wide[:, :, :W], F, M, TT, FL, fb), out)
    assert torch.equal(ops.gpen_paste(bases, F.flip(0).flip(0), M.transpose(1, 2).contiguous().transpose(1, 2), TT, FL, fb), out)
    # a skipped face is left out; face_begin that reaches past the faces reads none
    FL2 = FL.clone()
    FL2[0] |= ops.GPEN_FACE_SKIP
    assert torch.equal(ops.gpen_paste(bases[:1], F[:3], M[:3], TT[:3], FL2[:3], torch.tensor([0, 3], dtype=torch.int32, device=DEV)),
                       ops.gpen_paste(bases[:1], F[1:3], M[1:3], TT[1:3], FL[1:3], torch.tensor([0, 2], dtype=torch.int32, device=DEV)))
    assert torch.equal(ops.gpen_paste(bases[:1], F[:3], M[:3], TT[:3], FL[:3], torch.tensor([-4, 99], dtype=torch.int32, device=DEV)), out[:1])


# ------------------------------------------------------------------------------------------------ the chain
def _nets():
    """The three networks at the smallest admissible sizes, seeded: GPEN's s32 generator, ParseNet case C (32 -> 32), RetinaFace with 64 output channels."""
    if not _NETS:
        size, narrow, sdim, _ = GM.CASES["s32"]
        g = ops.GPEN(size, sdim, GM.N_MLP, 2, narrow).eval()
        g.load_state_dict(GM.state_dict("s32"), strict=True)
        p = PNM.make_module("C")
        p.load_state_dict(PNM.state_dict("C"), strict=True)
        d = RM.make_module("D")
        d.load_state_dict(RM.state_dict("D"), strict=True)
        _NETS.update(gpen=g.to(DEV), parsenet=p.to(DEV), detector=d.to(DEV))
    return _NETS["detector"], _NETS["gpen"], _NETS["parsenet"]


def _composition(gpen, parsenet, frames, base, per_frame):
    """``gpen_enhance_frames`` written out over the individual ops, from the detections."""
    S, D = 32, ops.GPEN_PASTE_DEFAULTS
    counts = [len(d) for d, _ in per_frame]
    dets, landms = torch.cat([d for d, _ in per_frame]), torch.cat([l for _, l in per_frame])
    fb = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)
    fof = torch.tensor(np.repeat(np.arange(len(counts)), counts), dtype=torch.int32, device=DEV)
    T, flags = ops.gpen_face_transforms(dets, landms, ops.gpen_reference_points(S), D["threshold"], D["small_face"])
    of = ops.gpen_warp_crop(frames, fof, T, S)
    ef = pipeline.gpen_enhance(gpen, of)
    masks = ops.gpen_mask_feather(pipeline.gpen_face_mask(parsenet, ef), D["ksize"], D["sigma"], D["thres"])
    return ops.gpen_paste(base, ops.gpen_smooth_small(ef, flags), masks, T, flags, fb), of, ef, flags


@pytest.mark.parametrize("tag", ["A", "B", "C", "D"])
def test_enhance_frames_on_the_cases(tag, golden, monkeypatch):
    """The chain on the cases' frames and detections (the detector replaced by the recorded detections, the generator and the ParseNet by seeded ones at S 32,
    the smallest pair whose sizes agree — B's S of 48 is no size of the generator, a power of two): bit for bit the composition of the individual ops.  The
    production constants (101 taps) do not fit a 32 x 32 mask, so the chain runs at the cases' own."""
    rec = PM.load_case(golden, tag)
    S, H, W, k, sigma, thres, small = PM.config(rec)
    detector, gpen, parsenet = _nets()
    monkeypatch.setattr(pipeline, "gpen_detect_faces", lambda net, frames, bgr=True: [(dev(rec["dets"]), dev(rec["landms"]))] * frames.shape[0])
    monkeypatch.setitem(ops.GPEN_PASTE_DEFAULTS, "ksize", 9)
    monkeypatch.setitem(ops.GPEN_PASTE_DEFAULTS, "sigma", 1.5)
    monkeypatch.setitem(ops.GPEN_PASTE_DEFAULTS, "thres", 3)
    monkeypatch.setitem(ops.GPEN_PASTE_DEFAULTS, "small_face", small)
    frames = dev(rec["frame"])[None]
    base = dev(rec["base"])[None] if "base" in rec else None
    out, orig, enh = pipeline.gpen_enhance_frames(detector, gpen, parsenet, frames, base, return_faces=True)
    want, of, ef, flags = _composition(gpen, parsenet, frames, frames if base is None else base, [(dev(rec["dets"]), dev(rec["landms"]))])
    kept = (flags & 1) == 0
    assert torch.equal(out, want) and len(orig) == len(enh) == 1 and torch.equal(orig[0], of[kept]) and torch.equal(enh[0], ef[kept])
    assert torch.equal(pipeline.gpen_enhance_frames(detector, gpen, parsenet, frames, base), out)
    if len(flags):
        want_flags = PM.flags_of(rec["dets"], 0.9, small)
        assert flags.cpu().tolist() == want_flags.tolist()
        T = PM.transforms(rec["dets"], rec["landms"], PM.reference_points(32), 0.9, small)[0]
        i = int(np.flatnonzero(want_flags & 1 == 0)[0])
        # (the device's matrix is the model's to 1e-12: a fixed-point coordinate on a rounding edge may fall the other way, a pixel in thousands)
        assert (orig[0][0].cpu().numpy() != PM.warp_affine(rec["frame"], T[i, 0], (32, 32))).mean() < 2e-3
        assert not torch.equal(out, frames if base is None else base)
    else:
        assert torch.equal(out, frames) and tuple(orig[0].shape) == (0, 32, 32, 3)


def test_enhance_frames_with_the_detector(golden, monkeypatch):
    """The whole chain with a seeded detector: a batch equals its single frames, a second run equals the first, a non-contiguous input is accepted."""
    detector, gpen, parsenet = _nets()
    for key, v in (("ksize", 9), ("sigma", 1.5), ("thres", 3)):
        monkeypatch.setitem(ops.GPEN_PASTE_DEFAULTS, key, v)
    a, c = PM.load_case(golden, "A"), PM.load_case(golden, "C")
    frames = dev(np.stack([a["frame"], c["base"]]))
    per_frame = pipeline.gpen_detect_faces(detector, frames, bgr=False)
    print("faces per frame:", [len(d) for d, _ in per_frame])
    out = pipeline.gpen_enhance_frames(detector, gpen, parsenet, frames)
    assert out.dtype == torch.uint8 and out.shape == frames.shape
    assert torch.equal(out, _composition(gpen, parsenet, frames, frames, per_frame)[0])
    singles = torch.cat([pipeline.gpen_enhance_frames(detector, gpen, parsenet, frames[b:b + 1]) for b in range(2)])
    assert torch.equal(out, singles) and torch.equal(pipeline.gpen_enhance_frames(detector, gpen, parsenet, frames), out)
    wide = torch.zeros((2, 80, 100, 3), dtype=torch.uint8, device=DEV)
    wide[:, :, :96] = frames
    assert torch.equal(pipeline.gpen_enhance_frames(detector, gpen, parsenet, wide[:, :, :96]), out)
    with pytest.raises(ValueError, match=r"base_u8 is \(1, 80, 96, 3\)"):
        pipeline.gpen_enhance_frames(detector, gpen, parsenet, frames, frames[:1])
    with pytest.raises(ValueError, match="16 x 16 face into a"):
        size, narrow, sdim, _ = GM.CASES["s16"]
        g16 = ops.GPEN(size, sdim, GM.N_MLP, 2, narrow).eval()
        g16.load_state_dict(GM.state_dict("s16"), strict=True)
        pipeline.gpen_enhance_frames(detector, g16.to(DEV), PNM_B(), frames)


def PNM_B():
    """ParseNet case B: 32 in, 64 out — on a 16 x 16 face its mask is 32 x 32, not the face's size."""
    p = PNM.make_module("B")
    p.load_state_dict(PNM.state_dict("B"), strict=True)
    return p.to(DEV)


def test_align_dropin_equals_the_op(golden):
    import e4s2024_amd
    rec = PM.load_case(golden, "B")
    S = PM.config(rec)[0]
    e4s2024_amd.install()
    try:
        from swap_face_fine.gpen import align_faces as AF
        ref = AF.get_reference_facial_points((S, S), 0.25, (0, 0), True)
        T, _ = ops.gpen_face_transforms(dev(rec["dets"]), dev(rec["landms"]), ref, 0., 0.)
        crops = ops.gpen_warp_crop(dev(rec["frame"])[None], torch.zeros(3, dtype=torch.int32, device=DEV), T, S)
        for i in range(3):
            face, tfm_inv = AF.warp_and_crop_face(rec["frame"], rec["landms"][i].reshape(2, 5), reference_pts=ref, crop_size=(S, S))
            assert face.dtype == np.uint8 and np.array_equal(face, crops[i].cpu().numpy())
            assert tfm_inv.shape == (2, 3) and np.array_equal(tfm_inv, T[i, 1].cpu().numpy())
            face2, _ = AF.warp_and_crop_face(rec["frame"], rec["landms"][i].reshape(2, 5).T, reference_pts=ref.T, crop_size=(S, S))
            assert np.array_equal(face2, face)
        with pytest.raises(AF.FaceWarpException, match="similarity"):
            AF.warp_and_crop_face(rec["frame"], np.full((2, 5), 3.0), reference_pts=ref, crop_size=(S, S))
    finally:
        e4s2024_amd.uninstall()


# ------------------------------------------------------------------------------------------------ the production sizes, once
def test_production_sizes_on_a_band():
    """S 512, 101 taps, a 1024 x 1024 frame, two overlapping faces (one small): crops and masks against the model in full, the paste on a 64-row band."""
    rng = np.random.default_rng(15)
    S, H, W = 512, 1024, 1024
    D = ops.GPEN_PASTE_DEFAULTS
    yy, xx = np.mgrid[0:H, 0:W]
    frame = ((xx // 2 + yy // 3)[..., None] + np.array([0, 60, 140]) + rng.integers(0, 40, (H, W, 3))).astype(np.uint8)
    ref = PM.reference_points(S)
    landms = []
    for cx, cy, s, deg in ((420., 500., 0.9, 10.), (640., 560., 0.17, -20.)):
        a = np.deg2rad(deg)
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        landms.append((s * (ref - S / 2) @ R.T + [cx, cy]).T.reshape(10))
    landms = np.array(landms, np.float32)
    dets = np.array([[200, 250, 640, 750, 0.99], [600, 520, 680, 605, 0.95]], np.float32)
    ys, xs = np.mgrid[0:S, 0:S]
    ef = np.stack([((xs * (2 + i) + ys * (1 + i))[..., None] // 3 * np.array([1, 2, 3]) + rng.integers(0, 64, (S, S, 3))).astype(np.uint8) for i in range(2)])
    pm = []
    for i in range(2):
        blocks = (rng.random((S // 32, S // 32)) < 0.9).astype(np.uint8)
        blocks[7:9, 7:9] = 0
        pm.append(np.kron(blocks, np.ones((32, 32), np.uint8)) * np.uint8(255))
    pm = np.stack(pm)
    T, flags = ops.gpen_face_transforms(dev(dets), dev(landms), ref)
    assert flags.cpu().tolist() == [0, 2]
    Tn = T.cpu().numpy()
    crops = ops.gpen_warp_crop(dev(frame)[None], torch.zeros(2, dtype=torch.int32, device=DEV), T, S).cpu().numpy()
    assert np.array_equal(crops[0], PM.warp_affine(frame, Tn[0, 0], (S, S))) and np.array_equal(crops[1], PM.warp_affine(frame, Tn[1, 0], (S, S)))
    masks = ops.gpen_mask_feather(dev(pm), D["ksize"], D["sigma"], D["thres"])
    err = float(np.abs(masks[0].cpu().numpy().astype(np.float64) - PM.feather(pm[0], D["thres"], D["ksize"], D["sigma"])).max())
    record_parity("gpen_paste.feather_abs.512", err, 2.0 ** -23)
    assert err <= 2.0 ** -23
    faces = ops.gpen_smooth_small(dev(ef), flags)
    assert np.array_equal(faces[1].cpu().numpy(), PM.filter2d_smooth(ef[1])) and np.array_equal(faces[0].cpu().numpy(), ef[0])
    out, fm = ops.gpen_paste(dev(frame)[None], faces, masks, T, flags, torch.tensor([0, 2], dtype=torch.int32, device=DEV), return_mask=True)
    _paste_check("512", frame, faces.cpu().numpy(), masks.cpu().numpy(), Tn, flags.cpu().numpy(), out[0].cpu().numpy(), fm[0].cpu().numpy(), rows=(520, 584))
    band = fm[0, 520:584].cpu().numpy()
    assert band.max() > 0.99 and (band == 0).any()
