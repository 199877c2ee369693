"""Generate g26_gpen_paste.npz: what the reference's own code gives for the steps of ``FaceEnhancement.process`` between its networks.

    python tests/golden/make_golden_gpen_paste.py [out.npz]

Only the build container has the reference tree.  cv2 and skimage are installed nowhere, so (no reference source is copied):
  * ``swap_face_fine/gpen/align_faces.py`` is loaded from where it lies with ``cv2`` a stub whose ``warpAffine`` records its matrix and ``skimage.transform`` an
    empty module (the file imports it and never uses it).  Its ``get_reference_facial_points``, ``_umeyama`` and the matrix pair of ``warp_and_crop_face`` are
    pure numpy: ``ref.<S>`` and, per landmark set, ``tfm`` / ``tfm_inv``;
  * cases A - D are the issue's; E adds a tie (one geometry and one mask twice) that separates ``>`` from ``>=`` and the order of the faces; ``half.*`` is a
    constructed blend on exact halves, evaluated by the model;
  * ``swap_face_fine/gpen/face_enhancement.py`` is loaded with the four network modules stubbed, a ``FaceEnhancement`` is made with ``object.__new__`` and given
    the attributes ``process`` reads, and ``process`` runs with tests/gpen_paste_model.py's functions as its ``cv2`` and stub networks that return the case's
    seeded faces and masks.  That pins the control flow — the threshold skip, the small-face branch, the order of composition, the choice of the base — against
    the reference's own text.  Three literals of the reference do not fit cases this small and are bridged, each exactly: ``GaussianBlur``'s ``(101, 101), 11``
    (the stub blurs with the case's taps), ``mask_postprocess``'s default ``thres=20`` (the instance calls the reference's method with the case's), and the
    small-face limit ``100`` (case B's limit is 20: the reference sees its integer boxes times 5, the same comparison exactly).
It asserts what tests/test_gpen_paste_cpu.py asserts."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

sys.path.insert(0, HERE)

import gpen_paste_model as PM  # noqa: E402
from reference_shim import REF  # noqa: E402  (where the reference tree lies; nothing else of the shim is used)

N_SETS = 24

# tag -> (S, H, W, ksize, sigma, thres, small_face, with a base)
CASES = {"A": (32, 80, 96, 9, 1.5, 3, 100, False), "B": (48, 70, 53, 13, 2.0, 4, 20, False), "C": (32, 80, 96, 9, 1.5, 3, 100, True),
         "D": (32, 40, 44, 9, 1.5, 3, 100, False), "E": (32, 40, 44, 9, 1.5, 3, 100, False)}
# per face: (centre x, centre y, frame pixels per crop pixel, angle in degrees, score, box width, box height)
FACES = {"A": [(34., 36., 1.3, 8., 0.99, 40, 44), (52., 47., 1.1, -12., 0.97, 36, 38), (88., 70., 0.9, 20., 0.95, 30, 31)],
         "B": [(20., 22., 0.6, 5., 0.98, 26, 30), (30., 40., 0.5, -10., 0.5, 14, 15), (26., 35., 2.5, 45., 0.93, 18, 25)],
         "D": [],
         "E": [(20., 19., 0.8, 0., 0.99, 30, 30), (20., 19., 0.8, 0., 0.98, 30, 30)]}         # a tie: one geometry and one mask twice, two textures
FACES["C"] = FACES["A"]
SEEDS = {"A": 1, "B": 2, "C": 1, "D": 4, "E": 5}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # `align_type is 'cv2_affine'`
        spec.loader.exec_module(mod)
    return mod


class _Cv2(types.ModuleType):
    """The model's functions under cv2's names; ``calls`` records every warpAffine matrix with its size."""

    def __init__(self):
        super().__init__("cv2")
        self.calls, self.blur = [], None

    def warpAffine(self, src, M, dsize, flags=None):
        self.calls.append((np.array(M, np.float64), tuple(dsize)))
        return PM.warp_affine(src, M, dsize, flags)

    def GaussianBlur(self, img, ksize, sigma):
        assert tuple(ksize) == (101, 101) and sigma == 11
        return PM.gaussian_blur(img, self.blur[0], self.blur[1])

    def filter2D(self, img, ddepth, kernel):
        assert ddepth == -1 and np.array_equal(np.asarray(kernel) * 16, [[1, 2, 1], [2, 4, 2], [1, 2, 1]])
        return PM.filter2d_smooth(img)

    def resize(self, img, dsize):
        assert tuple(dsize) == img.shape[:2][::-1]
        return img

    def convertScaleAbs(self, x):
        return PM.convert_scale_abs(x)


def reference_modules():
    cv2 = sys.modules["cv2"] = _Cv2()
    sk = sys.modules["skimage"] = types.ModuleType("skimage")
    sk.transform = sys.modules["skimage.transform"] = types.ModuleType("skimage.transform")
    gp = os.path.join(REF, "swap_face_fine", "gpen")
    for pkg in ("swap_face_fine", "swap_face_fine.gpen", "swap_face_fine.gpen.face_detect", "swap_face_fine.gpen.face_parse", "swap_face_fine.gpen.face_model",
                "swap_face_fine.gpen.sr_model"):
        m = sys.modules[pkg] = types.ModuleType(pkg)
        m.__path__ = []
    for mod, cls in (("face_detect.retinaface_detection", "RetinaFaceDetection"), ("face_parse.face_parsing", "FaceParse"), ("face_model.face_gan", "FaceGAN"),
                     ("sr_model.real_esrnet", "RealESRNet")):
        m = sys.modules["swap_face_fine.gpen." + mod] = types.ModuleType("swap_face_fine.gpen." + mod)
        setattr(m, cls, type(cls, (), {}))
    align = _load("swap_face_fine.gpen.align_faces", os.path.join(gp, "align_faces.py"))
    fe = _load("swap_face_fine.gpen.face_enhancement", os.path.join(gp, "face_enhancement.py"))
    return cv2, align, fe


def landmarks_of(S, cx, cy, scale, deg, noise, rng, mirror=False):
    """The reference points of an S crop carried into the frame: scale * rot(deg) * (p - S / 2) + (cx, cy), plus noise; float32 (x0..x4, y0..y4)."""
    p = PM.reference_points(S) - S / 2
    if mirror:
        p[:, 0] = -p[:, 0]
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    q = scale * p @ R.T + np.array([cx, cy]) + noise * rng.standard_normal((5, 2))
    return q.T.reshape(10).astype(np.float32)


def landmark_sets():
    rng = np.random.default_rng(26)
    out = []
    for i in range(N_SETS - 2):
        out.append(landmarks_of(512, rng.uniform(100, 900), rng.uniform(100, 900), float(np.exp(rng.uniform(np.log(0.2), np.log(3)))), rng.uniform(-60, 60),
                                rng.uniform(0, 3), rng))
    out.append(landmarks_of(512, 400., 300., 0.7, 25., 1.0, rng, mirror=True))
    line = np.stack([np.linspace(100, 300, 5), np.linspace(200, 260, 5) + np.array([0, 0.02, -0.01, 0.015, 0])])         # nearly collinear
    out.append(line.reshape(10).astype(np.float32))
    return np.stack(out)


def case_inputs(tag):
    S, H, W, k, sigma, thres, small, with_base = CASES[tag]
    rng = np.random.default_rng(SEEDS[tag])
    yy, xx = np.mgrid[0:H, 0:W]
    frame = ((xx * 3 + yy * 2)[..., None] + np.array([0, 60, 140]) + rng.integers(0, 40, (H, W, 3))).astype(np.uint8)
    faces = FACES[tag]
    dets = np.array([[cx - bw / 2, cy - bh / 2, cx - bw / 2 + bw, cy - bh / 2 + bh, sc] for cx, cy, _, _, sc, bw, bh in faces], np.float32).reshape(-1, 5)
    dets[:, :4] = np.round(dets[:, :4])
    landms = np.array([landmarks_of(S, cx, cy, s, deg, 0.2, rng) for cx, cy, s, deg, *_ in faces], np.float32).reshape(-1, 10)
    ys, xs = np.mgrid[0:S, 0:S]
    ef, pm = [], []
    for i in range(len(faces)):
        ef.append(((xs * (5 + i) + ys * (3 + 2 * i))[..., None] * np.array([1, 2, 3]) + rng.integers(0, 64, (S, S, 3))).astype(np.uint8))
        blocks = (rng.random((S // 4, S // 4)) < 0.85).astype(np.uint8)
        blocks[S // 8 - 1:S // 8 + 1, S // 8 - 1:S // 8 + 1] = 0                                           # the hole
        pm.append(np.kron(blocks, np.ones((4, 4), np.uint8)) * np.uint8(255))
    if tag == "E":
        landms[1], pm[1] = landms[0], pm[0]
    base = ((xx * 2 + yy * 5)[..., None] + np.array([90, 10, 200]) + rng.integers(0, 30, (H, W, 3))).astype(np.uint8) if with_base else None
    return frame, dets, landms, np.array(ef, np.uint8).reshape(-1, S, S, 3), np.array(pm, np.uint8).reshape(-1, S, S), base


def run_reference(tag, cv2, align, fe):
    S, H, W, k, sigma, thres, small, with_base = CASES[tag]
    frame, dets, landms, ef, pm, base = case_inputs(tag)
    obj = object.__new__(fe.FaceEnhancement)
    obj.in_size = obj.out_size = S
    obj.threshold = 0.9
    obj.kernel = np.array([[0.0625, 0.125, 0.0625], [0.125, 0.25, 0.125], [0.0625, 0.125, 0.0625]], dtype="float32")
    obj.reference_5pts = align.get_reference_facial_points((S, S), 0.25, (0, 0), True)
    obj.use_sr = with_base
    obj.mask_postprocess = lambda mask: fe.FaceEnhancement.mask_postprocess(obj, mask, thres=thres)
    seen_dets = dets.copy()
    seen_dets[:, :4] *= 100 / small                                                                      # the reference's literal limit is 100
    assert np.array_equal(seen_dets[:, :4] * np.float32(small / 100), dets[:, :4])
    n_gan, n_parse = [0], [0]

    def gan(of):
        n_gan[0] += 1
        return ef[order[n_gan[0] - 1]].copy()

    def parse(face):
        n_parse[0] += 1
        return [pm[order[n_parse[0] - 1]].copy()]

    order = [i for i in range(len(dets)) if not dets[i, 4] < np.float32(0.9)]          # the faces that reach the networks, in order
    obj.facedetector = types.SimpleNamespace(detect=lambda img: (seen_dets, landms))
    obj.facegan = types.SimpleNamespace(process=gan)
    obj.faceparser = types.SimpleNamespace(process=parse)
    obj.srmodel = types.SimpleNamespace(process=lambda img: base)
    cv2.calls.clear()
    cv2.blur = (k, sigma)
    with np.errstate(all="ignore"):
        out, orig_faces, enhanced = obj.process(frame.copy())
    assert n_gan[0] == n_parse[0] == len(order) == len(orig_faces)
    tfm = np.array([M for M, d in cv2.calls if d == (S, S)]).reshape(-1, 2, 3)
    inv = np.array([M for M, d in cv2.calls if d == (W, H)]).reshape(-1, 2, 3)[0::2]
    T = np.zeros((len(dets), 2, 2, 3))
    T[order, 0], T[order, 1] = tfm, inv
    rec = dict(frame=frame, dets=dets, landms=landms, ef=ef, pm=pm, out=out, orig=np.array(orig_faces, np.uint8).reshape(-1, S, S, 3), T=T,
               cfg=np.array([S, H, W, k, sigma, thres, small, int(with_base)], np.float64))
    if with_base:
        rec["base"] = base
    return rec


def main(path):
    cv2, align, fe = reference_modules()
    store = {}
    for S in (512, 32, 48):
        store[f"ref.{S}"] = align.get_reference_facial_points((S, S), 0.25, (0, 0), True)
        assert np.abs(store[f"ref.{S}"] - PM.reference_points(S)).max() <= 1e-12
    assert np.allclose(store["ref.512"][0], (202.04068428, 242.88396346), atol=1e-8)
    sets = landmark_sets()
    tfm, inv = [], []
    for l in sets:
        cv2.calls.clear()
        _, ti = align.warp_and_crop_face(np.zeros((4, 4, 3), np.uint8), l.reshape(2, 5), reference_pts=store["ref.512"], crop_size=(512, 512))
        tfm.append(cv2.calls[0][0])
        inv.append(np.array(ti, np.float64))
    store["sets.landms"], store["sets.tfm"], store["sets.tfm_inv"] = sets, np.array(tfm), np.array(inv)
    # what the reference's float32 path costs it: its own _umeyama on the same points in float64, against what warp_and_crop_face (float32) returned
    worst, own = 0.0, 0.0
    ref64 = store["ref.512"].astype(np.float32).astype(np.float64)
    for l, a, b in zip(sets, tfm, inv):
        src64 = l.reshape(2, 5).T.astype(np.float64)
        p64, scale = align._umeyama(src64, ref64)
        i64, _ = align._umeyama(ref64, src64, False, scale=1.0 / scale)
        own = max(own, np.abs(p64[:2] - a).max() / np.abs(a).max(), np.abs(i64[:2] - b).max() / np.abs(b).max())
        m, mi, ok = PM.similarity_pair(l, store["ref.512"])
        assert ok
        worst = max(worst, np.abs(m - a).max() / np.abs(a).max(), np.abs(mi - b).max() / np.abs(b).max())
    print(f"the reference's float32 path against its own float64: {own:.3e}; the closed form against the float32 path: {worst:.3e}")
    assert worst <= 4 * own
    for tag in CASES:
        rec = run_reference(tag, cv2, align, fe)
        out, orig, fm, pre, flags, faces, masks = PM.model_outputs(rec)
        assert np.array_equal(out, rec["out"]) and np.array_equal(orig, rec["orig"]), tag
        base = rec["base"] if "base" in rec else rec["frame"]
        strict = PM.strict_pixels(base, faces, masks, rec["T"], flags)
        print(f"case {tag}: {len(flags)} faces, flags {flags.tolist()}, changed pixels {(out != base).any(-1).mean():.3f}, non-strict {1 - strict.mean():.4f}")
        assert strict.mean() >= 0.99 or tag == "E", tag                       # E is the tie: every pixel both faces reach is non-strict by construction
        for k, v in rec.items():
            store[f"{tag}.{k}"] = v
    # a constructed blend whose sums fall on .5 over an even integer: base 0 or 2, face 1 or 3, mask 0.5 -> 0.5, 1.5, 2.5
    hb = np.array([[[0, 2, 0], [2, 2, 0]]], np.uint8)
    hp = np.array([[[1, 1, 3], [3, 1, 1]]], np.uint8)
    store["half.base"], store["half.img"], store["half.mask"] = hb, hp, np.full((1, 2), 0.5, np.float32)
    store["half.out"] = PM.compose(hb, [store["half.mask"]], [hp])[0]
    assert store["half.out"].tolist() == [[[0, 2, 2], [2, 2, 0]]]
    store["sets.deviation"] = np.float64(own)
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g26_gpen_paste.npz"))
