"""Generate g27_gpen_sr.npz: what the reference's own code gives for the RealESRNet pass of ``FaceEnhancement.process`` and for ``process`` with ``use_sr``.

    python tests/golden/make_golden_gpen_sr.py [out.npz]

Only the build container has the reference tree.  No reference source is copied:
  * ``swap_face_fine/gpen/sr_model/arch_util.py``, ``rrdbnet_arch.py`` and ``real_esrnet.py`` are loaded from where they lie (as make_golden_gpen_paste.py loads
    ``align_faces.py``).  A ``RealESRNet`` is made with ``object.__new__`` and given a reference ``RRDBNet`` on the CPU with the seeded, calibrated weights of
    tests/gpen_sr_model.py's image cases; its ``process`` runs on the cases' BGR images.  Stored per case: the image, the uint8 result and the network's float32
    output (taken with a forward hook; image cases only);
  * ``swap_face_fine/gpen/face_enhancement.py`` is loaded and run as make_golden_gpen_paste.py does it — the detector, the generator and the ParseNet stubbed
    with case A's detections, faces and masks — but with the real reference ``RealESRNet`` above as ``srmodel`` and ``use_sr=True``, once not aligned on an
    even-sized frame, once on an odd-sized one, once aligned.  ``cv2`` is the models' functions, ``resize`` now the fixed-point resize of gpen_sr_model.  That
    pins the control flow: the resize to the SR size, detection and crops on the resized frame, the paste over ``img_sr``, the order of the aligned branch.
It asserts what tests/test_gpen_sr_cpu.py asserts."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))                                    # the package (gpen_sr_model takes its seeded weights from it)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gpen_paste_model as PM  # noqa: E402
import gpen_sr_model as M  # noqa: E402
import make_golden_gpen_paste as MP  # noqa: E402


class _Cv2(MP._Cv2):
    """make_golden_gpen_paste's cv2 with a real ``resize``: the identity at equal size (the mask's), gpen_sr_model's fixed-point resize otherwise."""

    def resize(self, img, dsize):
        if tuple(dsize) == img.shape[:2][::-1]:
            return img
        self.resized.append(M.resize_linear(img, dsize))
        return self.resized[-1]


def reference_modules():
    cv2, align, fe = MP.reference_modules()
    cv2.__class__ = _Cv2
    cv2.resized = []
    sr = os.path.join(MP.REF, "swap_face_fine", "gpen", "sr_model")
    for name in ("arch_util", "rrdbnet_arch", "real_esrnet"):                                  # the real ones over reference_modules' empty stand-ins
        MP._load("swap_face_fine.gpen.sr_model." + name, os.path.join(sr, name + ".py"))
    return cv2, align, fe, sys.modules["swap_face_fine.gpen.sr_model.rrdbnet_arch"], sys.modules["swap_face_fine.gpen.sr_model.real_esrnet"]


def reference_sr(arch, resr, sd):
    """(a reference RealESRNet on the CPU with the weights ``sd``, the list its network's outputs are appended to)."""
    scale, nf, nb = M.scale_of(sd), int(sd["conv_first.weight"].shape[0]), M.num_blocks(sd)
    net = arch.RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=nf, num_block=nb, num_grow_ch=32, scale=scale)
    net.load_state_dict(sd, strict=True)
    net.eval()
    seen = []
    net.register_forward_hook(lambda mod, args, out: seen.append(out.detach().numpy().copy()))
    obj = object.__new__(resr.RealESRNet)
    obj.base_dir, obj.scale, obj.device, obj.srmodel = "./", scale, "cpu", net
    return obj, seen


def check_sr(tag, c, r32, out):
    """What tests/test_gpen_sr_cpu.py asserts of a stored RealESRNet result against the model ``c`` (``M.solved``)."""
    err, b = M.max_err(r32, c["r"]), M.bound(c["e32"], c["r"])
    strict, clamped, std = M.check_u8(out, c["u"], c["e32"])
    print(f"{tag}: net output {r32.shape}, err {err:.3e} = {err / c['e32']:.2f} e32 (bound {b:.3e}); uint8 {out.shape}: strict {100 * strict:.2f} %, "
          f"clamped {100 * clamped:.2f} %, std {std:.1f}")
    assert err <= b and strict >= 0.99 and clamped < 0.10 and std > 30, tag


def run_face_enhancement(tag, cv2, align, fe, arch, resr):
    H, W, aligned = M.FE_CASES[tag]
    P = M.FE_PASTE
    S = P["S"]
    _, dets, landms, ef, pm, _ = MP.case_inputs("A")
    img = ef[0].copy() if aligned else M.fe_frame(tag)                                         # (aligned: the face the stub generator returns)
    c = M.fe_solved(tag, img)
    srmodel, seen = reference_sr(arch, resr, c["sd"])
    obj = object.__new__(fe.FaceEnhancement)
    obj.in_size = obj.out_size = S
    obj.threshold = 0.9
    obj.kernel = np.array([[0.0625, 0.125, 0.0625], [0.125, 0.25, 0.125], [0.0625, 0.125, 0.0625]], dtype="float32")
    obj.reference_5pts = align.get_reference_facial_points((S, S), 0.25, (0, 0), True)
    obj.use_sr = True
    obj.mask_postprocess = lambda mask: fe.FaceEnhancement.mask_postprocess(obj, mask, thres=P["thres"])
    n_gan, n_parse, frames_seen = [0], [0], []
    order = [i for i in range(len(dets)) if not dets[i, 4] < np.float32(0.9)]

    def gan(of):
        n_gan[0] += 1
        return ef[order[n_gan[0] - 1]].copy()

    def parse(face):
        n_parse[0] += 1
        return [pm[order[n_parse[0] - 1]].copy()]

    def detect(frame):
        frames_seen.append(frame.copy())
        return dets, landms

    obj.facedetector = types.SimpleNamespace(detect=detect)
    obj.facegan = types.SimpleNamespace(process=gan)
    obj.faceparser = types.SimpleNamespace(process=parse)
    sr_results = []
    obj.srmodel = types.SimpleNamespace(process=lambda im: sr_results.append(srmodel.process(im)) or sr_results[-1])
    cv2.calls.clear()
    cv2.resized.clear()
    cv2.blur = (P["ksize"], P["sigma"])
    if aligned:
        probe = np.zeros((S, S, 3), np.uint8)
        out, orig_faces, enhanced = obj.process(probe, aligned=True)
        assert n_gan[0] == 1 and n_parse[0] == 0 and not frames_seen and orig_faces[0] is probe and np.array_equal(enhanced[0], img)
        check_sr(tag, c, seen[0], out[None])
        return dict(ef=img, out=out)
    with np.errstate(all="ignore"):
        out, orig_faces, enhanced = obj.process(img.copy())
    Ho, Wo = M.output_size(H, W, M.FE_NET[0])
    img_sr = sr_results[0]
    assert out.shape == (Ho, Wo, 3) and len(cv2.resized) == 1 and len(frames_seen) == 1 and np.array_equal(frames_seen[0], cv2.resized[0])
    assert n_gan[0] == n_parse[0] == len(order) == len(orig_faces)
    check_sr(tag, c, seen[0], img_sr[None])
    tfm = np.array([Mx for Mx, d in cv2.calls if d == (S, S)]).reshape(-1, 2, 3)
    inv = np.array([Mx for Mx, d in cv2.calls if d == (Wo, Ho)]).reshape(-1, 2, 3)[0::2]
    T = np.zeros((len(dets), 2, 2, 3))
    T[order, 0], T[order, 1] = tfm, inv
    rec = dict(frame=cv2.resized[0], dets=dets, landms=landms, ef=ef, pm=pm, out=out, orig=np.array(orig_faces, np.uint8).reshape(-1, S, S, 3), T=T,
               cfg=np.array([S, Ho, Wo, P["ksize"], P["sigma"], P["thres"], P["small_face"], 1], np.float64), base=img_sr)
    # the model of row f15 on the resized frame over the reference's img_sr gives the reference's result exactly
    mout, morig = PM.model_outputs(rec)[:2]
    assert np.array_equal(mout, out) and np.array_equal(morig, rec["orig"]), tag
    print(f"{tag}: frame {H} x {W} -> {Ho} x {Wo}, {len(order)} faces pasted, changed pixels {(out != img_sr).any(-1).mean():.3f}")
    rec["input"] = img
    return rec


def main(path):
    cv2, align, fe, arch, resr = reference_modules()
    store = {}
    for tag in M.IMAGE_CASES:
        c = M.image_case(tag)
        srmodel, seen = reference_sr(arch, resr, c["sd"])
        out = srmodel.process(c["img"][0].copy())
        assert out is not None and len(seen) == 1
        check_sr(tag, c, seen[0], out[None])
        store[f"{tag}.img"], store[f"{tag}.out"], store[f"{tag}.r"] = c["img"][0], out, seen[0][0]
    # the reference's own refusal: on an image with no more rows than the pad adds F.pad raises (it stands in front of process's try)
    srmodel, _ = reference_sr(arch, resr, M.image_case(M.tag_of(1, 64, 1, 5, 6))["sd"])
    try:
        srmodel.process(np.zeros((1, 8, 3), np.uint8))
        raise AssertionError("the reference accepted a 1 x 8 image at scale 1")
    except RuntimeError as e:
        assert "Padding size should be less" in str(e)
    for tag in M.FE_CASES:
        for k, v in run_face_enhancement(tag, cv2, align, fe, arch, resr).items():
            if k in M.FE_SHARED and not M.FE_CASES[tag][2]:                                      # case A's detections, faces and masks: stored once
                assert f"fe.{k}" not in store or np.array_equal(store[f"fe.{k}"], v)
                store[f"fe.{k}"] = v
            else:
                store[f"{tag}.{k}"] = v
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g27_gpen_sr.npz"))
