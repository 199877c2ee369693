"""Generate g16_face_parsing.npz: the face-parsing feature loss, its similarity improvement and its input gradient from the reference's own
``criteria/face_parsing/face_parsing_loss.py::FaceParsingLoss`` (on ``criteria/face_parsing/unet.py::unet``), on the CPU in float64.

    python tests/golden/make_golden_face_parsing.py [out.npz]

Only the build container has the reference tree.  Weights come from ``seeded.seeded_unet_state_dict(SEED)`` (saved to a temporary file that the
reference constructor ``torch.load``s as ``opts.face_parsing_model_path``), images from ``tests/fp_model.images``; neither is stored.  The
reference module imports cv2 and torchvision for its ``inference`` visualisation only; empty stand-ins are registered here when they are missing.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("E4S_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import fp_model  # noqa: E402  (tests/fp_model.py: the seeded images and the float64 restatement)
from e4s2024_amd import seeded  # noqa: E402

SEED = 43
CASES = [(512, 2), (1024, 2), (256, 2)]          # (side, batch)
N_SAMPLES = 4096


def sample_index(n: int):
    return np.sort(np.random.RandomState(SEED).choice(n, N_SAMPLES, replace=False)).astype(np.int64)


def _stub_visualisation_modules():
    for name in ("cv2", "torchvision", "torchvision.utils", "torchvision.transforms"):
        if name in sys.modules:
            continue
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    tv = sys.modules["torchvision"]
    for sub in ("utils", "transforms"):
        if not hasattr(tv, sub):
            setattr(tv, sub, sys.modules["torchvision." + sub])
    if not hasattr(sys.modules["torchvision.utils"], "save_image"):
        sys.modules["torchvision.utils"].save_image = None


def reference_loss(sd):
    if not os.path.isdir(REF):
        raise RuntimeError(f"reference tree not found at {REF}; goldens can only be made in the build container")
    if REF not in sys.path:
        sys.path.insert(0, REF)
    _stub_visualisation_modules()
    from criteria.face_parsing.face_parsing_loss import FaceParsingLoss
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "face_parsing.pth")
        torch.save(sd, path)
        m = FaceParsingLoss(types.SimpleNamespace(face_parsing_model_path=path))
    return m.double().eval()


def main(out):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = seeded.seeded_unet_state_dict(SEED)
    m = reference_loss(sd)
    gsd = m.state_dict()
    d = {"seed": np.int64(SEED), "keys": np.array(list(gsd.keys())),
         "shapes": np.array([list(v.shape) + [1] * (4 - v.dim()) for v in gsd.values()], dtype=np.int64)}
    for side, bs in CASES:
        x, y = fp_model.images(SEED, side, bs)
        rms, pos = fp_model.tap_rms(x, sd)
        assert all(0.05 <= r <= 20 for r in rms), rms
        xd = x.double().requires_grad_(True)
        loss, sim = m(xd, y.double())
        (g,) = torch.autograd.grad(loss, xd)
        g = g.numpy()
        l2, _, per, _ = fp_model.loss_and_grad(x, y, sd)        # per-tap losses from the float64 restatement, checked against the total here
        assert abs(l2.item() - float(loss)) <= 1e-12 * abs(float(loss)), (l2.item(), float(loss))
        d[f"loss{side}"], d[f"sim{side}"], d[f"per{side}"] = float(loss), float(sim), per.numpy()
        idx = sample_index(g.size)
        d[f"grad{side}_idx"], d[f"grad{side}_samples"], d[f"grad{side}_norm"] = idx, g.reshape(-1)[idx], np.linalg.norm(g)
        print(f"{side}: loss {float(loss):.6f} sim {float(sim):.6f} |g| {np.linalg.norm(g):.3e} tap rms {[round(r, 3) for r in rms]} "
              f"positive {[round(p, 2) for p in pos]}", flush=True)
    np.savez_compressed(out, **{k: np.asarray(v) for k, v in d.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g16_face_parsing.npz"))
