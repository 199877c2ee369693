"""Generate g15_id.npz: the ArcFace identity loss, its similarity improvement and its input gradient from the reference's own
``criteria/id_loss.py::IDLoss`` (on ``models/encoders/model_irse.py::Backbone(112, 50, 'ir_se')``), on the CPU in float64.

    python tests/golden/make_golden_id.py [out.npz]

Only the build container has the reference tree.  Weights come from ``seeded.seeded_irse50_state_dict(SEED)`` (saved to a temporary file that
the reference constructor ``torch.load``s as ``opts.ir_se50_path``), images from ``tests/id_model.images``; neither is stored.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import id_model  # noqa: E402  (tests/id_model.py: the seeded images)
from e4s2024_amd import seeded  # noqa: E402

SEED = 41
CASES = [(112, 2), (256, 2), (1024, 2)]          # (side, batch)
N_SAMPLES = 4096


def sample_index(n: int):
    return np.sort(np.random.RandomState(SEED).choice(n, N_SAMPLES, replace=False)).astype(np.int64)


def reference_idloss(sd, multiscale: bool):
    import reference_shim
    reference_shim.install()
    from criteria.id_loss import IDLoss
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ir_se50.pth")
        torch.save(sd, path)
        m = IDLoss(types.SimpleNamespace(ir_se50_path=path, id_loss_multiscale=multiscale))
    return m.double().eval()


def loss_grad(m, x, y):
    x = x.double().requires_grad_(True)
    loss, sim, _ = m(x, y.double())
    (g,) = torch.autograd.grad(loss, x)
    return float(loss), float(sim), g.numpy()


def main(out):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = seeded.seeded_irse50_state_dict(SEED)
    d = {"seed": np.int64(SEED)}
    for ms in (True, False):
        m = reference_idloss(sd, ms)
        if ms:
            fsd = m.state_dict()
            d["keys"] = np.array(list(fsd.keys()))
            d["shapes"] = np.array([list(v.shape) + [1] * (4 - v.dim()) for v in fsd.values()], dtype=np.int64)
        tag = "ms" if ms else "ss"
        for side, bs in CASES:
            x, y = id_model.images(SEED, side, bs)
            rms = id_model.tap_rms(x, sd)
            assert all(0.05 <= r <= 20 for r in rms), rms
            loss, sim, g = loss_grad(m, x, y)
            d[f"loss{side}_{tag}"], d[f"sim{side}_{tag}"] = loss, sim
            if ms:      # per-scale losses, from the float64 restatement (checked against the total here)
                l2, _, per, _ = id_model.loss_and_grad(x, y, sd)
                assert abs(l2.item() - loss) <= 1e-12 * abs(loss), (l2.item(), loss)
                d[f"per{side}"] = per.numpy()
            if side == 112 and ms:
                d[f"grad{side}_{tag}"] = g.astype(np.float32)
            idx = sample_index(g.size)
            d[f"grad{side}_{tag}_idx"], d[f"grad{side}_{tag}_samples"], d[f"grad{side}_{tag}_norm"] = idx, g.reshape(-1)[idx], np.linalg.norm(g)
            print(f"{side} {tag}: loss {loss:.6f} sim {sim:.6f} |g| {np.linalg.norm(g):.3e} tap rms {[round(r, 3) for r in rms]}", flush=True)
    np.savez_compressed(out, **{k: np.asarray(v) for k, v in d.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g15_id.npz"))
