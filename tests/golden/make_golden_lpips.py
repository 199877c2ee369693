"""Generate g14_lpips.npz: LPIPS-AlexNet loss and input gradient from the reference's own ``criteria/lpips`` classes, on the CPU in float64.

    python tests/golden/make_golden_lpips.py [out.npz]

Only the build container has the reference tree.  What is wired (no reference source is copied):
  * ``torchvision`` is not installed: ``torchvision.models.alexnet`` is a stub that builds AlexNet's documented ``features`` layer list
    (weights irrelevant: the seeded state_dict is loaded over them);
  * ``criteria.lpips.utils.get_state_dict`` downloads at construction: it is replaced, for the construction only, by the seeded lin weights.
Weights come from ``seeded.seeded_lpips_state_dict(SEED)``, images from ``tests/lpips_model.images``; neither is stored.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import lpips_model  # noqa: E402  (tests/lpips_model.py: the seeded images)
from e4s2024_amd import seeded  # noqa: E402

SEED = 31
CASES = [(64, 1, (1, 2)), (128, 1, (1, 2, 4))]          # (side, batch, box factors)
N_SAMPLES = 4096


def images(side: int, bs: int):
    return lpips_model.images(SEED, side, bs)


def sample_index(n: int):
    return np.sort(np.random.RandomState(SEED).choice(n, N_SAMPLES, replace=False)).astype(np.int64)


def _stub_torchvision():
    def alexnet(pretrained=False, **kw):
        m = types.SimpleNamespace()
        m.features = nn.Sequential(
            nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
            nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2))
        return m
    tv = sys.modules.get("torchvision") or types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.alexnet = alexnet
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tv.models


def reference_lpips(sd):
    import reference_shim
    reference_shim.install()
    _stub_torchvision()
    for m in [m for m in sys.modules if m == "criteria" or m.startswith("criteria.")]:
        del sys.modules[m]
    import criteria.lpips.lpips as L
    lin = {k[len("lin."):]: v for k, v in sd.items() if k.startswith("lin.")}
    saved = L.get_state_dict
    L.get_state_dict = lambda net_type='alex', version='0.1': lin
    try:
        m = L.LPIPS(net_type='alex', version='0.1')
    finally:
        L.get_state_dict = saved
    m.load_state_dict(sd)
    return m.double().eval()


def loss_grad(m, x, y, factors):
    x = x.double().requires_grad_(True)
    y = y.double()
    side = x.shape[-1]
    loss = sum(m(F.adaptive_avg_pool2d(x, side // f), F.adaptive_avg_pool2d(y, side // f)) for f in factors)
    (g,) = torch.autograd.grad(loss, x)
    return loss.item(), g.numpy()


def main(out):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = seeded.seeded_lpips_state_dict(SEED)
    m = reference_lpips(sd)
    d = {"seed": np.int64(SEED), "keys": np.array(list(m.state_dict().keys())),
         "shapes": np.array([list(v.shape) + [1] * (4 - v.dim()) for v in m.state_dict().values()], dtype=np.int64)}
    for side, bs, factors in CASES:
        x, y = images(side, bs)
        for f in factors:
            d[f"loss{side}_f{f}"], d[f"grad{side}_f{f}"] = loss_grad(m, x, y, (f,))
    x, y = images(1024, 2)
    d["loss1024"], g = loss_grad(m, x, y, (1, 2, 4))
    idx = sample_index(g.size)
    d["grad1024_idx"], d["grad1024_samples"], d["grad1024_norm"] = idx, g.reshape(-1)[idx], np.linalg.norm(g)
    np.savez_compressed(out, **{k: np.asarray(v) for k, v in d.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g14_lpips.npz"))
