"""A float64 restatement of LPIPS-AlexNet (criteria/lpips: lpips.py:28-34, networks.py:47-56 + 76-84, utils.py:6-9) and of the reference's
multi-scale use (training/video_swap_ft_coach.py:201-211), in plain torch on the CPU: the yardstick of tests/test_lpips_cpu.py (against the
fixture g14, made from the reference's own classes) and of tests/test_gpu_lpips.py."""
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import seeded

LAYERS = (0, 3, 6, 8, 10)
PADS = (2, 2, 1, 1, 1)
STRIDES = (4, 1, 1, 1, 1)


def taps(x, sd):
    """The five ReLU outputs of AlexNet's ``features`` on the z-scored ``x``."""
    z = (x - sd["net.mean"]) / sd["net.std"]
    out = []
    for i, li in enumerate(LAYERS):
        if i in (1, 2):
            z = F.max_pool2d(z, 3, 2)
        z = F.relu(F.conv2d(z, sd[f"net.layers.{li}.weight"], sd[f"net.layers.{li}.bias"], stride=STRIDES[i], padding=PADS[i]))
        out.append(z)
    return out


def normalize(f):
    return f / (torch.sqrt((f * f).sum(1, keepdim=True) + 1e-16) + 1e-10)


def lpips(x, y, sd):
    """LPIPS(x, y): sum over taps of the batch sum of the per-image mean over pixels of the lin-weighted squared difference, / batch size."""
    tot = 0.0
    for i, (fx, fy) in enumerate(zip(taps(x, sd), taps(y, sd))):
        d = (normalize(fx) - normalize(fy)) ** 2
        tot = tot + (d * sd[f"lin.{i}.1.weight"]).sum(1).mean((1, 2)).sum()
    return tot / x.shape[0]


def box(x, f: int):
    return x if f == 1 else F.avg_pool2d(x, f)


def multiscale(x, y, sd, scales: int = 3, mask=None):
    if mask is not None:
        x, y = x * mask, y * mask
    return sum(lpips(box(x, 1 << i), box(y, 1 << i), sd) for i in range(scales))


def double_sd(sd):
    return {k: v.detach().to(torch.float64) for k, v in sd.items()}


def loss_and_grad(x, y, sd, factor: int = 1, scales=None):
    """(loss, d loss / d x) in float64; ``scales`` given: the multi-scale sum, else one scale at ``factor``."""
    sd = double_sd(sd)
    x = x.detach().to(torch.float64).requires_grad_(True)
    y = y.detach().to(torch.float64)
    loss = multiscale(x, y, sd, scales) if scales else lpips(box(x, factor), box(y, factor), sd)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def images(seed: int, side: int, bs: int):
    """The seeded (x, y) image pair of a fixture case, float32 in (-1, 1)."""
    x = np.tanh(seeded.seeded_array(seed, f"lpips_x{side}", (bs, 3, side, side), dist="normal")).astype(np.float32)
    y = np.tanh(seeded.seeded_array(seed, f"lpips_y{side}", (bs, 3, side, side), dist="normal")).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y)
