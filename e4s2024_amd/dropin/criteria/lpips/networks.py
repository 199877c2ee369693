"""Drop-in for the reference's ``criteria/lpips/networks.py``: the same class names and state_dict layout (``mean``, ``std``,
``layers.{0,3,6,8,10}.{weight,bias}`` of AlexNet's ``features``; ``LinLayers`` ``{i}.1.weight``), built without torchvision and without
pretrained downloads.  ``BaseNet.forward`` runs on the HIP kernels (``e4s2024_amd.ops_lpips.features``); a network whose weights were never
loaded refuses to run."""
from typing import Sequence

import torch
import torch.nn as nn

from e4s2024_amd import ops_lpips

# AlexNet's ImageNet input statistics in LPIPS's [-1, 1] image scale (the reference's fixed buffers)
_SHIFT = (-.030, -.088, -.188)
_SCALE = (.458, .448, .450)


def get_network(net_type: str):
    if net_type == 'alex':
        return AlexNet()
    if net_type in ('squeeze', 'vgg'):
        raise NotImplementedError(f"LPIPS net_type={net_type!r} is not provided on this engine (only 'alex')")
    raise NotImplementedError(f"unknown LPIPS net_type {net_type!r} (alex, squeeze or vgg)")


def _frozen(module: nn.Module) -> nn.Module:
    module.requires_grad_(False)
    return module


class LinLayers(nn.ModuleList):
    """One bias-free 1x1 projection to a single channel per tap, each behind an identity slot (so that its weight is ``{i}.1.weight``)."""

    def __init__(self, n_channels_list: Sequence[int]):
        heads = [nn.Sequential(nn.Identity(), nn.Conv2d(c, 1, kernel_size=1, bias=False)) for c in n_channels_list]
        super().__init__(heads)
        _frozen(self)


class BaseNet(nn.Module):
    """Holds the input statistics (``mean``, ``std`` buffers of shape [1, 3, 1, 1]) and the load state of the feature network."""

    def __init__(self):
        super().__init__()
        self.register_buffer('mean', torch.tensor(_SHIFT).view(1, 3, 1, 1))
        self.register_buffer('std', torch.tensor(_SCALE).view(1, 3, 1, 1))
        self._loaded = False

    def set_requires_grad(self, state: bool):
        self.requires_grad_(state)
        for b in self.buffers():
            b.requires_grad_(state)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._loaded = self._loaded or set(self.state_dict().keys()) <= set(state_dict.keys())
        return out

    def forward(self, x: torch.Tensor):
        """The normalised activations at the five taps (no gradient)."""
        return ops_lpips.features(x, self)


def _alexnet_features():
    """AlexNet's ``features`` layer list (conv 11/4/2, ReLU, pool, conv 5/1/2, ReLU, pool, three conv 3/1/1 with ReLU, pool)."""
    return nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))


class AlexNet(BaseNet):
    def __init__(self):
        super().__init__()
        self.layers = _alexnet_features()
        self.target_layers = [2, 5, 8, 10, 12]          # 1-based positions of the five tapped ReLUs in ``layers``
        self.n_channels_list = list(ops_lpips.CHANNELS)
        _frozen(self)
