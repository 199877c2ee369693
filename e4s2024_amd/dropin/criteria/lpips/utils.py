"""Drop-in for the reference's ``criteria/lpips/utils.py``.

``get_state_dict`` never downloads: the reference fetches the lin weights from a URL at construction (:12-19).  Here the weights come from
``LPIPS.load_state_dict``; ``convert_upstream_state_dict`` builds that state_dict from the two published files (torchvision's AlexNet
``features.*`` and the lpips package's ``lin*.model.1.weight``)."""
import re
from collections import OrderedDict

import torch

from criteria.lpips.networks import AlexNet

_LAYERS = (0, 3, 6, 8, 10)


def normalize_activation(x, eps=1e-10):
    """``x`` divided per pixel by its channel norm (``sqrt(sum_c x^2 + 1e-16) + eps``)."""
    return x / ((x * x).sum(1, keepdim=True).add(1e-16).sqrt() + eps)


def get_state_dict(net_type: str = 'alex', version: str = '0.1'):
    raise RuntimeError("criteria.lpips.get_state_dict: weights are never downloaded here; build the module and load them with "
                       "LPIPS.load_state_dict(convert_upstream_state_dict(alexnet_state_dict, lpips_lin_state_dict))")


def convert_upstream_state_dict(alexnet_state_dict, lin_state_dict, net_type: str = 'alex', version: str = '0.1'):
    """The drop-in ``LPIPS`` state_dict from torchvision's ``alexnet`` weights (``features.{0,3,6,8,10}.{weight,bias}``; other keys ignored)
    and the lpips ``alex.pth`` lin weights (``lin{i}.model.1.weight`` -> ``lin.{i}.1.weight``); ``net.mean`` / ``net.std`` are the fixed buffers."""
    if net_type != 'alex':
        raise NotImplementedError(f"net_type={net_type!r}: only 'alex' is provided")
    if version != '0.1':
        raise ValueError(f"LPIPS version {version!r}: only '0.1' is provided")
    sd = OrderedDict((k, v.clone()) for k, v in AlexNet().state_dict().items() if k in ("mean", "std"))
    sd = OrderedDict(("net." + k, v) for k, v in sd.items())
    for i in _LAYERS:
        for n in ("weight", "bias"):
            sd[f"net.layers.{i}.{n}"] = alexnet_state_dict[f"features.{i}.{n}"]
    heads = {}
    for key, val in lin_state_dict.items():
        m = re.fullmatch(r"lin(\d+)\.model\.1\.weight", key)
        if m:
            heads[int(m.group(1))] = val
    missing = [i for i in range(5) if i not in heads]
    if missing:
        raise KeyError(f"lpips lin weights lack lin{missing[0]}.model.1.weight")
    for i in range(5):
        sd[f"lin.{i}.1.weight"] = heads[i]
    return sd
