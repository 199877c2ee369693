"""What the stage modules (``ops_recolor``, ``ops_rrdb``, ``ops_gpen*``, ``ops_parsenet``, ``ops_retinaface``) and ``pipeline`` share when they take a network's
weights and tensors from a caller: the description of a network (``_Net``), the one validation of a module or mapping against it (``_validated``: keys, shapes
and dtypes checked once per public call and handed on to ``lossnet.prepare``), and the tensor checks every public call makes before any launch."""
from __future__ import annotations

import functools
from collections import namedtuple

import torch
import torch.nn as nn


def _tensor_checked(name, nm, t, dtype, ndim, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a torch.Tensor")
    if t.dtype != dtype or t.dim() != ndim:
        raise ValueError(f"{name}: {nm}: expected {what}, got {t.dtype} {tuple(t.shape)}")


def _cuda_checked(name, **tensors):
    for nm, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {nm} must be a CUDA tensor")


# What ``_validated`` needs to know of a network: ``cls`` its name in messages; ``shapes(variant)`` the public ``{key: shape}`` function; ``prefixes`` the key
# prefixes a checkpoint may carry (``nested``: or a mapping of that name inside it); ``variant(name, sd)`` reads the width / small or full / block count off
# the bare keys and raises for a missing probe key; ``training``: why a module in training mode is refused (None: it makes no difference); ``skip``: the key
# suffixes that are not float weights.
_Net = namedtuple("_Net", "cls shapes prefixes nested probes variant training skip")


@functools.lru_cache(maxsize=8)
def _keys_shapes(cls, *args):
    with torch.device("meta"):
        return tuple((k, tuple(v.shape)) for k, v in cls(*args).state_dict().items())


@functools.lru_cache(maxsize=8)
def _float_keys(net, variant):
    return tuple((k, shape) for k, shape in net.shapes(variant).items() if not k.endswith(net.skip))


def _validated(name, weights, net):
    """(mapping with bare keys, variant, float tensors in key order) of ``weights``: a module with the network's keys or a mapping, bare or prefixed.  Made
    once per public call (one ``state_dict()``) and handed on.  Refused, in this order: a module in training mode, anything without keys, a missing probe key,
    a missing key, a wrong shape or dtype."""
    if isinstance(weights, nn.Module):
        if weights.training and net.training:
            raise RuntimeError(f"{name}: {type(weights).__name__} is in training mode; {net.training}: call .eval()")
        sd = weights.state_dict()
    elif hasattr(weights, "keys"):
        sd = weights
    else:
        raise TypeError(f"{name}: weights must be a module or a mapping with the keys of {net.cls}, got {type(weights).__name__}")
    if not any(p in sd for p in net.probes):
        for prefix in net.prefixes:
            if net.nested and isinstance(sd.get(prefix[:-1]), dict):          # the checkpoint file as torch.load gives it
                sd = sd[prefix[:-1]]
                break
            if any(prefix + p in sd for p in net.probes):
                sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
                break
    variant = net.variant(name, sd)
    out = []
    for k, shape in _float_keys(net, variant):
        t = sd.get(k)
        if t is None:
            raise KeyError(f"{name}: the weights lack '{k}': expected the keys of {net.cls} (ops.{net.shapes.__name__}({variant!r}))")
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32:
            raise ValueError(f"{name}: '{k}' is {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}, expected float32 {shape}")
        out.append(t)
    return sd, variant, out


def _devices_checked(name, nm, t, ts):
    if any(w.device != t.device for w in ts):
        raise RuntimeError(f"{name}: device mismatch: {nm} on {t.device}, the weights on {sorted({str(w.device) for w in ts})}")
