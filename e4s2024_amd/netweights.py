"""What every network of the package (the stage modules ``ops_recolor``, ``ops_rrdb``, ``ops_gpen*``, ``ops_parsenet``, ``ops_retinaface``, ``ops_reenact*``, the
frozen loss networks ``ops_lpips``, ``ops_id``, ``ops_fp``) and ``pipeline`` share when they take a network's weights and tensors from a caller: the description
of a network (``_Net``; ``module_net`` pins it to the structure a mirror module was built with), the one validation of a module or mapping against it
(``_validated``: keys, shapes and dtypes checked once per public call and handed on to ``prepare``), the cache of the kernels' copies of the weights
(``PreparedNet``: a network states its ``_Net`` and builds its payload, the key and the look-up are here; ``prepare`` keeps one per module, ``weights_key`` is
what it is keyed on), and the tensor checks every public call makes before any launch."""
from __future__ import annotations

import functools
import weakref
from collections import namedtuple

import torch
import torch.nn as nn

from .ops import _Prepared, _c

EVAL_ONLY = "the native path is the eval-mode forward (BatchNorm's running statistics)"       # a ``_Net.training`` most networks with a BatchNorm share


def _tensor_checked(name, nm, t, dtype, ndim, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a torch.Tensor")
    if t.dtype != dtype or t.dim() != ndim:
        raise ValueError(f"{name}: {nm}: expected {what}, got {t.dtype} {tuple(t.shape)}")


def _cuda_checked(name, **tensors):
    for nm, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {nm} must be a CUDA tensor")


def _image_checked(name, x, img_u8, what_x, what_u8):
    """The image argument of a public call, a float32 ``x [bs, C, H, W]`` or, without one, a uint8 ``img_u8 [bs, H, W, C]``: type, dtype and rank checked
    (``what_*``: the expectation the message states).  Returns (the tensor, its argument name, H, W, C); the sizes a network allows are the caller's rules."""
    if x is not None:
        _tensor_checked(name, "x", x, torch.float32, 4, what_x)
        return x, "x", x.shape[2], x.shape[3], x.shape[1]
    _tensor_checked(name, "img_u8", img_u8, torch.uint8, 4, what_u8)
    return img_u8, "img_u8", img_u8.shape[1], img_u8.shape[2], img_u8.shape[3]


def _placed_checked(name, nm, t, ts):
    """``t`` is on a GPU, and on the one the weight tensors ``ts`` are on: the last two refusals of a public call."""
    _cuda_checked(name, **{nm: t})
    _devices_checked(name, nm, t, ts)


# What ``_validated`` needs to know of a network: ``cls`` its name in messages; ``shapes(variant)`` the public ``{key: shape}`` function; ``prefixes`` the key
# prefixes a checkpoint may carry (``nested``: or a mapping of that name inside it); ``variant(name, sd)`` reads the width / small or full / block count off
# the bare keys and raises for a missing probe key (None: one fixed structure, ``shapes()`` takes no argument and the variant is ``()``); ``training``: why a
# module in training mode is refused (None: it makes no difference); ``skip``: the key suffixes that are not float weights.
_Net = namedtuple("_Net", "cls shapes prefixes nested probes variant training skip")


@functools.lru_cache(maxsize=8)
def _keys_shapes(cls, *args):
    with torch.device("meta"):
        return tuple((k, tuple(v.shape)) for k, v in cls(*args).state_dict().items())


# One entry per (network, structure) a process meets: a dozen stage networks, the three loss networks (LPIPS in two forms) and every structure ``module_net``
# pins pass through here in one process (PTI and the pipeline), several times per step.  64 holds them all, so that no call rebuilds a table another evicted.
@functools.lru_cache(maxsize=64)
def _float_keys(net, variant):
    shapes = net.shapes() if net.variant is None else net.shapes(variant)
    return tuple((k, shape) for k, shape in shapes.items() if not k.endswith(net.skip))


def _shapes_call(net, variant):
    """The call that lists the keys ``net`` expects, as a reader can type it: ``ops_id.state_dict_shapes()``."""
    return f"{net.shapes.__module__.rpartition('.')[2]}.{net.shapes.__name__}({'' if net.variant is None else repr(variant)})"


def check_eval(name, weights, net):
    """Raises for a module in training mode, if that changes what ``net`` computes; ``name`` None: no entry in front."""
    if isinstance(weights, nn.Module) and weights.training and net.training:
        raise RuntimeError(f"{name + ': ' if name else ''}{type(weights).__name__} is in training mode; {net.training}: call .eval()")


def _validated(name, weights, net):
    """(mapping with bare keys, variant, float tensors in key order) of ``weights``: a module with the network's keys or a mapping, bare or prefixed.  Made
    once per public call (one ``state_dict()``) and handed on.  Refused, in this order: a module in training mode, anything without keys, a missing probe key,
    a missing key, a wrong shape or dtype."""
    if isinstance(weights, nn.Module):
        check_eval(name, weights, net)
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
    variant = net.variant(name, sd) if net.variant else ()
    out = []
    for k, shape in _float_keys(net, variant):
        t = sd.get(k)
        if t is None:
            raise KeyError(f"{name}: the weights lack '{k}': expected the keys of {net.cls} ({_shapes_call(net, variant)})")
        if not isinstance(t, torch.Tensor) or t.shape != shape or t.dtype != torch.float32:      # (a torch.Size is a tuple)
            raise ValueError(f"{name}: '{k}' is {getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}, expected float32 {shape}")
        out.append(t)
    return sd, variant, out


def _devices_checked(name, nm, t, ts):
    if any(w.device != t.device for w in ts):
        raise RuntimeError(f"{name}: device mismatch: {nm} on {t.device}, the weights on {sorted({str(w.device) for w in ts})}")


_MODULE_NETS = {}


def module_net(base, structure):
    """``base`` with its variant pinned to ``structure``: what a mirror module, which knows the configuration it was built with, is validated against (only a
    mapping has its structure read off its keys and shapes).  One ``_Net`` object per (base, structure), so ``_float_keys`` caches on it."""
    net = _MODULE_NETS.get((base, structure))
    if net is None:
        net = _MODULE_NETS[base, structure] = base._replace(variant=lambda name, sd: structure)
    return net


def check_loaded(name, weights, what):
    """Raises for a mirror module that still has the random weights it was built with (``_loaded`` False: an output from them would be silently wrong).
    ``what``: the weights as the message names them; ``name`` None: no entry in front."""
    if isinstance(weights, nn.Module) and getattr(weights, "_loaded", True) is False:
        raise RuntimeError(f"{name + ': ' if name else ''}{type(weights).__name__}: {what} were never loaded (nothing is downloaded here); call load_state_dict first")


def bn_shapes(out, prefix, c):
    """The five ``state_dict`` entries of a BatchNorm over ``c`` channels, added to ``out`` in their order."""
    for k in ("weight", "bias", "running_mean", "running_var"):
        out[f"{prefix}.{k}"] = (c,)
    out[prefix + ".num_batches_tracked"] = ()


def weights_key(tensors) -> tuple:
    """What the prepared copies are keyed on: storage and version of every tensor."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


_CACHES = {}                                 # cache class -> WeakKeyDictionary[module, cache]


def prepare(cache_cls, weights, *checked):
    """Prepared copies (``cache_cls().get``) for ``weights``, cached on a module; a plain mapping is prepared on every call.  ``checked``: what the
    caller's own validation of ``weights`` already produced, handed to ``get`` so that it is not made twice."""
    if not isinstance(weights, nn.Module):
        return cache_cls().get(weights, *checked)
    per_module = _CACHES.setdefault(cache_cls, weakref.WeakKeyDictionary())
    cache = per_module.get(weights)
    if cache is None:
        cache = per_module[weights] = cache_cls()
    return cache.get(weights, *checked)


def caches_of(module):
    """The caches ``prepare`` holds for ``module`` and the modules under it (``ops.invalidate_weight_caches`` empties them)."""
    return [per_module[m] for per_module in _CACHES.values() for m in module.modules() if m in per_module]


class PreparedNet(_Prepared):
    """The kernels' copies of a network's weights, cached per storage and version of every tensor, the device and ``_settings()``.  A network states
    ``_entry``, the public name its messages carry; ``_net``, its ``_Net``, or a method ``_net(weights)`` where a mirror module pins the structure; if its payload
    depends on module knobs, ``_settings()``, read at call time; and ``_build(sd, variant, dev)``: the payload from the contiguous float tensors ``sd`` by bare
    key, called under ``no_grad``."""

    __slots__ = ()
    _entry = _net = None

    def _settings(self) -> tuple:
        return ()

    def _build(self, sd, variant, dev):
        raise NotImplementedError

    def get(self, weights, checked=None):
        """The payload for ``weights``; ``checked``: what the caller's own ``_validated`` of them returned, so that it is not made twice."""
        net = self._net if isinstance(self._net, _Net) else self._net(weights)
        sd, variant, ts = checked if checked is not None else _validated(self._entry, weights, net)
        key = weights_key(ts) + (ts[0].device,) + self._settings()
        hit = self._lookup(key)
        if hit is not None:
            return hit
        sd = {k: _c(sd[k].detach(), k) for k, _ in _float_keys(net, variant)}
        with torch.no_grad():
            return self._publish(key, self._build(sd, variant, ts[0].device))
