"""The contract of ``netweights.PreparedNet``, which every stage network's prepared weights rest on, on a toy network of two tensors whose ``_build`` counts its
calls: one build per (storage, version, device, settings), none of the caller's validation repeated, a mapping built on every call, and
``ops.invalidate_weight_caches`` emptying it.  No kernel of the library is launched."""
import pytest
import torch
import torch.nn as nn

from e4s2024_amd import lossnet, ops
from e4s2024_amd.netweights import PreparedNet, _Net, _validated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNT = {"build": 0, "variant": 0}
KNOB = ["a"]


def _shapes(variant):
    return {"a.weight": (variant, 2), "a.bias": (variant,)}


def _variant(name, sd):
    COUNT["variant"] += 1                                                                     # one per _validated
    return int(sd["a.weight"].shape[0])


TOY = _Net("Toy", _shapes, ("module.",), False, ("a.weight",), _variant, None, ())


class PreparedToy(PreparedNet):
    __slots__ = ()
    _entry, _net = "toy_forward", TOY

    def _settings(self):
        return (KNOB[0],)

    def _build(self, sd, variant, dev):
        COUNT["build"] += 1
        assert not torch.is_grad_enabled() and list(sd) == ["a.weight", "a.bias"] and dev == sd["a.weight"].device
        return dict(w2=sd["a.weight"] * 2, variant=variant, knob=KNOB[0])


class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(2, 3)


def _builds(fn):
    before = COUNT["build"]
    out = fn()
    return out, COUNT["build"] - before


def test_one_build_per_weights_device_and_settings():
    net = Toy().to(DEV)
    get = lambda: lossnet.prepare(PreparedToy, net)      # noqa: E731
    P, n = _builds(get)
    assert n == 1 and P["variant"] == 3 and torch.equal(P["w2"], net.a.weight.detach() * 2)
    for _ in range(3):
        again, n = _builds(get)
        assert n == 0 and again is P                                                          # repeated gets: the cached payload
    with torch.no_grad():
        net.a.weight.add_(1.0)                                                                # in place: the version moves
    P2, n = _builds(get)
    assert n == 1 and torch.equal(P2["w2"], net.a.weight.detach() * 2) and not torch.equal(P2["w2"], P["w2"])
    net.a.weight = nn.Parameter(net.a.weight.detach().clone() + 1.0)                          # replaced: new storage
    P3, n = _builds(get)
    assert n == 1 and torch.equal(P3["w2"], net.a.weight.detach() * 2)
    KNOB[0] = "b"                                                                             # a module knob in the key, read at call time
    try:
        P4, n = _builds(get)
        assert n == 1 and P4["knob"] == "b" and _builds(get)[1] == 0
    finally:
        KNOB[0] = "a"
    assert _builds(get)[1] == 1


def test_checked_weights_are_not_validated_again():
    net = Toy().to(DEV)
    checked = _validated("toy_forward", net, TOY)
    seen = COUNT["variant"]
    P = lossnet.prepare(PreparedToy, net, checked)
    assert lossnet.prepare(PreparedToy, net, checked) is P and COUNT["variant"] == seen
    assert lossnet.prepare(PreparedToy, net) is P and COUNT["variant"] == seen + 1            # without it, get validates under its own entry name
    with pytest.raises(KeyError, match="toy_forward: the weights lack 'a.bias'"):
        lossnet.prepare(PreparedToy, {"a.weight": net.a.weight.detach()})


def test_a_mapping_is_built_on_every_call_and_invalidate_empties_a_modules_cache():
    net = Toy().to(DEV)
    sd = {"module." + k: v.detach() for k, v in net.state_dict().items()}
    for _ in range(2):
        P, n = _builds(lambda: lossnet.prepare(PreparedToy, sd))
        assert n == 1 and torch.equal(P["w2"], net.a.weight.detach() * 2)
    P, n = _builds(lambda: lossnet.prepare(PreparedToy, net))
    assert n == 1 and [c.key is not None for c in lossnet.caches_of(net)] == [True]
    assert ops.invalidate_weight_caches(net) == 1
    assert [c.key for c in lossnet.caches_of(net)] == [None]
    again, n = _builds(lambda: lossnet.prepare(PreparedToy, net))
    assert n == 1 and again is not P and torch.equal(again["w2"], P["w2"])
