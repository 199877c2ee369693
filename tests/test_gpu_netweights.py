"""The contract of ``netweights.PreparedNet``, which every stage network's prepared weights rest on, on a toy network of two tensors whose ``_build`` counts its
calls: one build per (storage, version, device, settings), none of the caller's validation repeated, a mapping built on every call, and
``ops.invalidate_weight_caches`` emptying it; no kernel of the library is launched there.  Then the three frozen loss networks on that contract, each at
its smallest image: one walk of the weights per public call, the cached payload, an in-place write seen."""
import pytest
import torch
import torch.nn as nn

from e4s2024_amd import netweights, ops
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
    get = lambda: netweights.prepare(PreparedToy, net)      # noqa: E731
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
    P = netweights.prepare(PreparedToy, net, checked)
    assert netweights.prepare(PreparedToy, net, checked) is P and COUNT["variant"] == seen
    assert netweights.prepare(PreparedToy, net) is P and COUNT["variant"] == seen + 1            # without it, get validates under its own entry name
    with pytest.raises(KeyError, match="toy_forward: the weights lack 'a.bias'"):
        netweights.prepare(PreparedToy, {"a.weight": net.a.weight.detach()})


def test_a_mapping_is_built_on_every_call_and_invalidate_empties_a_modules_cache():
    net = Toy().to(DEV)
    sd = {"module." + k: v.detach() for k, v in net.state_dict().items()}
    for _ in range(2):
        P, n = _builds(lambda: netweights.prepare(PreparedToy, sd))
        assert n == 1 and torch.equal(P["w2"], net.a.weight.detach() * 2)
    P, n = _builds(lambda: netweights.prepare(PreparedToy, net))
    assert n == 1 and [c.key is not None for c in netweights.caches_of(net)] == [True]
    assert ops.invalidate_weight_caches(net) == 1
    assert [c.key for c in netweights.caches_of(net)] == [None]
    again, n = _builds(lambda: netweights.prepare(PreparedToy, net))
    assert n == 1 and again is not P and torch.equal(again["w2"], P["w2"])


# ------------------------------------------------------------------------------------------------ the loss networks on the same contract
def _loss_case(which):
    """(module on the device with seeded weights, its ops module, the public call on a seeded image pair of the network's smallest size)."""
    from conftest import install_dropin
    from e4s2024_amd import ops_fp, ops_id, ops_lpips, seeded
    if which == "lpips":
        install_dropin()
        from criteria.lpips.lpips import LPIPS
        m, sd, mod, side = LPIPS(), seeded.seeded_lpips_state_dict(3), ops_lpips, 32
        call = lambda x, y: ops_lpips.lpips(x, y, m)                                          # noqa: E731
    elif which == "id":
        m, sd, mod, side = ops_id.IdNet(), seeded.seeded_irse50_state_dict(3), ops_id, 112
        call = lambda x, y: ops_id.id_loss(x, y, m)                                           # noqa: E731
    else:
        m, sd, mod, side = ops_fp.FaceParsingNet(), seeded.seeded_unet_state_dict(3), ops_fp, 512
        call = lambda x, y: ops_fp.fp_loss(x, y, m)                                           # noqa: E731
    m.load_state_dict(sd)
    x, y = (torch.tanh(torch.from_numpy(seeded.seeded_array(70 + i, "img", (1, 3, side, side), dist="normal")).float()).to(DEV) for i in range(2))
    return m.to(DEV).eval(), mod, lambda: call(x, y)


@pytest.mark.parametrize("which", ["lpips", "id", "fp"])
def test_loss_network_walks_its_weights_once_caches_them_and_sees_an_in_place_write(which):
    m, mod, call = _loss_case(which)
    walks, state_dict = [], m.state_dict
    m.state_dict = lambda *a, **k: walks.append(1) or state_dict(*a, **k)
    loss = call()
    assert len(walks) == 1                                                                    # one public call: one state_dict()
    P = mod.prepare(m)
    assert mod.prepare(m) is P and torch.equal(call(), loss) and mod.prepare(m) is P           # a cache hit: the same payload, the same bits
    assert len(walks) == 5                                                                    # and still one walk per call
    with torch.no_grad():
        next(m.parameters()).add_(0)                                                          # in place: the version moves, the values do not
    P2 = mod.prepare(m)
    assert P2 is not P and mod.prepare(m) is P2
    assert torch.equal(call(), loss)
