"""What the stage networks share on the host, without a GPU: ``netweights.module_net`` / ``check_loaded`` / ``bn_shapes`` and ``lossnet.fold_conv_bn`` /
``prep_exact`` (plain torch).  The messages are the ones ``ops_gpen``, ``ops_parsenet``, ``ops_retinaface`` and ``ops_reenact`` raise, written out here."""
import pytest
import torch
import torch.nn as nn

from e4s2024_amd import lossnet, netweights
from e4s2024_amd.netweights import _Net, _validated, bn_shapes, check_loaded, module_net


def _toy_shapes(variant):
    return {"a.weight": (variant, 2), "a.bias": (variant,)}


def _toy_variant(name, sd):
    return int(sd["a.weight"].shape[0])


TOY = _Net("Toy", _toy_shapes, ("module.",), False, ("a.weight",), _toy_variant, None, ())


def test_module_net_is_one_object_per_structure_and_pins_the_variant():
    assert module_net(TOY, 3) is module_net(TOY, 3)
    assert module_net(TOY, 3) is not module_net(TOY, 4) and module_net(TOY, 3) is not TOY
    other = TOY._replace(cls="Other")
    assert module_net(other, 3) is not module_net(TOY, 3)                                     # the cache is per base, too
    pinned = module_net(TOY, 3)
    assert pinned._replace(variant=None) == TOY._replace(variant=None)                        # nothing but the variant differs
    sd = {"a.weight": torch.zeros(5, 2), "a.bias": torch.zeros(5)}
    assert TOY.variant("toy", sd) == 5 and pinned.variant("toy", sd) == 3 and pinned.variant("toy", {}) == 3
    assert _validated("toy", sd, TOY)[1] == 5
    with pytest.raises(ValueError, match=r"'a.weight' is torch.float32 \(5, 2\), expected float32 \(3, 2\)"):
        _validated("toy", sd, pinned)                                                         # the mapping's own shapes are held to the pinned structure


class _Loaded(nn.Module):
    def __init__(self, loaded):
        super().__init__()
        self._loaded = loaded


@pytest.mark.parametrize("name, what, message", [
    (None, "the GPEN weights", "_Loaded: the GPEN weights were never loaded (nothing is downloaded here); call load_state_dict first"),
    ("parsenet_mask", "the ParseNet weights",
     "parsenet_mask: _Loaded: the ParseNet weights were never loaded (nothing is downloaded here); call load_state_dict first"),
    ("retinaface_detect", "the RetinaFace weights",
     "retinaface_detect: _Loaded: the RetinaFace weights were never loaded (nothing is downloaded here); call load_state_dict first"),
    ("kp_detector_forward", "the weights", "kp_detector_forward: _Loaded: the weights were never loaded (nothing is downloaded here); call load_state_dict first"),
])
def test_check_loaded_raises_each_modules_message(name, what, message):
    with pytest.raises(RuntimeError) as e:
        check_loaded(name, _Loaded(False), what)
    assert str(e.value) == message
    check_loaded(name, _Loaded(True), what)
    check_loaded(name, nn.Linear(2, 2), what)                                                 # a module that keeps no such flag
    check_loaded(name, {"a.weight": torch.zeros(1)}, what)                                    # a mapping


def test_ops_gpen_check_loaded_keeps_its_message_and_returns_the_weights():
    from e4s2024_amd import ops_gpen
    sd = {}
    assert ops_gpen.check_loaded(sd) is sd
    with pytest.raises(RuntimeError) as e:
        ops_gpen.check_loaded(_Loaded(False))
    assert str(e.value) == "_Loaded: the GPEN weights were never loaded (nothing is downloaded here); call load_state_dict first"


def test_bn_shapes_gives_the_five_keys_in_state_dict_order():
    out = {"conv.weight": (7, 3, 1, 1)}
    bn_shapes(out, "bn", 7)
    bn = nn.BatchNorm2d(7)
    assert list(out)[1:] == ["bn." + k for k in bn.state_dict()]
    assert [out["bn." + k] for k in bn.state_dict()] == [tuple(v.shape) for v in bn.state_dict().values()]
    assert netweights.EVAL_ONLY == "the native path is the eval-mode forward (BatchNorm's running statistics)"


def test_fold_conv_bn_is_the_float64_formula():
    g = torch.Generator().manual_seed(5)
    c = 6
    sd = {"conv.bias": torch.randn(c, generator=g), "bn.weight": torch.randn(c, generator=g), "bn.bias": torch.randn(c, generator=g),
          "bn.running_mean": torch.randn(c, generator=g), "bn.running_var": torch.rand(c, generator=g) + 0.1}
    sd["bn.weight"][2] = 0.0                                                                  # a channel the BatchNorm switches off
    assert all(v.dtype == torch.float32 for v in sd.values())
    scale, shift = lossnet.fold_conv_bn(sd, "conv", "bn")
    s = sd["bn.weight"].double() / torch.sqrt(sd["bn.running_var"].double() + lossnet.BN_EPS)
    want = (sd["bn.bias"].double() - sd["bn.running_mean"].double() * s) + sd["conv.bias"].double() * s
    assert scale.dtype == shift.dtype == torch.float64
    assert torch.equal(scale, s) and torch.equal(shift, want)
    assert scale[2] == 0 and shift[2] == sd["bn.bias"][2].double()
    x = torch.randn(4, c, generator=g, dtype=torch.float64)                                   # and it is the BatchNorm of conv(x) + bias
    bn = (x + sd["conv.bias"].double() - sd["bn.running_mean"].double()) / torch.sqrt(sd["bn.running_var"].double() + lossnet.BN_EPS) \
        * sd["bn.weight"].double() + sd["bn.bias"].double()
    assert torch.allclose(x * scale + shift, bn, rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", [(5, 3, 7, 7), (4, 2, 1, 1)])
@pytest.mark.parametrize("scaled", [False, True])
def test_prep_exact_is_the_k_major_layout_bit_for_bit(shape, scaled):
    g = torch.Generator().manual_seed(shape[0])
    cout, cin, k, _ = shape
    w = torch.randn(shape, generator=g)
    scale = torch.randn(cout, generator=g, dtype=torch.float64) if scaled else None
    shift = torch.randn(cout, generator=g, dtype=torch.float64)
    wt, bias = lossnet.prep_exact(w, scale, shift)
    folded = (w.double() * scale[:, None, None, None]).float() if scaled else w
    assert wt.shape == (cin, k * k, cout) and wt.dtype == torch.float32 and wt.is_contiguous()
    assert torch.equal(wt, folded.permute(1, 2, 3, 0).reshape(cin, k * k, cout))
    assert wt[cin - 1, k * k - 1, 1] == folded[1, cin - 1, k - 1, k - 1]
    assert bias.dtype == torch.float32 and torch.equal(bias, shift.float())
    assert lossnet.prep_exact(w, scale)[1] is None
