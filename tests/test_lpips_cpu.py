"""LPIPS-AlexNet without a GPU: the drop-in criteria.lpips module's state_dict layout, the upstream-key conversion, the no-download rule, the
float64 restatement (tests/lpips_model.py) against the fixture g14 made from the reference's own classes, and the fixture's regeneration."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lpips_model as M
from conftest import GOLDEN, install_dropin, load_golden
from e4s2024_amd import ops_lpips, seeded

REF = os.environ.get("E4S_REFERENCE", "/root/reference")


@pytest.fixture(scope="module")
def g14():
    return load_golden("g14_lpips")


@pytest.fixture(scope="module")
def LPIPS():
    install_dropin()
    from criteria.lpips.lpips import LPIPS
    return LPIPS


def test_dropin_state_dict_layout_matches_reference(g14, LPIPS):
    sd = LPIPS(net_type="alex").state_dict()
    assert list(sd.keys()) == [str(k) for k in g14["keys"]] == ops_lpips.state_dict_keys()
    for (k, v), shp in zip(sd.items(), g14["shapes"]):
        assert list(v.shape) + [1] * (4 - v.dim()) == list(shp), k
    seeded_sd = seeded.seeded_lpips_state_dict(int(g14["seed"]))
    assert {k: tuple(v.shape) for k, v in seeded_sd.items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_upstream_key_conversion(LPIPS):
    from criteria.lpips.utils import convert_upstream_state_dict
    sd = seeded.seeded_lpips_state_dict(5)
    alex = {f"features.{i}.{n}": sd[f"net.layers.{i}.{n}"] for i in (0, 3, 6, 8, 10) for n in ("weight", "bias")}
    alex["classifier.1.weight"] = torch.zeros(4, 4)                  # torchvision's classifier: ignored
    lin = {f"lin{i}.model.1.weight": sd[f"lin.{i}.1.weight"] for i in range(5)}
    conv = convert_upstream_state_dict(alex, lin)
    assert list(conv.keys()) == ops_lpips.state_dict_keys()
    for k, v in sd.items():
        assert torch.allclose(conv[k].float(), v), k
    m = LPIPS()
    m.load_state_dict(conv)
    assert m._loaded


def test_no_download_and_unloaded_module_raises(LPIPS, monkeypatch):
    import torch.hub
    from criteria.lpips import utils
    from criteria.lpips.networks import get_network

    def refuse(*a, **k):
        raise AssertionError("network access attempted")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", refuse)
    monkeypatch.setattr(torch.hub, "download_url_to_file", refuse)
    with pytest.raises(RuntimeError, match="never downloaded"):
        utils.get_state_dict("alex", "0.1")
    m = LPIPS(net_type="alex", version="0.1")
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="never loaded"):
        m(x, x)
    for net in ("squeeze", "vgg"):
        with pytest.raises(NotImplementedError):
            get_network(net)
        with pytest.raises(NotImplementedError):
            LPIPS(net_type=net)


def test_unloaded_module_is_refused_by_every_entry_point(LPIPS):
    """A module that never had its weights loaded must not reach the kernels by any route: the tuning loops would optimise against its
    initial (random) parameters.  Every check happens before the network or the device is touched (nothing here needs a GPU)."""
    from e4s2024_amd import pti
    m = LPIPS()
    x = torch.zeros(1, 3, 128, 128)
    lab = torch.zeros(1, 512, 512, dtype=torch.uint8)
    calls = {
        "pti_step": lambda: pti.pti_step(None, None, None, lab, x, lpips=m),
        "style_vector_step": lambda: pti.style_vector_step(None, None, None, lab, x, lpips=m),
        "tune_clip": lambda: pti.tune_clip(None, None, x, lab, None, steps=1, lpips=m),
        "GraphedPTIStep": lambda: pti.GraphedPTIStep(None, None, None, lab, x, lpips=m),
        "lpips_multiscale": lambda: ops_lpips.lpips_multiscale(x, x, m),
        "lpips": lambda: ops_lpips.lpips(x, x, m),
        "prepare": lambda: ops_lpips.prepare(m),
        "BaseNet.forward": lambda: m.net(x),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="never loaded"):
            call()
    m.load_state_dict(seeded.seeded_lpips_state_dict(3))
    assert m._loaded and m.net._loaded
    half = LPIPS()
    half.load_state_dict({k: v for k, v in seeded.seeded_lpips_state_dict(3).items() if k.startswith("net.")}, strict=False)
    assert half.net._loaded is False and half._loaded is False
    with pytest.raises(RuntimeError, match="never loaded"):
        pti.pti_step(None, None, None, lab, x, lpips=half)


@pytest.mark.parametrize("side,factor", [(64, 1), (64, 2), (128, 1), (128, 2), (128, 4)])
def test_float64_restatement_matches_fixture(g14, side, factor):
    sd = seeded.seeded_lpips_state_dict(int(g14["seed"]))
    x, y = M.images(int(g14["seed"]), side, 1)
    loss, g = M.loss_and_grad(x, y, sd, factor)
    want = float(g14[f"loss{side}_f{factor}"])
    assert abs(loss.item() - want) <= 1e-10 * abs(want)
    wg = torch.from_numpy(g14[f"grad{side}_f{factor}"])
    assert ((g - wg).norm() / wg.norm()).item() <= 1e-10


def test_fixture_regenerates_bit_for_bit(tmp_path):
    if not os.path.isdir(REF):
        pytest.skip("the reference tree is not on this machine")
    out = tmp_path / "g14.npz"
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_golden_lpips.py"), str(out)])
    a, b = np.load(out), load_golden("g14_lpips")
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
