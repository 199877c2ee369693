import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


# ------------------------------------------------------------------------------- measured parity numbers -> $E4S_PARITY_JSON
_PARITY = {}
PARITY_ENV = "E4S_PARITY_JSON"


def record_parity(name: str, value, tol=None, note: str = ""):
    """Remember a measured parity figure (max-abs diff, flipped-pixel count ...) of the running session; at session end everything recorded
    is written as JSON to the file the environment variable E4S_PARITY_JSON names (unset: nowhere, so that a test run leaves the tree as it was)."""
    ent = {"value": (float(value) if not isinstance(value, (int, bool)) else int(value))}
    if tol is not None:
        ent["tol"] = float(tol)
    if note:
        ent["note"] = note
    _PARITY[name] = ent
    print(f"[parity] {name}: {ent['value']:.3e}" + (f" (tol {tol:.1e})" if tol is not None else "") + (f"  {note}" if note else ""))


def pytest_sessionfinish(session, exitstatus):
    path = os.environ.get(PARITY_ENV)
    if not _PARITY or not path:
        return
    doc = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "cpu", "exitstatus": int(exitstatus),
           "n": len(_PARITY), "parity": dict(sorted(_PARITY.items()))}
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    except OSError:
        pass


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session", autouse=True)
def _oracle_threads():
    """The CPU oracle on a many-core GPU host: torch's default of one thread per hardware thread (256 on the MI355X boxes) is tens of
    times slower than 16 (measured, tools/cpu_threads_probe.py); small hosts keep their default."""
    if (os.cpu_count() or 1) > 32:
        torch.set_num_threads(16)
    yield


@pytest.fixture(scope="session")
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def template_from_manifest(man):
    """manifest entry {key: [shape, dtype]} -> {key: meta tensor} usable by seeded_state_dict."""
    return {k: torch.empty(tuple(s), dtype=getattr(torch, d), device="meta") for k, (s, d) in man.items()}


@pytest.fixture(scope="session")
def net3_sd(manifest):
    """Seeded full-size Net3 state_dict (seed 4) on CPU — shared by the oracle tests."""
    from e4s2024_amd import seeded
    return seeded.seeded_state_dict(template_from_manifest(manifest["net3_1024_rli13"]), 4, "net3")


@pytest.fixture(scope="session")
def bisenet_sd(manifest):
    from e4s2024_amd import seeded
    return seeded.seeded_state_dict(template_from_manifest(manifest["bisenet_19"]), 7, "bisenet")


# ------------------------------------------------------------------------------- GPU fixtures
def install_dropin():
    import e4s2024_amd
    e4s2024_amd.install()


def default_opts(**kw):
    import argparse
    d = dict(fsencoder_type="psp", remaining_layer_idx=13, num_seg_cls=12, out_size=1024, train_G=False,
             start_from_latent_avg=True, learn_in_w=False)
    d.update(kw)
    return argparse.Namespace(**d)


@pytest.fixture(scope="session")
def gpu_net3(net3_sd):
    """The MI355X Net3 (drop-in) with the seeded weights, on cuda:0."""
    install_dropin()
    from models.networks import Net3
    from e4s2024_amd import seeded
    net = Net3(default_opts()).eval()
    net.load_state_dict(net3_sd)
    net.latent_avg = seeded.seeded_latent_avg(2, 18)
    net = net.to("cuda:0")
    net.latent_avg = net.latent_avg.to("cuda:0")
    return net
