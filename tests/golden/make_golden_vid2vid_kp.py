"""Generate g28_vid2vid_kp.npz: outputs of the reference's own ``KPDetector`` and ``HEEstimator`` (swap_face_fine/face_vid2vid/modules/keypoint_detector.py) in
eval mode on the CPU, with the seeded weights (``seeded.seeded_kp_detector_state_dict`` / ``seeded_he_estimator_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_vid2vid_kp.py [out.npz]

Only the build container has the reference tree.  The networks are imported as ``swap_face_fine.face_vid2vid.modules.keypoint_detector``, never through
``drive_demo`` (which needs imageio and skimage).  Per K and H case of ``tests/vid2vid_kp_model.py``: the uint8 input ``img`` (the float32 image is ``img / 255``)
and the reference's float32 outputs (``value``, ``jacobian``; the five heads); for case K-A alone also, by forward hooks, the ``prediction`` logits and the
normalised heatmap.  No weights are stored: the tests make them from the seed.  ``keys.kp`` / ``keys.he``: the reference's ``state_dict`` key names and shapes at
the upstream ``vox-256.yaml`` configuration, one ``name|d0xd1x...`` line per key (a scalar has no dimensions).  The script asserts what
tests/test_vid2vid_kp_cpu.py asserts."""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_shim as shim  # noqa: E402
import vid2vid_kp_model as M  # noqa: E402

UPSTREAM_KP = dict(block_expansion=32, feature_channel=32, num_kp=15, image_channel=3, max_features=1024, reshape_channel=16384, reshape_depth=16, num_blocks=5,
                   temperature=0.1, estimate_jacobian=False, scale_factor=0.25)
UPSTREAM_HE = dict(block_expansion=64, feature_channel=32, num_kp=15, image_channel=3, max_features=2048, num_bins=66, estimate_jacobian=False)


def key_lines(net):
    return "\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items())


def n_params(lines):
    """Parameters, not buffers: without the running statistics, ``num_batches_tracked`` and the anti-alias kernel ``down.weight``."""
    buffers = ("running_mean", "running_var", "num_batches_tracked", "down.weight")
    return sum(int(np.prod([int(d) for d in ln.split("|")[1].split("x") if d])) for ln in lines if not ln.split("|")[0].endswith(buffers))


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    shim.install()
    ref = importlib.import_module("swap_face_fine.face_vid2vid.modules.keypoint_detector")
    assert "swap_face_fine.face_vid2vid.drive_demo" not in sys.modules
    out = {}
    with torch.device("meta"):
        out["keys.kp"] = np.array(key_lines(ref.KPDetector(**UPSTREAM_KP)))
        out["keys.he"] = np.array(key_lines(ref.HEEstimator(**UPSTREAM_HE)))
    kp_lines, he_lines = str(out["keys.kp"]).split("\n"), str(out["keys.he"]).split("\n")
    assert len(kp_lines) == 75 and n_params(kp_lines) == 41940047, (len(kp_lines), n_params(kp_lines))
    assert len(he_lines) == 402 and n_params(he_lines) == 30254838, (len(he_lines), n_params(he_lines))
    assert "down.weight|3x1x13x13" in kp_lines

    for tag in list(M.KP_CASES) + list(M.HE_CASES):
        c = M.case(tag)
        kp = tag in M.KP_CASES
        net = (ref.KPDetector(**M.kp_config(tag)) if kp else ref.HEEstimator(**M.he_config(tag), estimate_jacobian=False)).eval()
        net.load_state_dict(c["sd"], strict=True)
        seen = {}
        if kp:      # the logits are the kp head's output; the heatmap is the softmax the module takes of them
            net.kp.register_forward_hook(lambda mod, inp, res: seen.__setitem__("prediction", res.detach().numpy().copy()))
        x = torch.from_numpy(c["x"])
        got = {k: v.numpy() for k, v in net(x).items()}
        heat = None
        if kp:
            p = torch.from_numpy(seen["prediction"])
            heat = F.softmax(p.view(p.shape[0], p.shape[1], -1) / net.temperature, dim=2).view(p.shape).numpy()
            got["prediction"], got["heatmap"] = seen["prediction"], heat
        for k in (M.KP_OUTPUTS + ("prediction", "heatmap")) if kp else M.HE_OUTPUTS:
            want = c["out64"].get(k)
            if want is None:
                assert k not in got
                continue
            assert got[k].dtype == np.float32 and got[k].shape == want.shape, (tag, k, got[k].shape, want.shape)
            e = M.max_err(got[k], want)
            assert e <= M.bound(c["e32"][k], want), (tag, k, e, c["e32"][k])
            print(f"  {tag}.{k}: ref_err {e:.2e} = {e / c['e32'][k]:.2f} e32, std {want.std():.3f}")
            if k not in ("prediction", "heatmap") or tag == M.STORED_VOLUME:
                out[f"{tag}.{k}"] = got[k]
        out[f"{tag}.img"] = c["img"]
        print(f"  {tag}: {M.check_conditions(tag, got, heat)}")
        M.check_conditions(tag, c["out64"], c["out64"].get("heatmap"))

    for tag in M.T_CASES:      # the transformation of the float64 model on the reference's stored head outputs: what the GPU test is held to
        c = M.case(tag)
        he_tag, kp_tag, _ = M.T_CASES[tag]
        if he_tag != "hand":
            he = {k: out[f"{he_tag}.{k}"] for k in M.HE_OUTPUTS}
            n = c["kp"].shape[0]
            t = M.transform_outputs(c, he=he, kp=out[f"{kp_tag}.value"][:n], jac=None if c["jac"] is None else out[f"{kp_tag}.jacobian"][:n])
            for k, v in t["e32"].items():
                assert v <= 1e-4 * t["out64"][k].std(), (tag, k)
        print(f"  {tag}: {M.check_conditions(tag, None)} degrees {c['out64']['deg'].min():.1f} .. {c['out64']['deg'].max():.1f}")
    hand = M.case("T-hand")["out64"]["deg"]
    assert hand.min() <= -55 and hand.max() >= 55, hand

    for m, (tag, name) in M.MUTANTS.items():
        c = M.case(tag)
        if tag in M.T_CASES:
            want, e32 = c["out64"][name], c["e32"][name]
        else:
            want, e32 = out[f"{tag}.{name}"], c["e32"][name]
        bars = M.max_err(M.mutant_output(m), want) / M.bound(e32, c["out64"][name])
        print(f"  mutant {m} on {tag}.{name}: {bars:.0f} bars from the fixture")
        assert bars >= M.MUTANT_MARGIN, (m, bars)
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays")
    assert size < 300_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g28_vid2vid_kp.npz"))
