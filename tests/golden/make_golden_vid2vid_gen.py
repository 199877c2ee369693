"""Generate g30_vid2vid_gen.npz: outputs of the reference's own ``OcclusionAwareSPADEGenerator`` (swap_face_fine/face_vid2vid/modules/generator.py) in eval mode
on the CPU, with the seeded weights (``seeded.seeded_generator_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_vid2vid_gen.py [out.npz]

Only the build container has the reference tree.  The class is imported as ``swap_face_fine.face_vid2vid.modules.generator`` through ``reference_shim``, never
through ``drive_demo``, and the package's drop-ins are not installed: every block is the reference's own.  Where a case's front is not 256 wide the fixed-width
``decoder`` is replaced by ``nn.Identity()`` after construction, so that ``prediction`` is the warped feature; ``feature_3d`` is read with a forward hook on
``resblocks_3d``.  Per case of ``tests/vid2vid_gen_model.py``: the keypoints (and Jacobians) it was run with and the float32 outputs ``STORED`` names.  G-D is
three calls of the reference, one per driving keypoint set, with the one source.  ``<tag>.ref.<name>``: the figures of the reference's own intermediates
(forward hooks on every ``norm1``, on ``third.norm`` and in front of every ``InstanceNorm2d``) that the conditions are held to.  No weights and no images are stored: the tests make them from the seed.
``keys.gen``: the reference's ``state_dict`` key names and shapes at the upstream ``vox-256.yaml`` configuration, one ``name|d0xd1x...`` line per key.  The script
asserts what tests/test_vid2vid_gen_cpu.py asserts."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_shim as shim  # noqa: E402
import vid2vid_gen_model as M  # noqa: E402

UPSTREAM = dict(image_channel=3, feature_channel=32, num_kp=15, block_expansion=64, max_features=512, num_down_blocks=2, reshape_channel=32, reshape_depth=16,
                num_resblocks=6, estimate_occlusion_map=True, estimate_jacobian=False,
                dense_motion_params=dict(block_expansion=32, max_features=1024, num_blocks=5, reshape_depth=16, compress=4))
BUFFERS = ("running_mean", "running_var", "num_batches_tracked", "weight_u", "weight_v")
UPSTREAM_KEYS, UPSTREAM_PARAMS = 386, 100_988_176


def key_lines(net):
    return "\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items())


def n_params(lines):
    return sum(int(np.prod([int(d) for d in ln.split("|")[1].split("x") if d])) for ln in lines if not ln.split("|")[0].endswith(BUFFERS))


def run_reference(ref, tag):
    """The reference's outputs of a case as float32 arrays, by the names of ``M.OUTPUTS``."""
    c = M.case(tag)
    net = ref.OcclusionAwareSPADEGenerator(**M.config(tag)).eval()
    if not M.CASES[tag][6]:
        net.decoder = torch.nn.Identity()
    net.load_state_dict(c["sd"], strict=True)
    held, stats = {}, {"norm1_zero": [], "third": [], "plane_var": []}
    net.resblocks_3d.register_forward_hook(lambda mod, inp, out: held.__setitem__("feature_3d", out.detach().clone()))
    # the intermediates the conditions are held to, from the reference's own layers: what the ReLU behind every norm1 zeroes, the signs in front of third's
    # LeakyReLU, the planes every instance norm of the decoder sees
    for block in net.resblocks_3d:
        block.norm1.register_forward_hook(lambda mod, inp, out: stats["norm1_zero"].append(float((out <= 0).double().mean())))
    net.third.norm.register_forward_hook(lambda mod, inp, out: stats["third"].append((float((out > 0).double().mean()), float((out < 0).double().mean()))))

    def planes(mod, inp):
        v = inp[0].double().var(dim=(2, 3), unbiased=False)
        stats["plane_var"].append(float((v / v.mean()).min()))

    for mod in net.decoder.modules():
        if isinstance(mod, torch.nn.InstanceNorm2d):
            mod.register_forward_pre_hook(planes)
    n = c["kp_d"].shape[0]
    source = torch.from_numpy(c["source"])
    calls = [slice(None)] if source.shape[0] == n else [slice(i, i + 1) for i in range(n)]        # G-D: one call per driving keypoint set
    parts = []
    for rows in calls:
        kd, ks = M.kp_dicts(tag, rows=rows)
        before = [{k: v.clone() for k, v in kp.items()} for kp in (kd, ks)]
        got = dict(net(source, kd, ks))
        assert all(torch.equal(v, was[k]) for kp, was in zip((kd, ks), before) for k, v in kp.items())
        got["feature_3d"] = held.pop("feature_3d")
        # the reference's output_dict has no deformation: it is the dense-motion network's, run again on the hooked feature (deterministic on the CPU)
        dm = net.dense_motion_network(feature=got["feature_3d"], kp_driving=kd, kp_source=ks)
        assert torch.equal(dm["mask"], got["mask"])
        got["deformation"] = dm["deformation"]
        if M.CASES[tag][6]:
            assert got["prediction"].shape[1] == 3
        else:
            got["feature"] = got.pop("prediction")
        parts.append(got)
    out = {k: torch.cat([p[k] for p in parts]).numpy() for k in parts[0] if k != "feature_3d"}
    out["feature_3d"] = parts[0]["feature_3d"].numpy()
    assert all(torch.equal(p["feature_3d"], parts[0]["feature_3d"]) for p in parts)
    nres = len(net.resblocks_3d)
    assert len(stats["norm1_zero"]) == nres * len(calls) and len(stats["third"]) == len(calls) and bool(stats["plane_var"]) == M.CASES[tag][6]
    ref = {"norm1_zero": np.array(stats["norm1_zero"][:nres]),               # the source-only part: the same in every call
           "third": np.array(stats["third"]).min(0)}                        # the smaller share of each sign over the calls
    if stats["plane_var"]:
        ref["plane_var"] = np.array([min(stats["plane_var"])])
    return out, ref


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    shim.install()
    ref = importlib.import_module("swap_face_fine.face_vid2vid.modules.generator")
    assert ref.__file__.startswith(shim.REF) and "swap_face_fine.face_vid2vid.drive_demo" not in sys.modules
    assert sys.modules["swap_face_fine.face_vid2vid.modules.dense_motion"].__file__.startswith(shim.REF)
    out = {}
    with torch.device("meta"):
        out["keys.gen"] = np.array(key_lines(ref.OcclusionAwareSPADEGenerator(**UPSTREAM)))
    lines = str(out["keys.gen"]).split("\n")
    print(f"  upstream: {len(lines)} keys, {n_params(lines)} parameters")
    assert len(lines) == UPSTREAM_KEYS and n_params(lines) == UPSTREAM_PARAMS, (len(lines), n_params(lines))

    for tag in M.CASES:
        c = M.case(tag)
        got, ref_stats = run_reference(ref, tag)
        assert set(got) == set(c["out64"]) - ({"feature"} if M.CASES[tag][6] else set()), (tag, sorted(got))
        for k, v in got.items():
            want = c["out64"][k]
            assert v.dtype == np.float32 and v.shape == want.shape, (tag, k, v.shape, want.shape)
            e = M.max_err(v, want)
            print(f"  {tag}.{k}: ref_err {e:.2e} = {e / c['e32'][k]:.2f} e32, std {want.std():.3f}")
            assert e <= M.bound(c["e32"][k], want), (tag, k, e, c["e32"][k])
            if k in M.STORED[tag]:
                out[f"{tag}.{k}"] = v
        for k in ("kp_d", "kp_s", "jac_d", "jac_s"):
            if c[k] is not None:
                out[f"{tag}.{k}"] = c[k]
        for k, v in ref_stats.items():
            out[f"{tag}.ref.{k}"] = v
        print(f"  {tag}: {M.check_conditions(tag, got, ref_stats)}")
        M.check_conditions(tag, c["out64"])

    for m, (tag, name) in M.MUTANTS.items():
        c = M.case(tag)
        bars = M.max_err(M.mutant_output(m), out[f"{tag}.{name}"]) / M.bound(c["e32"][name], c["out64"][name])
        print(f"  mutant {m} on {tag}.{name}: {bars:.0f} bars from the fixture")
        assert bars >= M.MUTANT_MARGIN, (m, bars)
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays")
    assert size < 300_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g30_vid2vid_gen.npz"))
