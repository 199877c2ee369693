"""Generate g29_vid2vid_motion.npz: outputs of the reference's own ``DenseMotionNetwork`` (swap_face_fine/face_vid2vid/modules/dense_motion.py) in eval mode on
the CPU, with the seeded weights (``seeded.seeded_dense_motion_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_vid2vid_motion.py [out.npz]

Only the build container has the reference tree.  The network is imported as ``swap_face_fine.face_vid2vid.modules.dense_motion``, never through ``drive_demo``.
Per case of ``tests/vid2vid_motion_model.py``: the keypoints (and Jacobians) the case was run with and the reference's float32 ``mask``, ``deformation`` and
``occlusion_map``.  No weights and no feature volumes are stored: the tests make them from the seed.  ``keys.dm``: the reference's ``state_dict`` key names and
shapes at the upstream ``vox-256.yaml`` configuration with the occlusion head, one ``name|d0xd1x...`` line per key.  The script asserts what
tests/test_vid2vid_motion_cpu.py asserts and, at the end, that the reference's own ``modules/generator.py`` builds its ``dense_motion_network`` from the drop-in."""
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
import vid2vid_motion_model as M  # noqa: E402

UPSTREAM = dict(block_expansion=32, num_blocks=5, max_features=1024, num_kp=15, feature_channel=32, reshape_depth=16, compress=4, estimate_occlusion_map=True)
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def key_lines(net):
    return "\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items())


def n_params(lines):
    return sum(int(np.prod([int(d) for d in ln.split("|")[1].split("x") if d])) for ln in lines if not ln.split("|")[0].endswith(BUFFERS))


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    shim.install()
    ref = importlib.import_module("swap_face_fine.face_vid2vid.modules.dense_motion")
    assert ref.__file__.startswith(shim.REF) and "swap_face_fine.face_vid2vid.drive_demo" not in sys.modules
    out = {}
    with torch.device("meta"):
        out["keys.dm"] = np.array(key_lines(ref.DenseMotionNetwork(**UPSTREAM)))
    lines = str(out["keys.dm"]).split("\n")
    assert len(lines) == 88 and n_params(lines) == 43545549, (len(lines), n_params(lines))

    for tag in M.CASES:
        c = M.case(tag)
        net = ref.DenseMotionNetwork(**M.config(tag)).eval()
        net.load_state_dict(c["sd"], strict=True)
        kd, ks = M.kp_dicts(tag)
        before = [{k: v.clone() for k, v in kp.items()} for kp in (kd, ks)]
        got = {k: v.numpy() for k, v in net(torch.from_numpy(c["feature"]), kd, ks).items()}
        assert all(torch.equal(v, was[k]) for kp, was in zip((kd, ks), before) for k, v in kp.items())
        assert set(got) == {k for k in M.OUTPUTS if k in c["out64"]}, (tag, sorted(got))
        for k, v in got.items():
            want = c["out64"][k]
            assert v.dtype == np.float32 and v.shape == want.shape, (tag, k, v.shape, want.shape)
            e = M.max_err(v, want)
            print(f"  {tag}.{k}: ref_err {e:.2e} = {e / c['e32'][k]:.2f} e32, std {want.std():.3f}")
            assert e <= M.bound(c["e32"][k], want), (tag, k, e, c["e32"][k])
            out[f"{tag}.{k}"] = v
        for k in ("kp_d", "kp_s", "jac_d", "jac_s"):
            if c[k] is not None:
                out[f"{tag}.{k}"] = c[k]
        print(f"  {tag}: {M.check_conditions(tag, got)}")
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

    # the reference's own generator builds its dense_motion_network from the drop-in, unchanged
    import e4s2024_amd
    from e4s2024_amd import ops
    e4s2024_amd.install(force=True)
    gen = importlib.import_module("swap_face_fine.face_vid2vid.modules.generator")
    assert gen.__file__.startswith(shim.REF)
    cfg = M.config("D-A")
    params = {k: cfg[k] for k in ("block_expansion", "max_features", "num_blocks", "reshape_depth", "compress")}
    g = gen.OcclusionAwareGenerator(image_channel=3, feature_channel=cfg["feature_channel"], num_kp=cfg["num_kp"], block_expansion=16, max_features=64,
                                    num_down_blocks=1, reshape_channel=8, reshape_depth=4, num_resblocks=1, estimate_occlusion_map=True,
                                    dense_motion_params=params)
    assert isinstance(g.dense_motion_network, ops.DenseMotionNetwork) and type(g.dense_motion_network).__module__.endswith("modules.dense_motion")
    assert [k[len("dense_motion_network."):] for k in g.state_dict() if k.startswith("dense_motion_network.")] == list(M.case("D-A")["sd"])
    print("  generator.py constructs the drop-in DenseMotionNetwork")


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g29_vid2vid_motion.npz"))
