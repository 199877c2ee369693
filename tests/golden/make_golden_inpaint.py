"""Generate g35_inpaint.npz: outputs of the reference's own ``FaceInpaintingArch`` (swap_face_fine/gcfsr_arch.py) in eval mode on the CPU with explicit seeded
noise, against the float64 model of tests/inpaint_model.py, with the seeded weights (``seeded.seeded_inpaint_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_inpaint.py [out.npz]

Only the build container has the reference tree.  The reference's module registers its classes with ``basicsr.utils.registry.ARCH_REGISTRY`` and imports
``swap_face_fine.ops.fused_act`` / ``.upfirdn2d``, which compile CUDA at import; basicsr is not installed.  This script puts ``types.ModuleType`` stubs into
``sys.modules`` before the import: the registry as tests/golden/make_golden_codeformer.py does, the two ops from the reference's own CPU fallbacks under
``swap_face_fine/gpen/face_model/op/``, loaded from where they lie (as reference_shim.py does for ``models.stylegan2.op``).  The reference's stored noise is
unusable (its buffers have the wrong resolutions, ``randomize_noise=False`` raises), so the module runs with an explicit ``noise=[...]`` list.  No weights and no
images are stored: the tests make them from the seed.  Per case of ``inpaint_model.CASES``:

    <tag>.out       the reference's float32 output; an array over 16384 elements as 4096 samples of its flat index at the odd stride <tag>.stride, with its
                    per-(sample, channel) means in <tag>.cmean
    <tag>.ref_err   the max-abs distance of the reference's whole output from the float64 model
    <tag>.share     the share of the reference's raw output values inside the hole that lie strictly inside (0, 1)
    <tag>.crc       a checksum of the network's input

``keys.default``: the reference's ``state_dict`` key names and shapes at ``out_size=256``, one ``name|d0xd1x...`` line per key.  The script asserts what
tests/test_inpaint_cpu.py asserts again from the file."""
import importlib
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import inpaint_model as M  # noqa: E402
from reference_shim import REF  # noqa: E402  (where the reference tree lies; nothing else of the shim is used)


def _load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stub_imports():
    class _Registry:
        def register(self, obj=None):
            return (lambda o: o) if obj is None else obj
    basicsr, utils, registry = (types.ModuleType(n) for n in ("basicsr", "basicsr.utils", "basicsr.utils.registry"))
    registry.ARCH_REGISTRY = _Registry()
    basicsr.utils, utils.registry = utils, registry
    sys.modules.update({"basicsr": basicsr, "basicsr.utils": utils, "basicsr.utils.registry": registry})
    gp = os.path.join(REF, "swap_face_fine", "gpen", "face_model", "op")
    fa = _load_file("_ref_gpen_fused_act", os.path.join(gp, "fused_act.py"))
    up = _load_file("_ref_gpen_upfirdn2d", os.path.join(gp, "upfirdn2d.py"))
    fused, upfirdn = types.ModuleType("swap_face_fine.ops.fused_act"), types.ModuleType("swap_face_fine.ops.upfirdn2d")
    fused.FusedLeakyReLU, fused.fused_leaky_relu, upfirdn.upfirdn2d = fa.FusedLeakyReLU, fa.fused_leaky_relu, up.upfirdn2d
    sys.modules.update({"swap_face_fine.ops.fused_act": fused, "swap_face_fine.ops.upfirdn2d": upfirdn})


def key_lines(net):
    return "\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items())


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    stub_imports()
    sys.path.insert(0, REF)
    ref = importlib.import_module("swap_face_fine.gcfsr_arch")
    assert ref.__file__.startswith(REF)
    out, worst = {}, 0.0
    out["keys.default"] = np.array(key_lines(ref.FaceInpaintingArch(out_size=256)))
    assert len(str(out["keys.default"]).split("\n")) == 122
    for tag, (size, bs) in M.CASES.items():
        c = M.case(tag)
        net = ref.FaceInpaintingArch(out_size=size).eval()
        net.load_state_dict(c["sd"], strict=True)
        assert net.num_latent == c["latent"].shape[1] and net.num_layers == len(c["noise"])
        got, latent = net(torch.from_numpy(c["x"]), torch.from_numpy(c["in_size"]).view(bs, 1), noise=[torch.from_numpy(n) for n in c["noise"]], return_latents=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == (bs, 3, size, size)
        got = got.numpy()
        e = M.max_err(got, c["want"])
        worst = max(worst, e)
        assert e <= M.bound(c["e32"], c["want"]), (tag, e, c["e32"])
        assert M.max_err(latent.numpy(), c["latent"]) <= M.bound(c["e32_latent"], c["latent"]), tag
        share = M.hole_inside_share(got, c["hole"])
        assert share >= 0.5, (tag, share)
        stride = M.sample_stride(got.size)
        out[f"{tag}.crc"] = np.uint32(zlib.crc32(c["x"].tobytes()))
        out[f"{tag}.out"] = M.stored(got)
        out[f"{tag}.stride"] = np.int64(stride)
        if stride > 1:
            out[f"{tag}.cmean"] = got.reshape(bs, 3, -1).mean(2).astype(np.float32)
        out[f"{tag}.ref_err"] = np.float64(e)
        out[f"{tag}.share"] = np.float64(share)
        v = got[np.broadcast_to(c["hole"][:, None] != 0, got.shape)]
        print(f"  {tag}: in_size {c['in_size']}, hole values mean {v.mean():.3f} std {v.std():.3f}, inside (0, 1) {share:.3f}, ref_err {e:.3e}, the float32 "
              f"model's own {c['e32']:.3e}")
    for m in M.MUTANTS:
        far = 0.0
        for tag in M.CASES:
            c = M.case(tag)
            mut = M.network(c["sd"], c["x"], c["in_size"], c["noise"], mutant=m).numpy()
            far = max(far, M.max_err(M.stored(mut), out[f"{tag}.out"]))
            if far >= M.MUTANT_MARGIN * M.PIXEL_TOL:
                break
        assert far >= M.MUTANT_MARGIN * M.PIXEL_TOL, (m, far)
        print(f"  mutant {m}: {far:.3e} from the fixture (first on {tag})")
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays; worst ref_err {worst:.3e}")
    assert size < 1_000_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g35_inpaint.npz"))
