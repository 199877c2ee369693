"""Generate g23_gpen.npz: outputs of the reference's own ``FullGenerator`` (swap_face_fine/gpen/face_model/gpen_model.py) in eval mode on the CPU, with the
seeded weights (``seeded.seeded_gpen_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_gpen.py [out.npz]

Only the build container has the reference tree.  With ``device='cpu'`` the reference's two ops take their own PyTorch fallbacks.  The inputs are not stored:
``tests/gpen_model.py`` makes them from seeds, here and in the tests; the file records a checksum of each.  Per case: the reference's float32 output and
``ref_err``, that output against the float64 model; for one case its latents.  ``keys.default``: the reference's ``state_dict`` key names and shapes at
``GPEN-BFR-512``'s configuration (512, 512, 8, 2, narrow 1), one ``name|d0xd1x...`` line per key.  The script asserts what tests/test_gpen_cpu.py asserts."""
import importlib
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_shim as shim  # noqa: E402
import gpen_model as GM  # noqa: E402


def key_lines(net):
    return "\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items())


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    shim.install()
    ref = importlib.import_module("swap_face_fine.gpen.face_model.gpen_model")
    out, worst = {}, 0.0
    with torch.device("meta"):
        out["keys.default"] = np.array(key_lines(ref.FullGenerator(512, 512, 8, channel_multiplier=2, narrow=1)))
    assert len(str(out["keys.default"]).split("\n")) == 163
    for tag, (size, narrow, sdim, bs) in GM.CASES.items():
        c = GM.case(tag)
        net = ref.FullGenerator(size, sdim, GM.N_MLP, channel_multiplier=2, narrow=narrow, device="cpu").eval()
        net.load_state_dict(c["sd"], strict=True)
        got, latent = net(torch.from_numpy(c["x"]), return_latents=True)
        assert got.dtype == torch.float32 and tuple(got.shape) == (bs, 3, size, size) and tuple(latent.shape) == (bs, 2 * int(np.log2(size)) - 2, sdim)
        got = got.numpy()
        e = GM.max_err(got, c["want"])
        worst = max(worst, e)
        assert e <= GM.bound(c["e32"], c["want"]), (tag, e, c["e32"])
        assert 0.3 <= got.std() <= 0.5 and (np.abs(got) >= 1).mean() <= 0.05, (tag, got.std())
        assert GM.strict_pixels(c["u"], c["e32"]).mean() >= 0.99
        out[f"{tag}.crc"] = np.uint32(zlib.crc32(c["x"].tobytes()))
        out[f"{tag}.out"] = got
        out[f"{tag}.ref_err"] = np.float64(e)
        if tag == GM.LATENT_CASE:
            out[f"{tag}.latent"] = latent.numpy()
            assert GM.max_err(latent.numpy(), c["latent"]) <= GM.bound(c["e32_latent"], c["latent"])
        print(f"  {tag}: output std {got.std():.3f}, outside (-1, 1) {(np.abs(got) >= 1).mean():.3f}, ref_err {e:.3e}, the float32 model's own {c['e32']:.3e}")
    for m in GM.MUTANTS:
        far = max(GM.max_err(GM.network(GM.case(tag)["sd"], GM.case(tag)["x"], mutant=m).numpy(), out[f"{tag}.out"]) for tag in GM.CASES)
        assert far >= GM.MUTANT_MARGIN * GM.PIXEL_TOL, (m, far)
        print(f"  mutant {m}: {far:.3e} from the fixture")
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays; worst ref_err {worst:.3e}")
    assert size < 1_000_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g23_gpen.npz"))
