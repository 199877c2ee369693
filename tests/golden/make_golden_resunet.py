"""Generate g21_resunet.npz: outputs of the reference's own ``ResUNet`` (swap_face_fine/Blender/model_center/res_u_net.py) in eval mode on the CPU, with the
seeded weights (``seeded.seeded_resunet_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_resunet.py [out.npz]

Only the build container has the reference tree.  ``res_u_net.py`` imports ``torchvision.models`` and does not use it: it is stubbed.  The inputs are not
stored: ``tests/resunet_model.py`` makes them from seeds, here and in the tests; the file records a checksum of each.  Per case: the reference's float32
output (at 256 x 256 its values at 8192 seeded positions), and ``ref_err``, that output against the float64 model.  Per width: the reference's
``state_dict`` key names and shapes, one ``name|d0xd1x...`` line per key."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_shim as shim  # noqa: E402
import resunet_model as RM  # noqa: E402


def reference_module():
    shim.install()
    tv = sys.modules["torchvision"]
    if not hasattr(tv, "models"):
        tv.models = types.ModuleType("torchvision.models")
        sys.modules["torchvision.models"] = tv.models
    return importlib.import_module("swap_face_fine.Blender.model_center.res_u_net")


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = reference_module()
    out, nets, worst = {}, {}, 0.0
    for width in (64, 16):
        net = ref.ResUNet(types.SimpleNamespace(small_FPN=width == 16)).eval()
        out[f"keys.w{width}"] = np.array("\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items()))
        net.load_state_dict(RM.state_dict(width), strict=True)
        nets[width] = net
    for tag, (H, W, bs, width) in RM.CASES.items():
        x = RM.case_inputs(tag)
        got = nets[width](torch.from_numpy(x))
        assert got.dtype == torch.float32 and tuple(got.shape) == (bs, 3, H, W)
        got = got.numpy()
        e = RM.max_err(got, RM.reference_output(tag))
        worst = max(worst, e)
        out[f"{tag}.crc"] = RM.crc(x)
        out[f"{tag}.out"] = got.reshape(-1)[RM.sample_positions(tag)] if tag in RM.SAMPLED else got
        out[f"{tag}.ref_err"] = np.float64(e)
        print(f"  {tag}: output std {got.std():.3f}, ref_err {e:.3e}, the float32 model's own {RM.e32(tag):.3e}")
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays; worst ref_err {worst:.3e}")
    assert size < 1_000_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g21_resunet.npz"))
