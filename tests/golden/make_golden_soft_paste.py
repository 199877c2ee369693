"""Generate g18_soft_paste.npz: outputs of the reference's own ``SoftErosion``, ``Trick.get_facial_mask_from_seg19``,
``Trick.blending_two_images_with_mask`` (utils/paste_back_tricks.py) and of ``_create_masks(..., 'expansion', radius)``
(Face_swap_with_two_imgs.py:784-792) composed here from the reference's ``utils.morphology.dilation / erosion`` and its ``SoftErosion``.

    python tests/golden/make_golden_soft_paste.py [out.npz]

Only the build container has the reference tree.  ``utils/paste_back_tricks.py`` imports ``cv2.gapi`` and ``PIL.ImageQt`` at module scope without
using them on these paths; both are stubbed here (``reference_shim`` stays as the other generators use it)."""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import reference_shim as shim  # noqa: E402
from e4s2024_amd import seeded  # noqa: E402
from oracle import e4s_oracle as O  # noqa: E402

CONFIGS = ((15, 0.6, 1), (17, 0.9, 7), (5, 0.5, 2))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


def reference_modules():
    shim.install()
    cv2 = sys.modules.get("cv2")
    if cv2 is None or not hasattr(cv2, "gapi"):
        cv2 = sys.modules.setdefault("cv2", types.ModuleType("cv2"))
        cv2.__path__ = []
        cv2.gapi = sys.modules["cv2.gapi"] = types.ModuleType("cv2.gapi")
    try:
        importlib.import_module("PIL.ImageQt")
    except Exception:
        import PIL
        PIL.ImageQt = sys.modules["PIL.ImageQt"] = types.ModuleType("PIL.ImageQt")
    return importlib.import_module("utils.paste_back_tricks"), importlib.import_module("utils.morphology")


def erosion_inputs():
    """name -> float32 [1, 1, H, W]: ragged cuts of the foregrounds of seeded label maps (every 4th pixel of a 512^2 map), and one non-binary mask."""
    face = seeded.facelike_labels(5, 2)[0][::4, ::4]
    blocky = seeded.blocky_labels(3, 2)[1][::4, ::4]
    fg = lambda lab: O.foreground_mask(lab, np.zeros(lab.shape, bool))  # noqa: E731
    soft = F.interpolate(T(fg(face))[None, None, 20:84, 30:90], size=(90, 75), mode="bilinear", align_corners=True).numpy()
    return {"face_96x80": fg(face)[None, None, 16:112, 24:104], "blocky_128": fg(blocky)[None, None], "resized_90x75": soft}


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    pbt, morph = reference_modules()
    from PIL import Image
    out = {"configs": np.array(CONFIGS, dtype=np.float64)}
    for name, m in erosion_inputs().items():
        out[f"se.{name}.x"] = m.astype(np.float32) if name.startswith("resized") else m.astype(np.uint8)
        for ci, (k, thr, it) in enumerate(CONFIGS):
            soft, hard = pbt.SoftErosion(k, thr, it)(T(m.astype(np.float32)).clone())
            out[f"se.{name}.c{ci}.soft"], out[f"se.{name}.c{ci}.hard"] = soft.numpy(), hard.numpy()
            print(f"  SoftErosion{(k, thr, it)} on {name} {m.shape[-2:]}: hard share {hard.float().mean():.3f}")
    # _create_masks(..., 'expansion', radius) of Face_swap_with_two_imgs.py:784-792 with the foreground of _past_back:178-182
    lab = seeded.facelike_labels(6, 1)[0][::4, ::4].copy()
    hole = np.zeros(lab.shape, bool)
    hole[70:90, 40:70] = True
    softer = pbt.SoftErosion()
    fgm = T(O.foreground_mask(lab, hole))[None, None]
    out["exp.labels"], out["exp.hole"] = lab, hole.astype(np.uint8)
    for radius in (2, 10):
        ones = torch.ones(2 * radius + 1, 2 * radius + 1)
        full, _ = softer(morph.dilation(fgm.clone(), ones, engine="convolution"))
        ero, _ = softer(morph.erosion(fgm.clone(), ones, engine="convolution"))
        border = (full - ero).clip(0, 1)
        content, _ = softer(fgm.clone())
        out[f"exp.r{radius}.content"], out[f"exp.r{radius}.border"], out[f"exp.r{radius}.full"] = content.numpy(), border.numpy(), full.numpy()
    # get_facial_mask_from_seg19 on a 12-class map with a target size
    lab12 = seeded.facelike_labels(7, 1)[0][::8, ::8].copy()
    out["facial.labels"], out["facial.size"] = lab12, np.array([100, 90])
    out["facial.out"] = pbt.Trick.get_facial_mask_from_seg19(T(lab12).long()[None, None], target_size=(100, 90), edge_softer=pbt.SoftErosion())
    # blending_two_images_with_mask: 64 x 48 x 3, a mask with NaN
    rs = np.random.RandomState(18)
    bottom, up = rs.randint(0, 256, (64, 48, 3)).astype(np.uint8), rs.randint(0, 256, (64, 48, 3)).astype(np.uint8)
    mask = rs.rand(64, 48).astype(np.float32)
    mask[rs.rand(64, 48) < 0.05] = np.nan
    mask[rs.rand(64, 48) < 0.1] = 1.0
    mask[rs.rand(64, 48) < 0.1] = 0.0
    out["blend.bottom"], out["blend.up"], out["blend.mask"] = bottom, up, mask
    for ratio in (1.0, 0.75):
        res = pbt.Trick.blending_two_images_with_mask(Image.fromarray(bottom), Image.fromarray(up), up_ratio=ratio, up_mask=mask.copy())
        out[f"blend.out_{int(ratio * 100)}"] = np.array(res)
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"wrote {out_path}: {os.path.getsize(out_path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g18_soft_paste.npz"))
