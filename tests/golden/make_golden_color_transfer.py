"""Generate g19_color_transfer.npz: outputs of the reference's own ``utils.morphology.dilation / erosion(engine='convolution')`` on float masks and of
``swap_face_fine.color_transfer.skin_color_transfer(src, trg, 'lct' | 'mkl')``, called the way ``_color_transfer`` calls it
(Face_swap_with_two_imgs.py:555-565).

    python tests/golden/make_golden_color_transfer.py [out.npz]

Only the build container has the reference tree.  ``swap_face_fine/color_transfer.py`` imports ``cv2`` and ``numexpr`` at module scope; neither is used
by the two modes pinned here and both are stubbed (matplotlib and scipy are installed).  The inputs are not stored: ``tests/colortransfer_model.py``
makes them from seeds, here and in the tests; the file records a checksum of each."""
import importlib
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

import reference_shim as shim  # noqa: E402
import colortransfer_model as CM  # noqa: E402

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
LAMBDA_MIN = 4e-3


def reference_modules():
    shim.install()
    for name in ("cv2", "numexpr"):
        if name not in sys.modules or not hasattr(sys.modules[name], "__file__"):
            sys.modules.setdefault(name, types.ModuleType(name))
    import matplotlib
    matplotlib.use("Agg")
    return importlib.import_module("swap_face_fine.color_transfer"), importlib.import_module("utils.morphology")


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ct, morph = reference_modules()
    out = {}
    # (a) grey dilation / erosion of float masks at ragged shapes
    for shape, radii in CM.MORPH_SHAPES:
        x = CM.morph_input(shape)
        tag = "x".join(str(v) for v in shape)
        out[f"morph.{tag}.crc"] = crc(x)
        assert (x == 0).any() and (x == 1).any() and ((x > 0) & (x < 1)).any()
        for r in radii:
            ones = torch.ones(2 * r + 1, 2 * r + 1)
            out[f"morph.{tag}.r{r}.dilate"] = morph.dilation(T(x).clone(), ones, engine="convolution").numpy()
            out[f"morph.{tag}.r{r}.erode"] = morph.erosion(T(x).clone(), ones, engine="convolution").numpy()
            print(f"  morphology {tag} r={r}: dilate mean {out[f'morph.{tag}.r{r}.dilate'].mean():.3f}, erode mean {out[f'morph.{tag}.r{r}.erode'].mean():.3f}")
    # (b) skin_color_transfer on seeded pairs, as _color_transfer calls it
    lam = np.zeros((CM.CT_PAIRS, 2, 3))
    for i in range(CM.CT_PAIRS):
        d, t, md, mt = CM.ct_pair(i)
        out[f"ct.p{i}.crc"] = crc(d, t, md, mt)
        src, trg = np.array(d * md) / 255., np.array(t * mt) / 255.
        assert src.dtype == np.float32 and np.array_equal(src, CM.inner(d, md))
        for j, v in enumerate((src, trg)):
            lam[i, j] = np.linalg.eigvalsh(np.cov(v.reshape(-1, 3).astype(np.float64).T))
        print(f"  pair {i}: mask means {md.mean():.3f} / {mt.mean():.3f}, covariance eigenvalues src {lam[i, 0]}, trg {lam[i, 1]}")
        for mode in CM.MODES:
            res = ct.skin_color_transfer(src.copy(), trg.copy(), ct_mode=mode)
            assert res.dtype == np.float32, res.dtype
            out[f"ct.p{i}.{mode}.q"] = np.uint8(res)
    assert lam.min() >= LAMBDA_MIN, f"smallest covariance eigenvalue {lam.min():.3e} < {LAMBDA_MIN}: change the inputs"
    out["ct.eigenvalues"] = lam
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays; smallest eigenvalue {lam.min():.3e}")
    assert size < 1_000_000


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g19_color_transfer.npz"))
