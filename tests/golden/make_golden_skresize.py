"""Generate g34_skresize.npz: what ``scipy.ndimage`` gives for the body of ``skimage.transform.resize(img / 255.0, (Ho, Wo))`` on the small cases of
tests/skresize_model.py.

    python tests/golden/make_golden_skresize.py [out.npz]
    python tests/golden/make_golden_skresize.py --seeds      (per seed, how many float32 values of the model differ from scipy's: how CASE_SEED was chosen)

This is skimage's ``resize`` body RESTATED, not skimage run: skimage is installed nowhere this project is built or tested, and scipy (1.15.3) on the build
machine only.  What skimage 0.19 / 0.20 does at its defaults on a float64 image (order 1, mode 'reflect' which it hands to scipy as 'mirror', clip,
anti_aliasing where a side shrinks) is written out below with the two ``scipy.ndimage`` calls it makes, ``gaussian_filter`` and ``zoom(grid_mode=True)``, run by
scipy itself.  Stored per case: the uint8 image and the float64 result.  It asserts what tests/test_skresize_cpu.py asserts."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import skresize_model as M  # noqa: E402

BOUND = 2.0 ** -47


def sk_resize_body(image, output_shape):
    """``skimage.transform.resize(image, output_shape)`` for a float64 ``[H, W, C]`` image at the defaults, by its two scipy calls."""
    from scipy import ndimage as ndi
    image = np.asarray(image, dtype=np.float64)
    output_shape = tuple(output_shape) + (image.shape[2],)
    factors = np.divide(image.shape, output_shape)
    filtered = image
    if any(o < i for o, i in zip(output_shape, image.shape)):
        filtered = ndi.gaussian_filter(image, np.maximum(0, (factors - 1) / 2), cval=0, mode="mirror")
    out = ndi.zoom(filtered, [1 / f for f in factors], order=1, mode="mirror", cval=0, grid_mode=True)
    assert out.shape == output_shape, (out.shape, output_shape)
    return np.clip(out, image.min(), image.max())


def differing(case, seed):
    """(float32 values of the model that differ from scipy's, the largest float64 difference) on ``case`` at ``seed``."""
    img = M.image_u8(case, seed)
    want, got = sk_resize_body(img / 255.0, case[2:]), M.resize(img, case[2:])
    return int((want.astype(np.float32) != got.astype(np.float32)).sum()), float(np.abs(want - got).max())


def main(path):
    out = {}
    for case in M.GOLDEN_CASES:
        img = M.image_u8(case)
        want = sk_resize_body(img / 255.0, case[2:])
        got = M.resize(img, case[2:])
        err = np.abs(want - got).max()
        assert err <= BOUND and np.array_equal(want.astype(np.float32), got.astype(np.float32)), (case, err)
        assert np.abs(M.resize_composed(img, case[2:]) - want).max() <= BOUND, case
        out[M.tag(case) + ".img"], out[M.tag(case) + ".out"] = img, want
        print(M.tag(case), "model - scipy", err)
    for name, case in M.SPECIAL_CASES.items():
        img = M.special_u8(name)
        want = sk_resize_body(img / 255.0, case[2:])
        assert np.abs(M.resize(img, case[2:]) - want).max() <= BOUND
        out[name + ".img"], out[name + ".out"] = img, want
    flat, chan = out["flat200.out"], out["chan100.out"][..., 0]
    assert (flat == 200 / 255.0).all() and (M.resize(M.special_u8("flat200"), (3, 3), "no_clip") != 200 / 255.0).any()
    assert (chan != 100 / 255.0).any() and (M.resize(M.special_u8("chan100"), (3, 3), "clip_per_channel")[..., 0] == 100 / 255.0).all()
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if "--seeds" in sys.argv:
        for seed in range(1, 9):
            print(seed, [differing(c, seed) for c in M.GOLDEN_CASES + (M.WORKLOAD_CASE,)])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g34_skresize.npz"))
