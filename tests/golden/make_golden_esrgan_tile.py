"""Generate g33_esrgan_tile.npz: what the reference's own ``RealESRGANer`` gives for the tiled Real-ESRGAN step of ``CodeFormerInfer.infer_image``.

    python tests/golden/make_golden_esrgan_tile.py [out.npz]
    python tests/golden/make_golden_esrgan_tile.py --seeds      (the conditioning of the model's cases per seed: how CASE_SEED was chosen)

Only the build container has the reference tree.  No reference source is copied:
  * ``swap_face_fine/realesrgan_utils.py`` is loaded from where it lies (as make_golden_gpen_sr.py loads its files) with ``cv2`` an object whose ``cvtColor`` is
    the channel flip and whose ``resize`` is tests/esrgan_tile_model.py's fixed-point Lanczos4 (cv2 is installed nowhere);
  * a ``RealESRGANer`` is made with ``object.__new__`` — ``half=False``, the CPU — and given the reference's own ``RRDBNet`` of gpen/sr_model/rrdbnet_arch.py at
    ``scale=4, num_feat=64, num_block=1`` with the seeded, calibrated weights of the model's cases;
  * per case ``pre_process -> tile_process`` (or ``process``) ``-> post_process`` runs on the RGB image, and ``enhance`` at ``outscale`` 2, None and 1.5 on its BGR
    flip, the result flipped back: the reference's two flips cancel, so the stored images are RGB in and out.
Stored per case: the image, the float32 x4 output of ``post_process`` and the three uint8 results.  It asserts what tests/test_esrgan_tile_cpu.py asserts."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))                                    # the package (the models take their seeded weights from it)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import esrgan_tile_model as M  # noqa: E402
import make_golden_gpen_paste as MP  # noqa: E402
import make_golden_gpen_sr as MS  # noqa: E402

OUT_KEYS = {2: "out2", None: "out_none", 1.5: "out1p5"}


class _Cv2(types.ModuleType):
    """What realesrgan_utils.py asks of cv2 on an RGB uint8 image: the channel flip and the model's Lanczos4 resize."""

    COLOR_BGR2RGB, COLOR_GRAY2RGB, COLOR_BGR2GRAY, COLOR_BGR2BGRA, INTER_LINEAR, INTER_LANCZOS4, IMREAD_UNCHANGED = "bgr2rgb", "gray2rgb", "bgr2gray", "bgr2bgra", 1, 4, -1

    def __init__(self):
        super().__init__("cv2")
        self.resized = []

    def cvtColor(self, img, code):
        assert code == self.COLOR_BGR2RGB
        return np.ascontiguousarray(img[:, :, ::-1])

    def resize(self, img, dsize, interpolation=None):
        assert interpolation == self.INTER_LANCZOS4 and img.dtype == np.uint8
        self.resized.append(tuple(dsize))
        return M.resize_lanczos4(img, dsize)


def reference_modules():
    """(the reference's rrdbnet_arch module, its realesrgan_utils module, the cv2 stand-in)."""
    arch = MS.reference_modules()[3]
    cv2 = sys.modules["cv2"] = _Cv2()
    utils = MP._load("swap_face_fine.realesrgan_utils", os.path.join(MP.REF, "swap_face_fine", "realesrgan_utils.py"))
    return arch, utils, cv2


def reference_upsampler(arch, utils, sd, tile, tile_pad, pre_pad):
    net = arch.RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=M.NUM_FEAT, num_block=M.SM.num_blocks(sd), num_grow_ch=32, scale=M.SCALE)
    net.load_state_dict(sd, strict=True)
    net.eval()
    obj = object.__new__(utils.RealESRGANer)
    obj.scale, obj.tile_size, obj.tile_pad, obj.pre_pad, obj.mod_scale, obj.half, obj.device, obj.model = M.SCALE, tile, tile_pad, pre_pad, None, False, torch.device("cpu"), net
    return obj


def check_case(tag, c, r32, outs):
    """What tests/test_esrgan_tile_cpu.py asserts of a stored case against the model ``c``."""
    H, W = c["img"].shape[:2]
    err, b = M.max_err(r32, c["r"]), M.bound(c["e32"], c["r"])
    strict, clamped, std = M.check_u8(outs[None], c["u"], c["e32"])
    mstrict, mclamped, mstd = M.conditioned(c)
    print(f"{tag}: x4 {r32.shape}, err {err:.3e} = {err / c['e32']:.2f} e32 (bound {b:.3e}); uint8: strict {100 * strict:.2f} %, clamped {100 * clamped:.2f} %, "
          f"std {std:.1f}; the model alone: strict {100 * mstrict:.2f} %")
    assert err <= b and strict >= 0.99 and clamped < 0.10 and std > 30 and mstrict >= 0.99, tag
    for outscale, out in outs.items():
        dsize = M.out_size(H, W, outscale)
        want = outs[None] if dsize is None else M.resize_lanczos4(outs[None], dsize)
        assert out.shape == want.shape and np.array_equal(out, want), (tag, outscale)


def seeds(limit=8):
    for seed in range(1, limit + 1):
        row = []
        for tag in M.GOLDEN_CASES:
            try:
                strict, clamped, std = M.conditioned(M.golden_case(tag, seed))
                row.append(f"{tag}: strict {100 * strict:.2f} % clamped {100 * clamped:.1f} % std {std:.0f}{'' if strict >= 0.99 and clamped < 0.10 and std > 30 else ' (no)'}")
            except AssertionError as e:
                row.append(f"{tag}: {e} (no)")
        print(f"seed {seed}: " + "; ".join(row))


def main(path):
    arch, utils, cv2 = reference_modules()
    store = {}
    for tag, (H, W, tile, tile_pad, pre_pad) in M.GOLDEN_CASES.items():
        c = M.golden_case(tag)
        up = reference_upsampler(arch, utils, c["sd"], tile, tile_pad, pre_pad)
        with torch.no_grad():
            up.pre_process(c["img"].astype(np.float32) / 255)
            up.tile_process() if tile > 0 else up.process()
            r32 = up.post_process().numpy().copy()
        assert r32.shape == (1, 3, M.SCALE * H, M.SCALE * W) and r32.dtype == np.float32
        outs = {}
        for outscale in M.GOLDEN_OUTSCALES:
            cv2.resized.clear()
            out, mode = up.enhance(np.ascontiguousarray(c["img"][:, :, ::-1]), outscale=outscale)
            assert mode == "RGB" and out.dtype == np.uint8 and cv2.resized == ([] if outscale is None else [M.out_size(H, W, outscale)])
            outs[outscale] = np.ascontiguousarray(out[:, :, ::-1])
        check_case(tag, c, r32, outs)
        store[f"{tag}.img"], store[f"{tag}.r"] = c["img"], r32[0]
        for outscale, out in outs.items():
            store[f"{tag}.{OUT_KEYS[outscale]}"] = out
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(1)
    if "--seeds" in sys.argv:
        seeds()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g33_esrgan_tile.npz"))
