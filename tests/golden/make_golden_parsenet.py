"""Generate g24_parsenet.npz: outputs of the reference's own ``ParseNet`` (swap_face_fine/gpen/face_parse/parse_model.py) in eval mode on the CPU, with the
seeded weights (``seeded.seeded_parsenet_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_parsenet.py [out.npz]

Only the build container has the reference tree.  Per case of ``tests/parsenet_model.py``: the uint8 BGR input ``img`` and the reference's float32 ``out_mask``
and ``out_img`` on ``FaceParse.img2tensor`` of it (the reference's own expression, run here on the CPU).  No weights are stored: the tests make them from the
seed.  The outputs are stored for the first ``PM.STORED[tag]`` samples of a case: all of them, except that case B, whose 64 x 64 x 19 logits are 311 KB a sample,
keeps its first sample's (the whole batch is still run and checked against the float64 model here and in the tests); that holds the file to about 0.7 MB.
``keys.default``: the reference's ``state_dict`` key names and shapes at the configuration ``FaceParse`` builds, one ``name|d0xd1x...`` line per key (a
scalar has no dimensions).  The script asserts what tests/test_parsenet_cpu.py asserts."""
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
import parsenet_model as PM  # noqa: E402


def key_lines(net):
    return "\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items())


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    shim.install()
    ref = importlib.import_module("swap_face_fine.gpen.face_parse.parse_model")
    out = {}
    with torch.device("meta"):
        out["keys.default"] = np.array(key_lines(ref.ParseNet(512, 512, 32, 64, 19, norm_type="bn", relu_type="LeakyReLU", ch_range=[32, 256])))
    assert len(str(out["keys.default"]).split("\n")) == 238
    for tag, ((in_size, out_size, min_feat, base_ch, res_depth, ch_range), (bs, H, W)) in PM.CASES.items():
        c = PM.case(tag)
        net = ref.ParseNet(in_size, out_size, min_feat, base_ch, PM.PARSING_CH, res_depth, norm_type="bn", relu_type="LeakyReLU", ch_range=list(ch_range)).eval()
        net.load_state_dict(c["sd"], strict=True)
        x = np.concatenate([(im[..., ::-1] / 255. * 2 - 1).transpose(2, 0, 1)[None] for im in c["img"]])      # FaceParse.img2tensor per image
        x = torch.from_numpy(x).float()
        assert np.array_equal(x.numpy(), c["x"])
        mask, img = (t.numpy() for t in net(x))
        assert mask.dtype == np.float32 and mask.shape == c["mask64"].shape and img.shape == c["img64"].shape
        e_mask, e_img = PM.max_err(mask, c["mask64"]), PM.max_err(img, c["img64"])
        assert e_mask <= PM.bound(c["e32_mask"], c["mask64"]), (tag, e_mask, c["e32_mask"])
        assert e_img <= PM.bound(c["e32_img"], c["img64"]), (tag, e_img, c["e32_img"])
        assert 1.0 <= mask.std() <= 10.0, (tag, mask.std())
        share = PM.check_labels(mask.argmax(1), c)
        out[f"{tag}.img"] = c["img"]
        out[f"{tag}.out_mask"] = mask[:PM.STORED[tag]]
        out[f"{tag}.out_img"] = img[:PM.STORED[tag]]
        hist = np.bincount(c["labels"].reshape(-1), minlength=PM.PARSING_CH)
        print(f"  {tag}: out {mask.shape[2]} x {mask.shape[3]}, logits std {mask.std():.2f}, image std {img.std():.2f}, ref_err {e_mask:.2e} / {e_img:.2e}, e32 "
              f"{c['e32_mask']:.2e} / {c['e32_img']:.2e}, non-strict {share:.5f}, classes 14 / 18 on {hist[14]} / {hist[18]} pixels")
    for m, tag in PM.MUTANTS.items():
        c = PM.case(tag)
        x = PM.img2tensor(c["img"], bgr=False) if m == "flip_dropped" else c["x"]
        far = PM.max_err(PM.network(c["sd"], x, mutant=None if m == "flip_dropped" else m)[0].numpy()[:PM.STORED[tag]], out[f"{tag}.out_mask"])
        bars = far / PM.bound(c["e32_mask"], c["mask64"])
        print(f"  mutant {m} on {tag}: {far:.3e} = {bars:.0f} bars from the fixture")
        assert bars >= PM.MUTANT_MARGIN, (m, bars)
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays")
    assert size < 750_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g24_parsenet.npz"))
