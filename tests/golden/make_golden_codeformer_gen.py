"""Generate g32_codeformer_gen.npz: the generator half of the reference's own ``CodeFormer`` (swap_face_fine/archs/codeformer_arch.py:264-276) in eval mode on the
CPU against the float64 model of tests/codeformer_gen_model.py, with the seeded weights (``seeded.seeded_codeformer_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_codeformer_gen.py [out.npz]

Only the build container has the reference tree; basicsr is stubbed as make_golden_codeformer.py does it.  No weights and no images are stored: the tests make
them from the seed.

Per case of ``codeformer_model.CASES`` at ``w = 0.8, adain=True``:

    <tag>.m.<name>        the float64 model's output rounded to float32: out, dec32 .. dec256 (the decoder feature behind each fuse block), stored as
                          ``codeformer_model.stored`` does (in full up to 16384 elements, else 4096 samples at the odd stride <tag>.stride.<name>)
    <tag>.e32.<name>      the max-abs distance of the REFERENCE's float32 tensor from the float64 model, over the whole array
    <tag>.m.out_w0, <tag>.e32.out_w0      the same at ``w = 0`` (no fuse block runs), for the small cases
    <tag>.ref_idx         the reference's top-1 codes, on which both sides look their ``quant_feat`` up (g31_codeformer.npz has the same)
    <tag>.before_std, <tag>.after_std     per fuse block the reference's deviation of the decoder stream in front of and behind it
    <tag>.growth, <tag>.term_ratio, <tag>.inside   after / before; std(after - before) / before; the share of the reference's ``out`` inside [-1, 1]

The reference's tensors: CF-F by its own ``net(x, w=0.8, adain=True)`` with forward hooks on ``fuse_convs_dict[s]``; the small cases (``forward`` hard-codes a
16 x 16 latent and names the fuse blocks by the feature's width) by driving its own ``generator.blocks[i]`` and ``fuse_convs_dict[s]`` by block index on its own
``quant_feat`` and taps.

Asserted here on the reference alone, and again by tests/test_codeformer_gen_cpu.py from the file: the stream grows by at most 2 per fuse block, the fused term
is at least 0.1 of the stream, between 0.2 and 0.95 of ``out`` lies inside [-1, 1], every e32 > 0.  Seeded weights that fail one are answered in ``seeded``'s
gains."""
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

import codeformer_gen_model as G  # noqa: E402
import codeformer_model as M  # noqa: E402
from make_golden_codeformer import REF, stub_basicsr  # noqa: E402


def reference_outputs(ref, tag, sd, x):
    """dict(idx, out, dec<s>, before<s>[, out_w0]) of the reference's float32 tensors."""
    E, n_head, n_layers, K, T = M.CASES[tag]["cfg"]
    net = ref.CodeFormer(dim_embd=E, n_head=n_head, n_layers=n_layers, codebook_size=K, latent_size=T, connect_list=list(M.CONNECT)).eval()
    net.load_state_dict(sd, strict=True)
    got, hooks = {}, []
    xt = torch.from_numpy(x)
    if tag == "CF-F":
        for s in M.CONNECT:
            hooks.append(net.fuse_convs_dict[s].register_forward_hook(
                lambda m, i, o, s=s: got.update({"before" + s: i[1].clone(), "dec" + s: o.clone()})))
        got["out"], logits, _ = net(xt, w=G.W, adain=True)
        got["idx"] = torch.topk(torch.softmax(logits, dim=2), 1, dim=2)[1][..., 0]
    else:
        taps = {}
        for b, s in M.TAP_BLOCKS.items():
            hooks.append(net.encoder.blocks[b].register_forward_hook(lambda m, i, o, s=s: taps.__setitem__(s, o.clone())))
        logits, lq = net(xt, code_only=True)
        top_idx = torch.topk(torch.softmax(logits, dim=2), 1, dim=2)[1]
        n, c, h, w = lq.shape
        quant = ref.adaptive_instance_normalization(net.quantize.get_codebook_feat(top_idx, shape=[n, h, w, c]), lq)
        got["idx"] = top_idx[..., 0]
        for fused in (True, False):
            t = quant
            for i, block in enumerate(net.generator.blocks):
                t = block(t)
                if fused and i in G.FUSE_BLOCKS:
                    s = G.FUSE_BLOCKS[i]
                    got["before" + s] = t
                    t = got["dec" + s] = net.fuse_convs_dict[s](taps[s], t, G.W)
            got["out" if fused else "out_w0"] = t
    for h in hooks:
        h.remove()
    return {k: v.numpy() for k, v in got.items()}


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    stub_basicsr()
    sys.path.insert(0, REF)
    ref = importlib.import_module("swap_face_fine.archs.codeformer_arch")
    assert ref.__file__.startswith(REF)
    g31 = np.load(os.path.join(HERE, "g31_codeformer.npz"))
    out = {}
    for tag in M.CASES:
        sd, x = M.case_weights(tag), M.case_input(tag)
        got = reference_outputs(ref, tag, sd, x)
        assert np.array_equal(got["idx"], g31[f"{tag}.ref_idx"]), tag                # the stage-1 weights are what they were
        front = M.front(sd, x, M.CASES[tag]["cfg"], idx=got["idx"])
        m64 = G.generate(sd, front)
        names = G.NAMES + (("out_w0",) if "out_w0" in got else ())
        if "out_w0" in got:
            m64["out_w0"] = G.generate(sd, front, w=0)["out"]
        for name in names:
            want = m64[name].numpy()
            assert got[name].dtype == np.float32 and got[name].shape == want.shape, (tag, name, got[name].shape, want.shape)
            e32 = float(np.abs(got[name].astype(np.float64) - want).max())
            assert e32 > 0, (tag, name)
            out[f"{tag}.e32.{name}"] = np.float64(e32)
            out[f"{tag}.m.{name}"] = M.stored(tag, name, want.astype(np.float32))
            out[f"{tag}.stride.{name}"] = np.int64(M.sample_stride(want.size))
            print(f"  {tag}.{name}: e32 {e32:.2e}, max {np.abs(want).max():.2f}, std {want.std():.3f}, shape {want.shape}")
        growth, ratio, inside = G.fuse_statistics(got)
        out[f"{tag}.ref_idx"] = got["idx"].astype(np.int64)
        out[f"{tag}.before_std"] = np.array([got["before" + s].astype(np.float64).std() for s in M.CONNECT])
        out[f"{tag}.after_std"] = np.array([got["dec" + s].astype(np.float64).std() for s in M.CONNECT])
        out[f"{tag}.growth"], out[f"{tag}.term_ratio"], out[f"{tag}.inside"] = growth, ratio, np.float64(inside)
        print(f"  {tag}: growth {np.round(growth, 3)}, term / dec {np.round(ratio, 3)}, inside [-1, 1] {inside:.3f}, out std {got['out'].std():.3f}")
        assert growth.max() <= 2 and ratio.min() >= 0.1 and 0.2 <= inside <= 0.95, tag
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays")
    assert size < 1_000_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g32_codeformer_gen.npz"))
