"""Generate g31_codeformer.npz: the reference's own ``CodeFormer`` (swap_face_fine/archs/codeformer_arch.py) in eval mode on the CPU against the float64 model
of tests/codeformer_model.py, with the seeded weights (``seeded.seeded_codeformer_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_codeformer.py [out.npz]

Only the build container has the reference tree.  The reference's module imports ``basicsr.utils.get_root_logger`` and registers its classes with
``basicsr.utils.registry.ARCH_REGISTRY``; basicsr is not installed, so this script puts ``types.ModuleType`` stubs of those two names into ``sys.modules`` before the
import (reference_shim.py is untouched and not needed).  No weights and no images are stored: the tests make them from the seed.

Per case of ``codeformer_model.CASES`` (CF-S small with two samples and H != W, CF-T one token row, CF-F the caller's configuration at 512 x 512 with
``w=0.8, adain=True``):

    <tag>.m.<name>        the float64 model's output rounded to float32: lq_feat, logits, quant_feat, tap32 .. tap256.  An array over 16384 elements is stored as
                          4096 samples of its flat index at the odd stride <tag>.stride.<name>, with its per-(sample, channel) means in <tag>.cmean.<name>; CF-F's
                          logits as every fourth token (<tag>.tstride)
    <tag>.e32.<name>      the max-abs distance of the REFERENCE's float32 output from the float64 model, over the whole array
    <tag>.ref_idx         the reference's top-1 codes
    <tag>.top1 / .top2    per token the float64 model's two largest logits

The reference's tensors: ``logits`` and ``lq_feat`` as ``forward`` returns them, the taps by forward hooks on encoder blocks 14, 11, 8, 5; ``quant_feat`` by a
pre-hook on ``generator.blocks[0]`` for CF-F, and for the small cases (``forward`` hard-codes a 16 x 16 latent) by the reference's own
``quantize.get_codebook_feat`` and ``adaptive_instance_normalization`` called on its own top-1 codes.  ``keys.codeformer``: the reference's ``state_dict`` key
names and shapes at the caller's configuration, one ``name|d0xd1x...`` line per key.

Asserted here on the reference alone, and again by tests/test_codeformer_cpu.py from the file: per case the *close* tokens (float64 top-1 - top-2 margin under
64 e32.logits) are at most 2 % of the tokens, and CF-F's codes take at least 32 distinct values.  A seed that fails either is answered in ``seeded``'s gains."""
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

import codeformer_model as M  # noqa: E402

REF = os.environ.get("E4S_REFERENCE", "/root/reference")


def stub_basicsr():
    class _Registry:
        def register(self, obj=None):
            return (lambda o: o) if obj is None else obj
    import logging
    basicsr, utils, registry = (types.ModuleType(n) for n in ("basicsr", "basicsr.utils", "basicsr.utils.registry"))
    utils.get_root_logger = lambda *a, **k: logging.getLogger("basicsr")
    registry.ARCH_REGISTRY = _Registry()
    basicsr.utils, utils.registry = utils, registry
    sys.modules.update({"basicsr": basicsr, "basicsr.utils": utils, "basicsr.utils.registry": registry})


def reference_outputs(ref, tag, sd, x):
    E, n_head, n_layers, K, T = M.CASES[tag]["cfg"]
    net = ref.CodeFormer(dim_embd=E, n_head=n_head, n_layers=n_layers, codebook_size=K, latent_size=T, connect_list=list(M.CONNECT)).eval()
    net.load_state_dict(sd, strict=True)
    got, hooks = {}, []
    for b, s in M.TAP_BLOCKS.items():
        hooks.append(net.encoder.blocks[b].register_forward_hook(lambda m, i, o, s=s: got.__setitem__("tap" + s, o.clone())))
    xt = torch.from_numpy(x)
    if tag == "CF-F":
        hooks.append(net.generator.blocks[0].register_forward_pre_hook(lambda m, i: got.__setitem__("quant_feat", i[0].clone())))
        _, got["logits"], got["lq_feat"] = net(xt, w=0.8, adain=True)
        got["idx"] = torch.topk(torch.softmax(got["logits"], dim=2), 1, dim=2)[1][..., 0]
    else:
        got["logits"], got["lq_feat"] = net(xt, code_only=True)
        top_idx = torch.topk(torch.softmax(got["logits"], dim=2), 1, dim=2)[1]
        n, c, h, w = got["lq_feat"].shape
        quant = net.quantize.get_codebook_feat(top_idx, shape=[n, h, w, c])
        got["quant_feat"] = ref.adaptive_instance_normalization(quant, got["lq_feat"])
        got["idx"] = top_idx[..., 0]
    for h in hooks:
        h.remove()
    return {k: v.numpy() for k, v in got.items()}


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    stub_basicsr()
    sys.path.insert(0, REF)
    ref = importlib.import_module("swap_face_fine.archs.codeformer_arch")
    assert ref.__file__.startswith(REF)
    out = {}
    with torch.device("meta"):
        full = ref.CodeFormer(dim_embd=512, codebook_size=1024, n_head=8, n_layers=9, connect_list=["32", "64", "128", "256"])
    out["keys.codeformer"] = np.array("\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in full.state_dict().items()))
    print(f"  keys.codeformer: {len(full.state_dict())} keys")
    for tag in M.CASES:
        sd, x = M.case_weights(tag), M.case_input(tag)
        got = reference_outputs(ref, tag, sd, x)
        ref_idx = got["idx"]
        m64 = M.front(sd, x, M.CASES[tag]["cfg"], idx=ref_idx)                  # quant_feat on the reference's codes; idx is compared from top1 / top2
        own = (m64["logits"] == m64["top1"].unsqueeze(-1)).to(torch.int64).argmax(2).numpy()
        for name in M.NAMES:
            want = m64[name].numpy()
            assert got[name].dtype == np.float32 and got[name].shape == want.shape, (tag, name, got[name].shape, want.shape)
            e32 = float(np.abs(got[name].astype(np.float64) - want).max())
            out[f"{tag}.e32.{name}"] = np.float64(e32)
            out[f"{tag}.m.{name}"] = M.stored(tag, name, want.astype(np.float32))
            if name != "logits":
                stride = M.sample_stride(want.size)
                out[f"{tag}.stride.{name}"] = np.int64(stride)
                if stride > 1:
                    out[f"{tag}.cmean.{name}"] = want.reshape(want.shape[0], want.shape[1], -1).mean(2).astype(np.float32)
            print(f"  {tag}.{name}: e32 {e32:.2e}, max {np.abs(want).max():.2f}, std {want.std():.3f}")
        out[f"{tag}.tstride"] = np.int64(M.token_stride(tag))
        out[f"{tag}.ref_idx"] = ref_idx.astype(np.int64)
        out[f"{tag}.top1"], out[f"{tag}.top2"] = m64["top1"].numpy(), m64["top2"].numpy()
        close = M.close_tokens(out[f"{tag}.top1"], out[f"{tag}.top2"], out[f"{tag}.e32.logits"])
        print(f"  {tag}: {int(close.sum())} close of {close.size} tokens, {len(np.unique(ref_idx))} distinct codes, smallest margin "
              f"{(out[f'{tag}.top1'] - out[f'{tag}.top2']).min():.3e}")
        assert close.sum() <= M.CLOSE_SHARE * close.size, (tag, int(close.sum()))
        assert (ref_idx == own)[~close].all(), tag
        if tag == "CF-F":
            assert len(np.unique(ref_idx)) >= 32
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays")
    assert size < 1_000_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g31_codeformer.npz"))
