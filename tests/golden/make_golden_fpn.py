"""Generate g22_fpn.npz: outputs of the reference's own ``AdaptiveFeatureGenerator`` and ``SmallFPN`` (swap_face_fine/Blender/model_center/backbone.py) in
eval mode on the CPU, built from the defaults of ``get_base_parser()`` + ``add_hyper`` (utils/parser.py, inference.py:19-32) with the seeded weights
(``seeded.seeded_fpn_state_dict`` / ``seeded_small_fpn_state_dict``) loaded with ``strict=True``.

    python tests/golden/make_golden_fpn.py [out.npz]

Only the build container has the reference tree.  ``cmodules/architecture.py`` imports ``torchvision`` for a VGG it does not build here: it is stubbed.
``add_hyper`` lives in ``inference.py``, whose imports reach far beyond the network; its eight ``add_argument`` lines are read from the file's syntax tree
and applied to the parser, without importing the module.  The inputs are not stored: ``tests/fpn_model.py`` makes them from seeds, here and in the tests; the
file records a checksum of each.  Per case: the reference's float32 output (at 256 x 256 its values at 8192 seeded positions), ``ref_err``, that output
against the float64 model, and ``e32``, the float32 model against the float64 model (at 256 x 256 over the recorded positions, so that no test has to run
the float64 model at that size).  ``20x12.flip.out``: the reference on the mirrored image of that case, what ``Referencer.forward`` takes as the target's
features when it flips.  Per network: the reference's ``state_dict`` key names and shapes, one ``name|d0xd1x...`` line per key.

Every case must be well conditioned: the maker asserts ``e32 <= 1e-3 std(output)``.  InstanceNorm over a 2 x 2 plane can amplify; a seed that gives an
ill-conditioned case is changed, never the bound."""
import ast
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

import fpn_model as FM  # noqa: E402
import reference_shim as shim  # noqa: E402

CONDITION = 1e-3


def reference_args(**changed):
    """The namespace ``BlenderInfer`` builds its network from: ``get_base_parser()`` + ``add_hyper`` at their defaults."""
    parser = importlib.import_module("swap_face_fine.Blender.utils.parser").get_base_parser()
    with open(os.path.join(shim.REF, "swap_face_fine", "Blender", "inference.py")) as f:
        tree = ast.parse(f.read())
    add_hyper = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "add_hyper")
    calls = [s.value for s in add_hyper.body if isinstance(s, ast.Expr) and isinstance(s.value, ast.Call) and s.value.func.attr == "add_argument"]
    assert len(calls) == 8, len(calls)
    for c in calls:
        kw = {k.arg: (k.value.id if isinstance(k.value, ast.Name) else ast.literal_eval(k.value)) for k in c.keywords}
        if kw.get("type") is not None:
            kw["type"] = {"float": float, "int": int, "str": str}[kw["type"]]
        parser.add_argument(*[ast.literal_eval(a) for a in c.args], **kw)
    args = parser.parse_args([])
    args.eval_only = True
    for k, v in changed.items():
        setattr(args, k, v)
    return args


def reference_backbone():
    shim.install()
    return importlib.import_module("swap_face_fine.Blender.model_center.backbone")


def keys_text(net):
    return np.array("\n".join(f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items()))


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = reference_backbone()
    args = reference_args()
    nets = {False: ref.AdaptiveFeatureGenerator(args).eval(), True: ref.SmallFPN().eval()}
    out = {"keys.fpn": keys_text(nets[False]), "keys.small": keys_text(nets[True])}
    for small, net in nets.items():
        net.load_state_dict(FM.state_dict(small), strict=True)
    worst = 0.0
    for tag, (H, W, bs, small) in FM.CASES.items():
        x = FM.case_inputs(tag)
        got = nets[small](torch.from_numpy(x), torch.from_numpy(x))
        h, w = FM.out_size(H, W)
        assert got.dtype == torch.float32 and tuple(got.shape) == (bs, 256, h, w), (got.dtype, got.shape)
        got = got.numpy()
        want, f32 = FM.reference_output(tag), FM.reference_output(tag, torch.float32)
        if tag in FM.SAMPLED:
            pos = FM.sample_positions(tag)
            got_s, want_s, f32_s = got.reshape(-1)[pos], want.reshape(-1)[pos], f32.reshape(-1)[pos]
        else:
            got_s, want_s, f32_s = got, want, f32
        e, e32 = FM.max_err(got_s, want_s), FM.max_err(f32_s, want_s)
        worst = max(worst, e / e32)
        out[f"{tag}.crc"] = FM.crc(x)
        out[f"{tag}.out"] = got_s
        out[f"{tag}.ref_err"] = np.float64(e)
        out[f"{tag}.e32"] = np.float64(e32)
        out[f"{tag}.absmax"] = np.float64(np.abs(want).max())
        print(f"  {tag}: output std {want.std():.3f}, max {np.abs(want).max():.2f}, ref_err {e:.3e}, e32 {e32:.3e} = {e32 / want.std():.1e} std")
        assert e32 <= CONDITION * want.std(), f"{tag} is ill conditioned: change the seed or the size"
        assert e <= FM.bound(e32, want), f"{tag}: the float64 model is not the reference"
    tag = "20x12"
    flipped = np.ascontiguousarray(FM.case_inputs(tag)[..., ::-1])
    out[f"{tag}.flip.out"] = nets[False](torch.from_numpy(flipped), torch.from_numpy(flipped)).numpy()
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays; worst ref_err / e32 {worst:.2f}")
    assert size < 1_000_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g22_fpn.npz"))
