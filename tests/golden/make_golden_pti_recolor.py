"""Generate g17_pti_recolor.npz: the two-target PTI objective of ``VideoSwapPTICoach.train_e4s`` (training/video_swap_ft_coach.py:277-287) —
``calc_loss(driven, recon, fg) + recolor_lambda * calc_loss(recolor, recon, fg)`` with the reference's own ``calc_loss`` (:179-219) on its own
``LPIPS``, ``IDLoss`` and ``FaceParsingLoss`` — and its gradient with respect to the reconstruction, on the CPU in float64 at 1024 x 1024.

    python tests/golden/make_golden_pti_recolor.py [out.npz]

Only the build container has the reference tree.  Weights come from ``seeded`` (LPIPS_SEED, ID_SEED, FP_SEED), the images and the region map from
``inputs()`` below (also used by the GPU test); neither is stored.  The fixture holds the total, the eight per-term values (``terms [2, 4]``: driven
and recolor x l2, lpips, id, face parsing, unweighted) and d loss / d recon at N_SAMPLES positions."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("E4S_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from e4s2024_amd import seeded  # noqa: E402

SEED = 47
LPIPS_SEED, ID_SEED, FP_SEED = 31, 42, 43
LAMBDAS = {"l2_lambda": 1.0, "lpips_lambda": 0.8, "id_lambda": 0.1, "face_parsing_lambda": 0.1}      # PTI's defaults (pti.py)
RECOLOR_LAMBDA = 5.0                                                                                    # our_swap_face_pipeline_options.py:45
BG_CLASSES = (0, 4, 11)                                                                                 # video_swap_ft_coach.py:277
N_SAMPLES = 4096


def inputs():
    """(recon, driven, recolor [1, 3, 1024, 1024], fg [1, 1, 1024, 1024]) float32 on the CPU: the fg as train_e4s computes it (:277-280)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    recon = torch.tanh(T(seeded.seeded_array(SEED, "recolor_recon", (1, 3, 1024, 1024), dist="normal")))
    driven = (0.7 * recon + 0.3 * torch.tanh(T(seeded.seeded_array(SEED, "recolor_driven", (1, 3, 1024, 1024), dist="normal")))).clamp(-1, 1)
    recolor = (0.8 * driven + 0.1 * torch.tanh(T(seeded.seeded_array(SEED, "recolor_recolor", (1, 3, 1024, 1024), dist="normal")))).clamp(-1, 1)
    m = torch.from_numpy(np.asarray(seeded.blocky_labels(3, 1, 12, 512, 16))).long()[:, None]
    bg = torch.zeros_like(m, dtype=torch.bool)
    for c in BG_CLASSES:
        bg = bg | (m == c)
    fg = F.interpolate(torch.logical_not(bg).float(), (1024, 1024), mode="bilinear", align_corners=False)
    return recon, driven, recolor, fg


def sample_index(n: int):
    return np.sort(np.random.RandomState(SEED).choice(n, N_SAMPLES, replace=False)).astype(np.int64)


def reference_coach():
    """A stand-in ``self`` for the reference's ``calc_loss``: its options and its three loss modules, in float64."""
    import make_golden_face_parsing
    import make_golden_id
    import make_golden_lpips
    lp = make_golden_lpips.reference_lpips(seeded.seeded_lpips_state_dict(LPIPS_SEED))
    idl = make_golden_id.reference_idloss(seeded.seeded_irse50_state_dict(ID_SEED), True)
    fpl = make_golden_face_parsing.reference_loss(seeded.seeded_unet_state_dict(FP_SEED))
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return types.SimpleNamespace(opts=types.SimpleNamespace(recolor_lambda=RECOLOR_LAMBDA, **LAMBDAS), lpips_loss=lp, id_loss=idl, face_parsing_loss=fpl)


def calc_loss_source():
    """The reference's ``VideoSwapPTICoach.calc_loss``, taken from its file (the module itself imports the whole training stack)."""
    import ast
    import textwrap
    path = os.path.join(REF, "training", "video_swap_ft_coach.py")
    src = open(path).read()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == "calc_loss":
            code = textwrap.dedent("\n".join(src.splitlines()[node.lineno - 1:node.end_lineno]))
            ns = {"F": F, "torch": torch}
            exec(compile(code, path, "exec"), ns)
            return ns["calc_loss"]
    raise RuntimeError(f"calc_loss not found in {path}")


def main(out):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    coach = reference_coach()
    calc_loss = calc_loss_source()
    recon, driven, recolor, fg = inputs()
    x = recon.double().requires_grad_(True)
    fgd = fg.double()
    loss, d_drv, _ = calc_loss(coach, driven.double(), x, foreground_mask=fgd)          # train_e4s :281-282 (erode: the fg-weighted driven term)
    loss_rec, d_rec, _ = calc_loss(coach, recolor.double(), x, foreground_mask=fgd)     # :286
    total = loss + loss_rec * coach.opts.recolor_lambda                                  # :287
    (g,) = torch.autograd.grad(total, x)
    g = g.numpy()
    names = ("loss_l2", "loss_lpips", "loss_id", "loss_face_parsing")
    terms = np.array([[d[n] for n in names] for d in (d_drv, d_rec)], dtype=np.float64)
    idx = sample_index(g.size)
    d = {"seed": np.int64(SEED), "seeds": np.array([LPIPS_SEED, ID_SEED, FP_SEED], dtype=np.int64), "recolor_lambda": np.float64(RECOLOR_LAMBDA),
         "lambdas": np.array([LAMBDAS[k] for k in ("l2_lambda", "lpips_lambda", "id_lambda", "face_parsing_lambda")]),
         "loss": np.float64(total.item()), "terms": terms, "grad_idx": idx, "grad_samples": g.reshape(-1)[idx], "grad_norm": np.linalg.norm(g)}
    print(f"loss {total.item():.8f} terms {terms.tolist()} |g| {np.linalg.norm(g):.4e}", flush=True)
    np.savez_compressed(out, **{k: np.asarray(v) for k, v in d.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g17_pti_recolor.npz"))
