"""Generate g20_color_refer.npz: outputs of the reference's own ``get_color_refer`` (swap_face_fine/Blender/model_center/semantic_tools.py:50-167) and of
``Referencer.forward`` (referencer.py:24-86), all at batch 1 on the CPU.

    python tests/golden/make_golden_color_refer.py [out.npz]

Only the build container has the reference tree.  ``referencer.py`` imports ``torchvision.models`` and does not use it: it is stubbed.  ``forward`` is called
unbound on a stand-in ``self`` whose ``FPN`` returns the seeded features (first call: A's, second call: T's, whichever way the random flip goes), with
``args(small_FPN=False, lambda_CYC2=10.)``, ``trainable_tao`` and ``compute_inv=True``.  The inputs are not stored: ``tests/colorref_model.py`` makes them from
seeds, here and in the tests; the file records a checksum of each.  For every case ``ref_err`` is the reference's float32 output against the float64
model: the tests' bound is four times it.  Outputs of a part with a single pixel are left out of it (``colorref_model.one_pixel_outputs``: the
reference divides 0 by 0 there and writes zero); the maker asserts that it does."""
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
import colorref_model as RM  # noqa: E402

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


def reference_modules():
    shim.install()
    tv = sys.modules["torchvision"]
    if not hasattr(tv, "models"):
        tv.models = types.ModuleType("torchvision.models")
        sys.modules["torchvision.models"] = tv.models
    return (importlib.import_module("swap_face_fine.Blender.model_center.semantic_tools"),
            importlib.import_module("swap_face_fine.Blender.model_center.referencer"))


def dict_to_planes(d, h, w):
    """The reference's dict of [1, 3, h, w] entries -> ([9, 3, h, w] with zeros for missing parts, the keys in its order)."""
    out = np.zeros((len(RM.PARTS), 3, h, w), np.float32)
    for k, v in d.items():
        assert v.dtype == torch.float32 and tuple(v.shape) == (1, 3, h, w), (k, v.dtype, v.shape)
        out[RM.PARTS.index(k)] = v[0].numpy()
    return out, list(d.keys())


def err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def refer_case(st, out, tag, img_t, fa, ft, pa, pt, tau):
    """One ``get_color_refer`` call; returns ref_err."""
    da, dt = RM.part_dicts(pa, pt)
    refs, pair = st.get_color_refer(T(img_t), T(fa), T(ft), da, dt, torch.tensor(float(tau)), True, False)
    h, w = fa.shape[-2:]
    planes, keys = dict_to_planes(refs, h, w)
    m_refs, m_present, m_inv, m_tgt = RM.color_reference(img_t, fa, ft, pa, pt, tau)
    assert keys == [n for i, n in enumerate(RM.PARTS) if m_present[0, i]], (keys, m_present)
    inv_ref = pair[0][0].numpy()
    ru, iu = RM.one_pixel_outputs(pa, pt, h, w)                    # a one-pixel part: the reference divides 0 by 0 and writes zero; not compared
    ru, iu = np.broadcast_to(ru, planes.shape), np.broadcast_to(iu, inv_ref.shape)
    assert not planes[ru].any() and not inv_ref[iu].any() and not np.isnan(planes).any() and not np.isnan(inv_ref).any()
    e = max(err(np.where(ru, 0, planes), np.where(ru, 0, m_refs[0])), err(np.where(iu, 0, inv_ref), np.where(iu, 0, m_inv[0])),
            err(pair[1][0].numpy(), m_tgt[0]))
    if ru.any() or iu.any():
        print(f"  {tag}: {int(ru.sum())} reference and {int(iu.sum())} inverse values lie in one-pixel parts (the reference writes zero there)")
    out[f"{tag}.refs"], out[f"{tag}.inv"], out[f"{tag}.inv_target"] = planes, pair[0][0].numpy(), pair[1][0].numpy()
    out[f"{tag}.keys"] = np.array(",".join(keys))
    out[f"{tag}.ref_err"] = np.float64(e)
    print(f"  {tag}: present {keys}, ref_err {e:.3e}")
    return e


def forward_case(rf, out, tag, img_a, img_t, la, lt, fa, ft, tau):
    """``Referencer.forward`` unbound; returns ref_err over the packages and both inverse pairs."""
    feats = iter([T(fa), T(ft)])
    me = types.SimpleNamespace(FPN=lambda x, y: next(feats), args=types.SimpleNamespace(small_FPN=False, lambda_CYC2=10.),
                               trainable_tao=torch.tensor(float(tau)), compute_inv=True)
    np.random.seed(0)
    packages, pair, pair_cro = rf.Referencer.forward(me, T(img_a), T(img_t), T(la).long(), T(lt).long())
    assert packages.dtype == torch.float32 and tuple(packages.shape) == (1, 12) + img_t.shape[-2:]
    m_pack, (m_inv, m_tgt), m_present = RM.packages(img_a, img_t, la, lt, fa, ft, tau)
    exact = bool(np.array_equal(packages[0, 6:].numpy(), m_pack[0, 6:].astype(np.float32)))
    assert exact, "the mask, grey and background channels of the model differ from the reference's"
    e = max(err(packages[0, :6].numpy(), m_pack[0, :6]), err(pair[0][0].numpy(), m_inv[0]), err(pair[1][0].numpy(), m_tgt[0]),
            err(pair_cro[0][0].numpy(), m_inv[0]), err(pair_cro[1][0].numpy(), m_tgt[0]))
    out[f"{tag}.packages"] = packages[0].numpy()
    out[f"{tag}.inv"], out[f"{tag}.inv_target"] = pair[0][0].numpy(), pair[1][0].numpy()
    out[f"{tag}.inv_cro"], out[f"{tag}.inv_target_cro"] = pair_cro[0][0].numpy(), pair_cro[1][0].numpy()
    keys = [n for i, n in enumerate(RM.PARTS) if m_present[0, i]]
    out[f"{tag}.keys"] = np.array(",".join(keys))
    out[f"{tag}.ref_err"] = np.float64(e)
    print(f"  {tag}: present {keys}, reference channels max {np.abs(packages[0, :6].numpy()).max():.3f}, ref_err {e:.3e}")
    return e


def main(out_path):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    st, rf = reference_modules()
    out, worst = {}, 0.0
    # (i) hand-built parts at four temperatures
    img_t, fa, ft, pa, pt = RM.case_hand()
    out["hand.crc"] = RM.crc(img_t, fa, ft, pa, pt)
    for tau in RM.HAND_TAUS:
        worst = max(worst, refer_case(st, out, f"hand.tau{tau:g}", img_t, fa, ft, pa, pt, tau))
    assert str(out["hand.tau1.keys"]).split(",") == list(RM.HAND_PRESENT)
    # (ii) Referencer.forward on blocky maps
    c = RM.case_forward()
    out["forward.crc"] = RM.crc(*c[:6])
    worst = max(worst, forward_case(rf, out, "forward", *c))
    # (iii) 64 x 64 features, parts of some hundred pixels
    img_t, fa, ft, pa, pt, tau = RM.case_large()
    out["large.crc"] = RM.crc(img_t, fa, ft, pa, pt)
    sizes = RM.nearest_pick(pa[0], 64, 64).reshape(9, -1).sum(1), RM.nearest_pick(pt[0], 64, 64).reshape(9, -1).sum(1)
    print(f"  large: part sizes A {sizes[0].tolist()}, T {sizes[1].tolist()}")
    worst = max(worst, refer_case(st, out, "large", img_t, fa, ft, pa, pt, tau))
    # (iv) two classes: skin and inpainting only — two parts are enough for a reference
    c = RM.case_two_class()
    out["two_class.crc"] = RM.crc(*c[:6])
    worst = max(worst, forward_case(rf, out, "two_class", *c))
    assert str(out["two_class.keys"]) == "skin,inpainting" and np.abs(out["two_class.packages"][:6]).max() > 0
    np.savez_compressed(out_path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(out_path)
    print(f"wrote {out_path}: {size / 1024:.0f} KiB, {len(out)} arrays; worst ref_err {worst:.3e}")
    assert size < 1_000_000


if __name__ == "__main__":
    with torch.no_grad():
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g20_color_refer.npz"))
