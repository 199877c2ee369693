"""Row f8 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

``ops.color_reference`` and ``ops.blender_packages`` against this project's own PyTorch composition of the same formulas on the same device (per part:
``nonzero`` to list the pixels, gather, centre, normalise, one ``[N_A, N_T]`` score matrix, two softmaxes, two products — its host synchronisations are
part of what it costs), at batch 1 and 8, 64 x 64 features from 256 x 256 maps, on two label layouts: a portrait-like one (a skin part of about 2000
feature pixels) and blocky random maps.

    python tools/time_color_refer.py [--rounds 5] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F

import colorref_model as RM
from e4s2024_amd import ops

dev = "cuda:0"
H = W = 256
h = w = 64


def portrait_labels(bs, seed=0):
    """uint8 [bs, 256, 256] 19-class maps laid out like a portrait: a skin ellipse of about 2000 feature pixels with eyes, brows, nose, lips, teeth and ears
    on it and hair above, shifted a little from sample to sample."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((bs, H, W), np.uint8)
    for b in range(bs):
        cy, cx = 136 + rs.randint(-6, 7), 128 + rs.randint(-6, 7)
        ell = lambda y, x, ry, rx: ((yy - y) / ry) ** 2 + ((xx - x) / rx) ** 2 <= 1   # noqa: E731
        lab = out[b]
        lab[ell(cy - 20, cx, 130, 112)] = 17
        lab[ell(cy, cx, 122, 104)] = 1
        for s in (-1, 1):
            lab[ell(cy - 4, cx + s * 96, 22, 10)] = 7 if s < 0 else 8
            lab[ell(cy - 26, cx + s * 36, 9, 20)] = 4 if s < 0 else 5
            lab[ell(cy - 46, cx + s * 36, 6, 26)] = 2 if s < 0 else 3
        lab[ell(cy + 8, cx, 26, 14)] = 10
        lab[ell(cy + 48, cx, 8, 30)] = 12
        lab[ell(cy + 56, cx, 4, 22)] = 11
        lab[ell(cy + 64, cx, 8, 28)] = 13
    return out


def torch_color_reference(img_t, feats_a, feats_t, parts_a, parts_t, tau):
    """The formulas of ``ops.color_reference`` with stock PyTorch ops on the device, sample by sample and part by part."""
    bs = img_t.shape[0]
    iy = torch.from_numpy(RM.nearest_index(h, H)).to(img_t.device)
    ix = torch.from_numpy(RM.nearest_index(w, W)).to(img_t.device)
    pick = lambda x: x[..., iy[:, None], ix[None, :]]   # noqa: E731
    mean, std = img_t.new_tensor(RM.MEAN).view(1, 3, 1, 1), img_t.new_tensor(RM.STD).view(1, 3, 1, 1)
    rgb = (pick(img_t) * std + mean).clamp(0, 1).flatten(2)
    ma, mt = pick(parts_a).flatten(2) != 0, pick(parts_t).flatten(2) != 0
    refs = torch.zeros(bs, 9, 3, h * w, device=img_t.device)
    inv = torch.zeros(bs, 3, h * w, device=img_t.device)
    for b in range(bs):
        fa, ft = feats_a[b].flatten(1).t(), feats_t[b].flatten(1).t()
        for p in range(9):
            ia, it = torch.nonzero(ma[b, p])[:, 0], torch.nonzero(mt[b, p])[:, 0]                  # host synchronisations
            if len(ia) == 0 or len(it) == 0:
                continue
            x = fa[ia]
            y = ft[it] * ma[b, p][it][:, None]
            x, y = x - x.mean(1, keepdim=True), y - y.mean(1, keepdim=True)
            c = (x / x.norm(dim=1, keepdim=True).clamp_min(1e-8)) @ (y / y.norm(dim=1, keepdim=True).clamp_min(1e-8)).t()
            ref = torch.softmax(c * tau, dim=1) @ rgb[b][:, it].t()
            refs[b, p][:, ia] = ref.t()
            inv[b][:, it] += (torch.softmax(c.t() * tau, dim=1) @ ref).t()
    present = (ma.any(2) & mt.any(2))
    return refs.view(bs, 9, 3, h, w), present, inv.view(bs, 3, h, w), (rgb * pick(parts_t).flatten(2).sum(1, keepdim=True)).view(bs, 3, h, w)


def torch_blender_packages(img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau):
    """``Referencer.forward`` after its FPN calls with stock PyTorch ops (``max_pool2d`` dilation, ``interpolate``) around ``torch_color_reference``."""
    k = int(W * 0.1 / 2) * 2 + 1
    dil = lambda m: F.max_pool2d(m, kernel_size=k, stride=1, padding=k // 2)   # noqa: E731

    def parts(lab):
        return torch.stack([sum((lab == i) for i in RM.NAME_TO_IDS[n]).float() for n in RM.PARTS[:-1]], dim=1)

    pa, pt = parts(labels_a), parts(labels_t)
    head_a, head_t = pa.sum(1, keepdim=True), pt.sum(1, keepdim=True)
    inp_t = (dil(head_t) - head_t).clamp(0, 1)
    e_at = dil((head_a + head_t).clamp(0, 1))
    inp_a = (e_at - head_a).clamp(0, 1)
    refs, present, inv, inv_target = torch_color_reference(img_t, feats_a, feats_t, torch.cat([pa, inp_a], 1), torch.cat([pt, inp_t], 1), tau)
    gate = (present.sum(1) >= 2).float().view(-1, 1, 1, 1)
    six = F.interpolate(torch.cat([refs[:, :-1].sum(1), refs[:, -1]], dim=1) * gate, size=(H, W), mode="bilinear", align_corners=True)
    mean, std = img_a.new_tensor(RM.MEAN).view(1, 3, 1, 1), img_a.new_tensor(RM.STD).view(1, 3, 1, 1)
    a01 = (img_a * std + mean).clamp(0, 1)
    grey = (a01[:, 0] * 0.299 + a01[:, 1] * 0.587 + a01[:, 2] * 0.114).clamp(0, 1)[:, None] * head_a
    return torch.cat([six, head_a, inp_a, grey, img_t * (1 - e_at)], dim=1), (inv, inv_target)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, rounds, reps):
    """{name: [ms per call, one per round]}: every function warmed, then round by round one after the other."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, reps))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def report(title, res):
    s = {k: summary(v) for k, v in res.items()}
    for k, v in s.items():
        print(f"  {title} {k:6s}: median {v['median_ms']:9.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}", flush=True)
    faster = max(res["hip"]) < min(res["torch"])
    print(f"  {title}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.1f}x, slowest hip round below fastest torch round: {faster}", flush=True)
    return {**s, "hip_faster_beyond_spread": faster}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"color_reference / blender_packages, 64 x 64 features from 256 x 256 maps, {doc['device']}")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    for layout in ("portrait", "blocky"):
        for bs in (1, 8):
            if layout == "portrait":
                la, lt = portrait_labels(bs, 1), portrait_labels(bs, 2)
            else:
                la, lt = RM.blocky_labels(11, bs, H, W, 32), RM.blocky_labels(12, bs, H, W, 32)
            pa, pt, _, _, _ = RM.part_masks(la, lt)
            sizes = RM.nearest_pick(torch.from_numpy(pa), h, w).flatten(2).sum(2)[0].tolist()
            img_a, img_t, fa, ft = T(RM.image(21, bs, H, W)), T(RM.image(22, bs, H, W)), T(RM.features(23, bs, h, w)), T(RM.features(24, bs, h, w))
            la, lt, pa, pt = T(la), T(lt), T(pa), T(pt)
            tau = 7.0
            tag = f"{layout} bs{bs}"
            print(f" {tag}: part sizes of A, sample 0: {sizes}")
            got, want = ops.color_reference(img_t, fa, ft, pa, pt, tau), torch_color_reference(img_t, fa, ft, pa, pt, tau)
            agree = max(float((g.float() - x.float()).abs().max()) for g, x in zip(got, want))
            res = alternate({"hip": lambda: ops.color_reference(img_t, fa, ft, pa, pt, tau),
                             "torch": lambda: torch_color_reference(img_t, fa, ft, pa, pt, tau)}, a.rounds, 5)
            doc["cases"][f"color_reference {tag}"] = {**report(f"color_reference   {tag}", res), "outputs_agree_to": agree, "part_sizes_a": sizes}
            gp, wp = ops.blender_packages(img_a, img_t, la, lt, fa, ft, tau), torch_blender_packages(img_a, img_t, la, lt, fa, ft, tau)
            agree_p = float((gp[0] - wp[0]).abs().max())
            res = alternate({"hip": lambda: ops.blender_packages(img_a, img_t, la, lt, fa, ft, tau),
                             "torch": lambda: torch_blender_packages(img_a, img_t, la, lt, fa, ft, tau)}, a.rounds, 5)
            doc["cases"][f"blender_packages {tag}"] = {**report(f"blender_packages  {tag}", res), "outputs_agree_to": agree_p}
            print(f"  {tag}: outputs agree to {agree:.1e} (color_reference), {agree_p:.1e} (packages)", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_color_refer", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
