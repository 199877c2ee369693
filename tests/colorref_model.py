"""The semantic colour reference of the Blender recolouring network (row f8) restated directly, in float64 or float32, and the seeded inputs of its fixture
(``tests/golden/g20_color_refer.npz``) and tests.

Per sample and part ``p`` with pixels ``A_p`` / ``T_p`` at the feature size (masks and the image brought there by the legacy nearest pick
``floor(i * (H / h))``), absent when either set is empty:

    x_a = fA[:, a];   y_t = fT[:, t] if mA_p[t] else 0;   both minus their channel mean
    c[a, t] = x_a . y_t / (max(|x_a|, 1e-8) max(|y_t|, 1e-8))
    ref_p[:, a] = sum_t softmax_t(tau c[a, t]) rgb_T[:, t];      inv_p[:, t] = sum_a softmax_a(tau c[a, t]) ref_p[:, a]

``dtype=torch.float32`` runs the same expressions in float32 — the reference's arithmetic class, from which the tests take their bounds."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

PARTS = ("skin", "hair", "eye", "nose", "lip", "tooth", "ear", "brow", "inpainting")
NAME_TO_IDS = {"skin": (1,), "hair": (17,), "eye": (4, 5), "nose": (10,), "lip": (12, 13), "tooth": (11,), "ear": (7, 8), "brow": (2, 3)}
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
D = 256
FLOOR = 2e-7                               # three float32 ulps at 1.0
MARGIN = 4.0


def bound(err):
    return max(MARGIN * float(err), FLOOR)


def crc(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return np.uint32(c)


def nearest_index(out_size, in_size):
    """torch's legacy 'nearest': min(floor(i * scale), in - 1) with scale = in / out in float32."""
    scale = np.float32(in_size) / np.float32(out_size)
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)


def nearest_pick(x, h, w):
    """[..., H, W] -> [..., h, w]."""
    iy, ix = nearest_index(h, x.shape[-2]), nearest_index(w, x.shape[-1])
    return x[..., iy[:, None], ix[None, :]]


def denorm(img):
    """clamp(img * std + mean, 0, 1) in float32, as the float32 tensor expression forms it."""
    img = torch.as_tensor(img, dtype=torch.float32)
    return (img * torch.tensor(STD).view(-1, 1, 1) + torch.tensor(MEAN).view(-1, 1, 1)).clamp(0, 1)


def dilate(m, k):
    return F.max_pool2d(m[:, None].float(), kernel_size=k, stride=1, padding=k // 2)[:, 0]


def part_masks(labels_a, labels_t):
    """uint8 [bs, H, W] label maps -> (parts_a, parts_t uint8 [bs, 9, H, W], head_a, head_t, e_at float32 [bs, 1, H, W]) as numpy arrays."""
    la, lt = torch.as_tensor(labels_a).long(), torch.as_tensor(labels_t).long()
    k = int(la.shape[-1] * 0.1 / 2) * 2 + 1

    def parts(lab):
        return torch.stack([sum((lab == i) for i in NAME_TO_IDS[n]).float() for n in PARTS[:-1]], dim=1)

    pa, pt = parts(la), parts(lt)
    head_a, head_t = pa.sum(1), pt.sum(1)
    inp_t = (dilate(head_t, k) - head_t).clamp(0, 1)
    e_at = dilate((head_a + head_t).clamp(0, 1), k)
    inp_a = (e_at - head_a).clamp(0, 1)
    full_a, full_t = torch.cat([pa, inp_a[:, None]], 1), torch.cat([pt, inp_t[:, None]], 1)
    return (full_a.to(torch.uint8).numpy(), full_t.to(torch.uint8).numpy(), head_a[:, None].numpy(), head_t[:, None].numpy(), e_at[:, None].numpy())


def _unit_rows(x):
    """[N, D] rows minus their mean, over max(norm, 1e-8)."""
    x = x - x.mean(1, keepdim=True)
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-8)


def color_reference(img_t, feats_a, feats_t, parts_a, parts_t, tau, compute_inv=True, dtype=torch.float64):
    """Inputs as ``ops.color_reference`` (numpy or CPU tensors).  Returns numpy ``(refs [bs, 9, 3, h, w], present uint8 [bs, 9], inv, inv_target)`` in
    ``dtype`` (``inv`` / ``inv_target`` None without ``compute_inv``).  Every sample on its own."""
    img_t, feats_a, feats_t = (torch.as_tensor(v, dtype=torch.float32) for v in (img_t, feats_a, feats_t))
    parts_a, parts_t = torch.as_tensor(parts_a), torch.as_tensor(parts_t)
    bs, _, h, w = feats_a.shape
    hw = h * w
    tau = float(tau)
    refs = torch.zeros(bs, len(PARTS), 3, hw, dtype=dtype)
    inv = torch.zeros(bs, 3, hw, dtype=dtype)
    inv_target = torch.zeros(bs, 3, hw, dtype=dtype)
    present = np.zeros((bs, len(PARTS)), np.uint8)
    for b in range(bs):
        rgb = nearest_pick(denorm(img_t[b]), h, w).reshape(3, hw).to(dtype)
        fa, ft = feats_a[b].reshape(D, hw).t().to(dtype), feats_t[b].reshape(D, hw).t().to(dtype)
        ma, mt = nearest_pick(parts_a[b], h, w).reshape(-1, hw) != 0, nearest_pick(parts_t[b], h, w).reshape(-1, hw) != 0
        inv_target[b] = rgb * nearest_pick(parts_t[b], h, w).reshape(-1, hw).sum(0).to(dtype)
        for p in range(len(PARTS)):
            ia, it = torch.nonzero(ma[p])[:, 0], torch.nonzero(mt[p])[:, 0]
            if len(ia) == 0 or len(it) == 0:
                continue
            present[b, p] = 1
            x = _unit_rows(fa[ia])
            y = _unit_rows(ft[it] * ma[p][it].to(dtype)[:, None])
            c = x @ y.t()
            ref = torch.softmax(c * tau, dim=1) @ rgb[:, it].t()              # [N_A, 3]
            refs[b, p][:, ia] = ref.t()
            if compute_inv:
                inv[b][:, it] += (torch.softmax(c.t() * tau, dim=1) @ ref).t()
    shape = (bs, 3, h, w)
    return (refs.reshape(bs, len(PARTS), 3, h, w).numpy(), present, inv.reshape(shape).numpy() if compute_inv else None,
            inv_target.reshape(shape).numpy() if compute_inv else None)


def one_pixel_outputs(parts_a, parts_t, h, w):
    """Where the reference itself is undefined.  It numbers a part's N pixels with ``linspace(0, N - 1, N) * 2 / (N - 1) - 1`` (semantic_tools.py:29): at
    N = 1 that is 0 / 0, the NaN coordinate samples as padding, and it writes ZERO — for the forward reference of a part with one pixel of A (and so for that
    part's inverse, whose values are the reference), and for the inverse of a part with one pixel of T.  Sample 0 only.  Returns boolean
    ``(refs_undefined [9, 1, h, w], inv_undefined [1, h, w])``; the restated semantics (and the kernel) give the softmax's value there like anywhere else."""
    ma = nearest_pick(torch.as_tensor(parts_a)[0], h, w) != 0
    mt = nearest_pick(torch.as_tensor(parts_t)[0], h, w) != 0
    na, nt = ma.flatten(1).sum(1), mt.flatten(1).sum(1)
    present = (na > 0) & (nt > 0)
    refs_u = ma & (present & (na == 1)).view(-1, 1, 1)
    inv_u = (mt & (present & ((na == 1) | (nt == 1))).view(-1, 1, 1)).any(0)
    return refs_u[:, None].numpy(), inv_u[None].numpy()


def packages(img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau, dtype=torch.float64):
    """``Referencer.forward`` after its FPN calls: (packages [bs, 12, H, W], (inv, inv_target), present).  The mask, grey and background channels are float32
    expressions of float32 inputs whatever ``dtype`` is (they are exact); the six reference channels are in ``dtype``."""
    img_a, img_t = torch.as_tensor(img_a, dtype=torch.float32), torch.as_tensor(img_t, dtype=torch.float32)
    pa, pt, head_a, _, e_at = part_masks(labels_a, labels_t)
    refs, present, inv, inv_target = color_reference(img_t, feats_a, feats_t, pa, pt, tau, True, dtype)
    refs = torch.from_numpy(refs)
    gate = torch.from_numpy((present.sum(1) >= 2)).to(dtype).view(-1, 1, 1, 1)
    six = torch.cat([refs[:, :-1].sum(1), refs[:, -1]], dim=1) * gate
    six = F.interpolate(six, size=img_t.shape[-2:], mode="bilinear", align_corners=True)
    head_a, e_at = torch.from_numpy(head_a), torch.from_numpy(e_at)
    a01 = torch.stack([denorm(i) for i in img_a])
    grey = (a01[:, 0] * 0.299 + a01[:, 1] * 0.587 + a01[:, 2] * 0.114).clamp(0, 1)[:, None] * head_a
    rest = torch.cat([head_a, torch.from_numpy(pa[:, -1:]).float(), grey, img_t * (1 - e_at)], dim=1)
    return torch.cat([six, rest.to(dtype)], dim=1).numpy(), (inv, inv_target), present


# ------------------------------------------------------------------------------------------------ seeded inputs
def features(seed, bs, h, w):
    """float32 [bs, 256, h, w]: a rank-8 field plus noise, so that cosines between pixels spread over (-1, 1) instead of crowding at 0."""
    rs = np.random.RandomState(seed)
    low = np.einsum("bdk,bkp->bdp", rs.randn(bs, D, 8), rs.randn(bs, 8, h * w))
    return (low + 0.7 * rs.randn(bs, D, h * w) + 0.3 * rs.randn(bs, 1, h * w)).reshape(bs, D, h, w).astype(np.float32)


def image(seed, bs, H, W):
    """float32 [bs, 3, H, W], ImageNet-normalised, reaching past [0, 1] after de-normalisation so that the clamp acts."""
    rs = np.random.RandomState(seed)
    rgb = rs.uniform(-0.1, 1.1, (bs, 3, H, W))
    return ((rgb - np.array(MEAN).reshape(1, 3, 1, 1)) / np.array(STD).reshape(1, 3, 1, 1)).astype(np.float32)


def blocky_labels(seed, bs, H, W, cell, classes=19):
    """uint8 [bs, H, W]: one random class of 0 .. classes - 1 per cell x cell block."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, classes, (bs, -(-H // cell), -(-W // cell))).astype(np.uint8)
    return np.kron(lab, np.ones((cell, cell), np.uint8))[:, :H, :W]


def masks_from_ranges(ranges_a, ranges_t, h, w, up):
    """Hand-built part masks: per part a (start, stop) range of flat feature-size pixels (None = empty), blown up ``up`` times.  uint8 [1, 9, h up, w up]."""
    out = []
    for ranges in (ranges_a, ranges_t):
        m = np.zeros((len(PARTS), h * w), np.uint8)
        for p, r in enumerate(ranges):
            if r is not None:
                m[p, r[0]:r[1]] = 1
        out.append(np.kron(m.reshape(len(PARTS), h, w), np.ones((up, up), np.uint8))[None])
    return out


# (i): 12 x 20 features from 48 x 80 maps.  skin 130 / 130 with half of T's pixels outside A's mask; hair 63 / 64 with ALL of T's pixels outside A's mask (every
# key a zero key: the plain mean of their RGB); eye 64 / 65; nose 65 / 63; lip one pixel of A; tooth absent in A only; ear absent in T only; brow one pixel of T
HAND_A = ((0, 130), (0, 63), (10, 74), (150, 215), (5, 6), None, (200, 220), (220, 240), (100, 140))
HAND_T = ((60, 190), (100, 164), (20, 85), (150, 213), (5, 8), (30, 40), None, (215, 216), (90, 150))
HAND_TAUS = (1.0, 12.0, 40.0, -5.0)
HAND_PRESENT = ("skin", "hair", "eye", "nose", "lip", "brow", "inpainting")


def case_hand():
    """(img_t, feats_a, feats_t, parts_a, parts_t) of case (i), batch 1."""
    pa, pt = masks_from_ranges(HAND_A, HAND_T, 12, 20, 4)
    return image(101, 1, 48, 80), features(102, 1, 12, 20), features(103, 1, 12, 20), pa, pt


def case_forward():
    """(img_a, img_t, labels_a, labels_t, feats_a, feats_t, tau) of case (ii): 24 x 24 features from 96 x 96 blocky maps."""
    return (image(201, 1, 96, 96), image(202, 1, 96, 96), blocky_labels(203, 1, 96, 96, 12), blocky_labels(204, 1, 96, 96, 12),
            features(205, 1, 24, 24), features(206, 1, 24, 24), 7.0)


def case_large():
    """(img_t, feats_a, feats_t, parts_a, parts_t, tau) of case (iii): 64 x 64 features from 256 x 256 blocky maps, parts of some hundred pixels."""
    pa, pt, _, _, _ = part_masks(blocky_labels(303, 1, 256, 256, 32), blocky_labels(304, 1, 256, 256, 32))
    return image(301, 1, 256, 256), features(305, 1, 64, 64), features(306, 1, 64, 64), pa, pt, 7.0


def case_two_class():
    """Case (iv), as ``case_forward``: maps of background and skin only — skin and inpainting are the two present parts."""
    la, lt = np.zeros((1, 96, 96), np.uint8), np.zeros((1, 96, 96), np.uint8)
    la[:, 30:70, 24:60] = 1
    lt[:, 20:64, 36:80] = 1
    return image(401, 1, 96, 96), image(402, 1, 96, 96), la, lt, features(405, 1, 24, 24), features(406, 1, 24, 24), 7.0


def part_dicts(parts_a, parts_t):
    """The reference's two part dictionaries (int64 [bs, H, W] masks, 'head' = the sum of the eight parts, then 'inpainting') from uint8 [bs, 9, H, W]."""
    out = []
    for parts in (parts_a, parts_t):
        m = torch.as_tensor(parts).long()
        d = {n: m[:, i] for i, n in enumerate(PARTS[:-1])}
        d["head"] = sum(d.values())
        d["inpainting"] = m[:, -1]
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ cases the reference cannot run cheaply (model only)
def case_big():
    """(img_t, feats_a, feats_t, parts_a, parts_t, tau): one 2300-pixel part on both sides at 64 x 64 (72 x 72 tiles of 32, the last ragged, 1500 of T's
    pixels outside A's mask) and a small inpainting part."""
    ra, rt = [None] * 9, [None] * 9
    ra[0], rt[0], ra[8], rt[8] = (100, 2400), (900, 3200), (3300, 3403), (3500, 3590)
    pa, pt = masks_from_ranges(ra, rt, 64, 64, 4)
    return image(501, 1, 256, 256), features(502, 1, 64, 64), features(503, 1, 64, 64), pa, pt, 12.0


def case_full():
    """One part of exactly 4096 pixels on both sides: the full 64 x 64 plane, from 128 x 128 maps."""
    ra, rt = [None] * 9, [None] * 9
    ra[0] = rt[0] = (0, 4096)
    pa, pt = masks_from_ranges(ra, rt, 64, 64, 2)
    return image(601, 1, 128, 128), features(602, 1, 64, 64), features(603, 1, 64, 64), pa, pt, 7.0


BATCH3_ABSENT = ("hair", "tooth", "brow")


def case_batch3():
    """As ``case_forward`` at batch 3, 64 x 64 features from 256 x 256 maps with all nine parts, except that sample b lacks ``BATCH3_ABSENT[b]``: hair in A
    only, tooth in T only, brow on both sides."""
    la, lt = blocky_labels(703, 3, 256, 256, 16), blocky_labels(704, 3, 256, 256, 16)
    la[0][la[0] == 17] = 0
    lt[1][lt[1] == 11] = 0
    for lab in (la, lt):
        lab[2][(lab[2] == 2) | (lab[2] == 3)] = 0
    return image(701, 3, 256, 256), image(702, 3, 256, 256), la, lt, features(705, 3, 64, 64), features(706, 3, 64, 64), 7.0


def reference_inputs(tag):
    """(img_t, feats_a, feats_t, parts_a, parts_t, tau) of a ``color_reference`` case by name ('hand.tau12', 'forward', 'large', 'two_class', 'big', 'full',
    'batch3')."""
    if tag.startswith("hand.tau"):
        return case_hand() + (float(tag[len("hand.tau"):]),)
    if tag in ("forward", "two_class", "batch3"):
        _, img_t, la, lt, fa, ft, tau = {"forward": case_forward, "two_class": case_two_class, "batch3": case_batch3}[tag]()
        pa, pt, _, _, _ = part_masks(la, lt)
        return img_t, fa, ft, pa, pt, tau
    return {"large": case_large, "big": case_big, "full": case_full}[tag]()


FIXTURE_REFER_CASES = tuple(f"hand.tau{t:g}" for t in HAND_TAUS) + ("forward", "large", "two_class")
MODEL_ONLY_CASES = ("big", "full", "batch3")
_CACHE = {}


def reference_outputs(tag, dtype=torch.float64):
    """``color_reference`` of a named case, computed once per session and shared (do not write into the arrays)."""
    key = (tag, dtype)
    if key not in _CACHE:
        _CACHE[key] = color_reference(*reference_inputs(tag), True, dtype)
    return _CACHE[key]


def max_err(got, want):
    """The largest absolute difference over corresponding arrays."""
    return max(float(np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64)).max()) for g, w in zip(got, want))
