"""Row f14 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.retinaface_detect`` (uint8 frames to detections, everything on the device, one read of the counts) against the parent path on the same GPU with the
  same seeded weights: ``ops.RetinaFace.forward`` run by stock PyTorch, then the host side as ``RetinaFaceDetection.detect`` writes it — the priors from a
  Python double loop over every anchor, ``decode`` / ``decode_landm`` as tensor expressions, three copies to the host, threshold, argsort and a numpy
  ``py_cpu_nms`` — as ``parent_tail`` below spends it, on the restatement of ``tests/retinaface_model.py``.  1024 x 1024 (what the live path feeds: the 4 x super-resolved 256 x 256 frame) at batch 1 and 4, eager
  and captured in a graph (the parent's graph holds its network; its host side cannot be captured).

    python tools/time_retinaface.py [--rounds 5] [--json out.json]
    python tools/time_retinaface.py --profile-pass         # a few native calls at batch 1 and nothing else: the run to put under
                                                           # rocprofv3 --kernel-trace for the per-kernel shares (tools/rocpd_summary.py)

The seeded class heads would put a third of the 43 008 anchors above the 0.9 score, which no photograph does and which would time the parent's Python NMS on
5 000 boxes.  The tool lowers the class-1 biases so that about ``CANDIDATES`` anchors of the first frame pass, and prints the counts it then sees.
Each figure is the median over the rounds with the min .. max of the rounds beside it.  The native route counts as not slower only if its slowest round is below
the parent's fastest."""
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

import retinaface_model as RM
from e4s2024_amd import ops, seeded
from time_resunet import alternate, graphed

dev = "cuda:0"
SIZE = 1024
WARMUP = 10                                  # calls of either route before a batch size is timed
CANDIDATES = 60


def parent_priors(H, W):
    """The parent's prior boxes, float32 ``[N, 4]``: one Python iteration per anchor, which is what ``PriorBox.forward`` spends on them (the vectorised
    ``retinaface_model.priors`` gives the same values and would flatter the parent)."""
    flat = []                                    # a flat list: torch.tensor is slower on nested rows
    for (h, w), step, sizes in zip(RM.level_sizes(H, W), RM.STEPS, RM.MIN_SIZES):
        for y in range(h):
            for x in range(w):
                for ms in sizes:
                    flat.extend(((x + 0.5) * step / W, (y + 0.5) * step / H, ms / W, ms / H))
    return torch.tensor(flat, dtype=torch.float32).view(-1, 4)


def parent_tail(loc, conf, landms, H, W, conf_t=RM.CONF_T, nms_t=RM.NMS_T, top_k=RM.TOP_K, keep_top_k=RM.KEEP_TOP_K):
    """The host side of the parent path for one image, with the work where ``detect`` has it: the priors from the Python loop, the two decodes as tensor
    expressions on the device, three copies to the host, then threshold, sort and the greedy NMS in numpy (``retinaface_model.nms`` on the float32 boxes)."""
    pr = parent_priors(H, W).to(loc.device)
    centre, size = pr[:, :2], pr[:, 2:]
    v0, v1 = RM.VARIANCE
    wh = size * torch.exp(loc[:, 2:] * v1)
    x1y1 = centre + loc[:, :2] * v0 * size - wh / 2
    boxes = torch.cat([x1y1, wh + x1y1], 1) * pr.new_tensor([W, H, W, H])
    lm = (centre.repeat(1, 5) + landms * v0 * size.repeat(1, 5)) * pr.new_tensor([W, H] * 5)
    boxes, scores, lm = boxes.cpu().numpy(), conf[:, 1].cpu().numpy(), lm.cpu().numpy()
    cand = np.flatnonzero(scores > conf_t)
    cand = cand[np.argsort(-scores[cand], kind="stable")][:top_k]
    rows = cand[RM.nms(boxes[cand], nms_t)[:keep_top_k]]
    dets = np.concatenate([boxes[rows], scores[rows, None]], 1).astype(np.float32)
    return dets, lm[rows].reshape(-1, 5, 2).transpose(0, 2, 1).reshape(-1, 10)


def parent_detect(forward, x):
    """The parent path for a batch: one network pass (``forward``: stock PyTorch, eager or a graph replay), then the host side image by image."""
    loc, conf, landms = forward()
    return [parent_tail(loc[b], conf[b], landms[b], x.shape[2], x.shape[3]) for b in range(x.shape[0])]


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--size", type=int, default=SIZE)
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    size = a.size
    net = ops.RetinaFace().eval()
    net.load_state_dict(seeded.seeded_retinaface_state_dict(RM.WEIGHT_SEEDS["A"]), strict=True)
    net = net.to(dev)
    frames = lambda bs: torch.from_numpy(RM.images_u8(5, bs, size, size)).to(dev)              # noqa: E731
    to_x = lambda img: torch.from_numpy(RM.to_input(img.cpu().numpy())).to(dev)                # noqa: E731
    # a photograph's candidate count: lower the class-1 biases until about CANDIDATES anchors of the first frame pass
    conf = net(to_x(frames(1)))[1][0]
    d = torch.log(conf[:, 1]) - torch.log(conf[:, 0])
    top = torch.sort(d, descending=True)[0]
    shift = float(top[CANDIDATES - 1] + top[CANDIDATES]) / 2 - float(np.log(0.9 / 0.1))          # the threshold midway between two anchors, not on one
    with torch.no_grad():
        for h in net.ClassHead:
            h.conv1x1.bias[1::2] -= shift
    if a.profile_pass:
        img = frames(1)
        for _ in range(6):
            ops.retinaface_detect(img, net)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_retinaface", "profile_pass": True, "calls": 6, "ok": True}))
        return
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "size": size, "cases": {}}
    print(f"retinaface_detect against stock net(x) + the reference's host side, {size} x {size}, {ops.retinaface_level_sizes(size, size)[1]} anchors, {doc['device']}; "
          f"class-1 biases lowered by {shift:.2f}")
    for bs in (1, 4):
        img = frames(bs)
        x = to_x(img)
        want = parent_detect(lambda: net(x), x)
        got = ops.retinaface_detect(img, net)
        counts = [(len(w[0]), len(g[0])) for w, g in zip(want, got)]
        agree = max([float(np.abs(g[0].cpu().numpy() - w[0]).max()) for w, g in zip(want, got) if len(w[0]) == len(g[0]) and len(w[0])] or [float("nan")])
        for _ in range(WARMUP):
            ops.retinaface_detect(img, net)
            net(x)
        for mode in ("eager", "graph"):
            if mode == "eager":
                fns = {"hip": lambda: ops.retinaface_detect(img, net), "parent": lambda: parent_detect(lambda: net(x), x)}
            else:
                out = {}
                replay_hip = graphed(lambda: out.__setitem__("hip", ops.retinaface_detect_padded(img, net)))
                replay_net = graphed(lambda: out.__setitem__("net", net(x)))

                def hip():
                    replay_hip()
                    dets, lm, nkeep = out["hip"]
                    return [(dets[b, :n], lm[b, :n]) for b, n in enumerate(nkeep.tolist())]

                def replayed():
                    replay_net()
                    return out["net"]

                fns = {"hip": hip, "parent": lambda: parent_detect(replayed, x)}
            res = alternate(fns, a.rounds, 3)
            s = spread(res)
            for k, v in s.items():
                print(f"  detect bs {bs} {mode:5s} {k:6s}: median {v['median_ms']:9.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}", flush=True)
            faster = max(res["hip"]) < min(res["parent"])
            print(f"  detect bs {bs} {mode}: parent / hip = {s['parent']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest parent round: "
                  f"{faster}", flush=True)
            doc["cases"][f"detect bs{bs} {mode}"] = {**s, "hip_not_slower_beyond_spread": faster}
        # the network alone, so that the host side's share of the parent path can be read off
        res = alternate({"hip": lambda: ops.retinaface_forward(x, net), "torch": lambda: net(x)}, a.rounds, 3)
        s = spread(res)
        print(f"  forward bs {bs} eager: hip median {s['hip']['median_ms']:.3f} ms ({s['hip']['min_ms']:.3f} .. {s['hip']['max_ms']:.3f}), torch "
              f"{s['torch']['median_ms']:.3f} ms ({s['torch']['min_ms']:.3f} .. {s['torch']['max_ms']:.3f})", flush=True)
        doc["cases"][f"forward bs{bs} eager"] = s
        print(f"  bs {bs}: detections (parent, hip) per frame {counts}, boxes agree to {agree:.1e} pixels", flush=True)
        doc["cases"][f"agreement bs{bs}"] = {"counts_parent_hip": counts, "boxes_agree_to": agree}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_retinaface", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
