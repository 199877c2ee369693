"""Row f25 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.inpaint_forward`` against ``ops.FaceInpainting.forward`` run by stock PyTorch on the same device with the same seeded weights and noise, at 256 x 256
  (the caller's size), batch 1 and 8, eager and captured in a graph;
* ``pipeline.inpaint_faces`` (512 x 512 faces and masks in, the two resizes, the network, the uint8 composite) at the same batches;
* per decoder layer at batch 1 (``--layers``): the up layers on both routes they can take, every same-resolution layer with its scale-shift epilogue, the other
  entries of csrc/gcfsr.hip, and the share of that file's entries in the whole ``inpaint_image`` call.

    python tools/time_inpaint.py [--rounds 5] [--layers] [--json out.json]
    python tools/time_inpaint.py --profile-pass            # a few native calls at batch 1 and nothing else: the run to put under
                                                           # rocprofv3 --kernel-trace --stats for the per-kernel shares

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  No ratio is expected in advance:
the baseline is the stock forward, the numbers are reported as measured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import inpaint_model as M
from e4s2024_amd import netweights, ops, ops_inpaint, pipeline, sg2net
from time_resunet import alternate, graphed

dev = "cuda:0"
SIZE = 256
WARMUP = 20                                  # calls of either route before a batch size is timed


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def inputs(bs):
    faces = torch.from_numpy(M.GM.images_u8(5, bs, 2 * SIZE)).to(dev)
    yy, xx = torch.meshgrid(torch.arange(2 * SIZE, device=dev), torch.arange(2 * SIZE, device=dev), indexing="ij")
    mask = ((((yy - 280) / 150.0) ** 2 + ((xx - 240) / 110.0) ** 2) < 1).float()[None].repeat(bs, 1, 1).contiguous()
    small, hole = ops.pil_resize(faces, (SIZE, SIZE)), ops.cv_mask_support(mask, SIZE)
    x, in_size, _ = ops.inpaint_input(small, hole)
    noise = [torch.randn(bs, 1, r, r, device=dev) for r in ops_inpaint.noise_sizes(SIZE)]
    return faces, mask, small, hole, x, in_size, noise


def layer_table(net, rounds):
    """Time of every decoder entry at batch 1 on buffers of the layer's shapes (the time does not depend on the values), the up layers on both routes."""
    checked = ops_inpaint._weights_checked("time_inpaint", net)
    rows, own = [], {}
    default_width = ops_inpaint.UP_COMPOSED_MAX_WIDTH
    new = lambda *s: torch.randn(s, device=dev)          # noqa: E731
    for width, label in ((default_width, "default"), (0, "up layers fused"), (4096, "up layers composed")):
        ops_inpaint.UP_COMPOSED_MAX_WIDTH = width
        P = netweights.prepare(ops_inpaint.PreparedInpaint, net, checked)
        h = 16
        for i, L in enumerate(P["convs"]):
            ho = 2 * h if L["up"] else h
            x, y, s, d, nz = new(1, L["cin"], h, h), new(1, L["cout"], ho, ho), new(L["cin"]), new(L["cout"]).abs(), new(1, 1, ho, ho)
            if label == "default" or L["up"]:
                route = ("composed" if L["composed"] else "fused") if L["up"] else "same"
                bias, act = (None, 0) if L["norm"] else (L["bias"], 1)
                fn = lambda: sg2net.modconv(L, x, y, s, d, sb=P["sb"], blur=P["fir4"], noise=nz, bias=bias, act=act, bs=1, h=h, st=ops._stream())      # noqa: E731
                ms = statistics.median(alternate({"l": fn}, rounds, 20)["l"])
                rows.append((label, f"decoder {L['cin']:4d} -> {L['cout']:3d} @ {h:3d}{' up' if L['up'] else '   '}", route, ms))
            if label == "default" and L["norm"]:
                sh, t1, t2 = new(1, L["cout"], ho, ho), new(1, L["cout"]), new(1, L["cout"])
                ms = statistics.median(alternate({"l": lambda: ops.scale_shift_act(y, sh, t1, t2, L["bias"])}, rounds, 20)["l"])
                rows.append((label, f"epilogue {L['cout']:3d} @ {ho:3d} scale, shift, bias, lrelu", "gcfsr", ms))
                own[f"scale_shift_act {L['cout']} @ {ho}"] = ms
            h = ho
    ops_inpaint.UP_COMPOSED_MAX_WIDTH = default_width
    return rows, own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    net = ops.FaceInpainting(SIZE).eval()
    net.load_state_dict(M.state_dict(SIZE))
    net = net.to(dev)
    if a.profile_pass:
        _, _, small, hole, _, _, noise = inputs(1)
        for _ in range(6):
            ops.inpaint_image(small, hole, net, noise)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_inpaint", "profile_pass": True, "calls": 6, "ok": True}))
        return
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"inpaint_forward against ops.FaceInpainting.forward on stock PyTorch, size {SIZE}, {doc['device']}")
    for bs in (1, 8):
        faces, mask, small, hole, x, in_size, noise = inputs(bs)
        want = net(x, in_size, noise)[0]
        agree = float((ops.inpaint_forward(x, in_size, net, noise)[0] - want).abs().max())
        for _ in range(WARMUP):                                                                # the clocks settle: the first block is timed like the later ones
            ops.inpaint_forward(x, in_size, net, noise)
            net(x, in_size, noise)
        fns = {"hip": lambda: ops.inpaint_forward(x, in_size, net, noise), "torch": lambda: net(x, in_size, noise),
               "faces": lambda: pipeline.inpaint_faces(net, faces, mask, noise=noise)}
        for mode in ("eager", "graph"):
            if mode == "graph":
                fns = {k: graphed(fn) for k, fn in fns.items()}
            res = alternate(fns, a.rounds, 3)
            s = spread(res)
            for k, v in s.items():
                what = {"hip": "inpaint_forward", "torch": "stock forward", "faces": "inpaint_faces"}[k]
                print(f"  bs {bs} {mode:5s} {what:15s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}", flush=True)
            faster = max(res["hip"]) < min(res["torch"])
            print(f"  bs {bs} {mode}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch round: {faster}",
                  flush=True)
            doc["cases"][f"network bs{bs} {mode}"] = {**s, "hip_not_slower_beyond_spread": faster, "outputs_agree_to": agree}
        print(f"  bs {bs}: outputs agree to {agree:.1e} (max |out| {float(want.abs().max()):.2f})", flush=True)
    if a.layers:
        rows, own = layer_table(net, a.rounds)
        for label, name, route, ms in rows:
            print(f"  [{label:18s}] {name:48s} {route:9s} {ms * 1e3:9.1f} us", flush=True)
        faces, mask, small, hole, x, in_size, noise = inputs(1)
        img = ops.inpaint_forward(x, in_size, net, noise)[0]
        sd = net.state_dict()
        lv = [[(sd[f"condition_scale{k}.{j}.weight"], sd[f"condition_scale{k}.{j}.bias"]) for j in range(5)] for k in (1, 2)]
        ends = {"inpaint_input": lambda: ops.inpaint_input(small, hole), "inpaint_condition": lambda: ops.inpaint_condition(in_size, lv[0], lv[1]),
                "inpaint_tail": lambda: ops.inpaint_tail(img, small, hole), "cv_mask_support 512 -> 256": lambda: ops.cv_mask_support(mask, SIZE)}
        for k, v in alternate(ends, a.rounds, 20).items():
            own[k] = statistics.median(v)
            print(f"  [default           ] {k:48s} {'gcfsr':9s} {own[k] * 1e3:9.1f} us", flush=True)
        whole = statistics.median(alternate({"g": graphed(lambda: ops.inpaint_image(small, hole, net, noise))}, a.rounds, 5)["g"])
        in_call = sum(v for k, v in own.items() if not k.startswith("cv_mask"))
        print(f"  inpaint_image bs 1 as a graph: {whole:.3f} ms; csrc/gcfsr.hip's entries in it, each timed alone (launch included): {in_call:.3f} ms = "
              f"{100 * in_call / whole:.1f} %, of which scale_shift_act {sum(v for k, v in own.items() if k.startswith('scale')):.3f} ms", flush=True)
        doc["cases"]["gcfsr share bs1"] = {"inpaint_image_graph_ms": whole, "gcfsr_entries_ms": in_call, "entries": own}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_inpaint", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
