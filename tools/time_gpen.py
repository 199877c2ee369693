"""Row f12 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round:

* ``ops.gpen_forward`` against ``ops.GPEN.forward`` run by stock PyTorch on the same device with the same seeded weights, the default network
  (512, narrow 1: GPEN-BFR-512's shapes) at batch 1 and 4, eager and captured in a graph;
* per decoder layer and encoder level, the native entry's time at batch 1 (``--layers``; the up layers under both routes they can take);
* the whole native call at batch 1 with the composed / fused threshold of the up layers moved (``--routes``).

    python tools/time_gpen.py [--rounds 5] [--layers] [--routes] [--json out.json]
    python tools/time_gpen.py --profile-pass               # a few native calls at batch 1 and nothing else: the run to put under
                                                           # rocprofv3 --kernel-trace --stats for the per-kernel shares

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The multiply-adds are counted
from the layer shapes (``flop``) and printed with the rate they give."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import gpen_model as GM
from e4s2024_amd import netweights, ops, ops_gpen, seeded, sg2net
from time_resunet import alternate, graphed

dev = "cuda:0"
SIZE, SDIM, N_MLP = 512, 512, 8
WARMUP = 30                                  # calls of either route before a batch size is timed


def flop(size=SIZE, channel_multiplier=2, narrow=1):
    """(encoder, decoder) multiply-adds x 2 of one sample, from the layer shapes; the decoder's up layers at the transposed convolution's count."""
    ch = ops_gpen.gpen_channels(channel_multiplier, narrow)
    enc = 3 * ch[size] * size * size
    r = size
    while r > 4:
        enc += 9 * ch[r] * ch[r // 2] * (r // 2) ** 2
        r //= 2
    dec = 9 * ch[4] * ch[4] * 16 + 3 * 2 * ch[4] * 16
    r, cin = 8, ch[4]
    while r <= size:
        dec += 9 * 2 * cin * ch[r] * (r // 2) ** 2 + 9 * 2 * ch[r] * ch[r] * r * r + 3 * 2 * ch[r] * r * r
        cin, r = ch[r], 2 * r
    return 2 * enc, 2 * dec


def spread(res):
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in res.items()}


def layer_table(net, x, rounds):
    """Time of every convolution entry of one native call at batch 1, each on the buffers the call leaves behind."""
    checked = ops_gpen._weights_checked("time_gpen", net)
    rows = []
    default_width = ops_gpen.UP_COMPOSED_MAX_WIDTH
    for width, label in ((ops_gpen.UP_COMPOSED_MAX_WIDTH, "default"), (0, "up layers fused"), (4096, "up layers composed")):
        ops_gpen.UP_COMPOSED_MAX_WIDTH = width
        P = netweights.prepare(ops_gpen.PreparedGPEN, net, checked)
        S = ops_gpen._scratch(P, x.device)
        out = torch.empty((1, 3, SIZE, SIZE), device=dev)
        lat = torch.empty((1, 1, SDIM), device=dev)
        ops_gpen._gpen_sample(P, S, x[:1], None, out, lat)
        conv_t, _ = ops_gpen._tables(P, S, lat)
        h = 4
        for i, L in enumerate(P["convs"]):
            src = P["const"] if i == 0 else S["outs"][i - 1]
            fn = lambda L=L, src=src, i=i, h=h: sg2net.modconv(L, src, S["outs"][i][:, :L["cout"]], *conv_t[i], sb=P["sb"], blur=L["blur"],      # noqa: E731
                                                               bias=L["bias"], act=1, bs=1, h=h, st=ops._stream())
            if label == "default" or L["up"]:
                route = ("composed" if L["composed"] else "fused") if L["up"] else "same"
                ms = statistics.median(alternate({"l": fn}, rounds, 20)["l"])
                rows.append((label, f"decoder {L['cin']:4d} -> {L['cout']:3d} @ {h:3d}{' up' if L['up'] else '   '}", route, ms))
            if L["up"]:
                h *= 2
        if label == "default":
            r = SIZE
            for L, s_, d_, blur in zip(P["enc"], S["feats"][:-1], S["feats"][1:], S["blurs"]):
                enc = lambda L=L, s_=s_, d_=d_, r=r, blur=blur: sg2net.conv3x3(L, s_, d_, 1, r, P["sb"], ops._stream(), L["fir"], blur)      # noqa: E731
                ms = statistics.median(alternate({"l": enc}, rounds, 20)["l"])
                rows.append((label, f"encoder {L['cin']:4d} -> {L['cout']:3d} @ {r:3d} blur + conv", "sb", ms))
                r //= 2
    ops_gpen.UP_COMPOSED_MAX_WIDTH = default_width
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--routes", action="store_true")
    ap.add_argument("--profile-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    net = ops.GPEN(SIZE, SDIM, N_MLP, 2, 1).eval()
    net.load_state_dict(seeded.seeded_gpen_state_dict(GM.WEIGHT_SEED, SIZE, SDIM, N_MLP, 2, 1))
    net = net.to(dev)
    image = lambda bs: torch.from_numpy(GM.img2tensor(GM.images_u8(5, bs, SIZE))).to(dev)      # noqa: E731
    if a.profile_pass:
        x = image(1)
        for _ in range(6):
            ops.gpen_forward(x, net)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_gpen", "profile_pass": True, "calls": 6, "ok": True}))
        return
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    enc, dec = flop()
    print(f"gpen_forward against ops.GPEN.forward on stock PyTorch, size {SIZE}, narrow 1, {doc['device']}; per sample {enc / 1e9:.1f} GFLOP encoder + "
          f"{dec / 1e9:.1f} GFLOP decoder counted")
    for bs in (1, 4):
        x = image(bs)
        want = net(x)[0]
        agree = float((ops.gpen_forward(x, net)[0] - want).abs().max())
        for _ in range(WARMUP):                                                                # the clocks settle: the first block is timed like the later ones
            ops.gpen_forward(x, net)
            net(x)
        gflop = bs * (enc + dec) / 1e9
        fns = {"hip": lambda: ops.gpen_forward(x, net), "torch": lambda: net(x)}
        for mode in ("eager", "graph"):
            if mode == "graph":
                fns = {k: graphed(fn) for k, fn in fns.items()}
            res = alternate(fns, a.rounds, 3)
            s = spread(res)
            for k, v in s.items():
                print(f"  network bs {bs} {mode:5s} {k:5s}: median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. {v['max_ms']:.3f}   "
                      f"{gflop / v['median_ms']:.1f} TFLOP/s of {gflop:.1f} GFLOP counted", flush=True)
            faster = max(res["hip"]) < min(res["torch"])
            print(f"  network bs {bs} {mode}: torch / hip = {s['torch']['median_ms'] / s['hip']['median_ms']:.2f}x, slowest hip round below fastest torch round: "
                  f"{faster}", flush=True)
            doc["cases"][f"network bs{bs} {mode}"] = {**s, "hip_not_slower_beyond_spread": faster, "gflop_counted": gflop, "outputs_agree_to": agree}
        print(f"  network bs {bs}: outputs agree to {agree:.1e} (max |out| {float(want.abs().max()):.2f})", flush=True)
    x = image(1)
    default_width = ops_gpen.UP_COMPOSED_MAX_WIDTH
    if a.routes:
        for width in (0, 4, 8, 16, 32, 64, 4096):
            ops_gpen.UP_COMPOSED_MAX_WIDTH = width
            v = spread(alternate({"hip": lambda: ops.gpen_forward(x, net)}, a.rounds, 3))["hip"]
            print(f"  up layers composed up to input width {width:4d}, fused above: bs 1 eager median {v['median_ms']:8.3f} ms   rounds {v['min_ms']:.3f} .. "
                  f"{v['max_ms']:.3f}", flush=True)
            doc["cases"][f"routes composed<={width}"] = v
        ops_gpen.UP_COMPOSED_MAX_WIDTH = default_width
    if a.layers:
        for label, name, route, ms in layer_table(net, x, a.rounds):
            print(f"  [{label:18s}] {name:40s} {route:9s} {ms * 1e3:9.1f} us", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_gpen", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
