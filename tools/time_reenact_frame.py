"""Row f20 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round: a reenacted frame of face-vid2vid
at the upstream vox-256 configuration (256 x 256 source, decoder input ``[bs, 256, 64, 64]``, 15 keypoints, the occlusion head), seeded weights:

* the decoder alone, ``ops.spade_decoder_forward`` against the mirror's ``SPADEDecoder`` on stock PyTorch, same device, same weights (and both outputs
  against that mirror run in float64 on the device);
* a frame, ``ops.generator_frames`` on the held source feature, against what the parent commit offers for a frame: the native front
  (``ops.generator_warp``) followed by ``generator.decoder`` on stock PyTorch;
* both at batch 1 and batch ``--batch``, eager and replayed from a captured graph;
* with ``--trace``, the device time of every entry point of one native frame, each timed alone, summed per entry point;
* the multiply-adds per part of the decoder, counted from the layer shapes.

    python tools/time_reenact_frame.py [--batch 4] [--rounds 5] [--trace] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from e4s2024_amd import ops, seeded
from e4s2024_amd import ops_reenact_frames as RF
from time_generator_front import trace
from time_reenact import show
from time_resunet import alternate, graphed

dev = "cuda:0"
SEED = 20


def decoder_macs(h, w):
    """{part: multiply-adds of one sample} of the SPADEDecoder on an ``h x w`` feature, from the layer shapes."""
    out = {"fc": 9 * 256 * 512 * h * w}
    for p, fin, fout, up in RF._BLOCKS:
        h, w = h * up, w * up
        mid = min(fin, fout)
        norms = 9 * 256 * 128 * (3 if fin != fout else 2) + 9 * 128 * 2 * (fin + mid + (fin if fin != fout else 0))
        convs = 9 * fin * mid + 9 * mid * fout + (fin * fout if fin != fout else 0)
        part = "G_middle" if p.startswith("G_middle") else p
        out[part] = out.get(part, 0) + (norms + convs) * h * w
        out[part + " (its SPADE norms)"] = out.get(part + " (its SPADE norms)", 0) + norms * h * w
    out["conv_img"] = 9 * 64 * 3 * h * w
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"face-vid2vid reenacted frame at the upstream configuration, source 256 x 256, decoder input [bs, 256, 64, 64], {doc['device']}")
    net = ops.OcclusionAwareSPADEGenerator().eval()
    template = {k: torch.empty(s, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32, device="meta")
                for k, s in ops.generator_state_dict_shapes().items()}
    net.load_state_dict(seeded.seeded_generator_state_dict(template, SEED), strict=True)
    net = net.to(dev)
    K = net.structure[9][0]
    parts = decoder_macs(64, 64)
    total = sum(v for k, v in parts.items() if "(" not in k)
    doc["gmac"] = {k: v / 1e9 for k, v in parts.items()}
    print("  decoder per sample: " + ", ".join(f"{k} {v / 1e9:.1f}" for k, v in parts.items()) + f"; in all {total / 1e9:.1f} GMAC", flush=True)

    source = torch.from_numpy(seeded.seeded_array(SEED, "source", (1, 3, 256, 256), 0.5, 0.25)).clamp_(0, 1).to(dev)
    f3 = ops.appearance_feature(source, net)
    decoder64 = copy.deepcopy(net.decoder).double()
    for bs in sorted({1, a.batch}):
        ks = torch.from_numpy(seeded.seeded_array(SEED, f"kp_s{bs}", (1, K, 3), 0.0, 0.3)).to(dev).expand(bs, -1, -1).contiguous()
        kd = (ks + torch.from_numpy(seeded.seeded_array(SEED, f"kp_d{bs}", (bs, K, 3), 0.0, 0.15)).to(dev)).contiguous()
        kd, ks = {"value": kd}, {"value": ks}
        feature = ops.generator_warp(f3, kd, ks, net)["feature"]
        got, want = ops.spade_decoder_forward(feature, net), net.decoder(feature)
        want64 = decoder64(feature.double())             # the same mirror in float64 on the device: which of the two float32 paths is the closer one
        print(f"  spade_decoder_forward batch {bs} against the mirror on stock PyTorch: {float((got - want).abs().max()):.2e} (prediction {float(got.min()):.3f} .. "
              f"{float(got.max()):.3f}, std {float(got.std()):.3f}); against the mirror in float64: hip {float((got - want64).abs().max()):.2e}, "
              f"torch {float((want - want64).abs().max()):.2e}", flush=True)
        del want64
        parent = lambda: net.decoder(ops.generator_warp(f3, kd, ks, net)["feature"])      # noqa: E731   what the parent commit offers for a frame
        res = alternate({"hip": lambda: ops.spade_decoder_forward(feature, net), "torch": lambda: net.decoder(feature)}, a.rounds, 3)
        show(doc, f"decoder batch {bs}", res, f"   ({2 * bs * total / 1e9:.0f} GFLOP counted)")
        res = alternate({"hip": lambda: ops.generator_frames(f3, kd, ks, net), "torch": parent}, a.rounds, 3)
        show(doc, f"frame batch {bs} (torch: the native front, then generator.decoder on stock PyTorch)", res)
        res = alternate({"hip": graphed(lambda: ops.spade_decoder_forward(feature, net)), "torch": graphed(lambda: net.decoder(feature))}, a.rounds, 3)
        show(doc, f"decoder batch {bs} replayed from a graph", res)
        res = alternate({"hip": graphed(lambda: ops.generator_frames(f3, kd, ks, net)), "torch": graphed(parent)}, a.rounds, 3)
        show(doc, f"frame batch {bs} replayed from a graph", res)
        if a.trace:
            doc.setdefault("trace_ms", {})[f"frame{bs}"] = stages = trace(lambda: ops.generator_frames(f3, kd, ks, net))
            for name, ms in sorted(stages.items(), key=lambda kv: -sum(kv[1])):
                print(f"  trace frame batch {bs} {name:28s} {len(ms):3d} calls  {sum(ms):8.3f} ms", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_reenact_frame", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
