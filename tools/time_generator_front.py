"""Row f19 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round: face-vid2vid's generator in front
of its decoder at the upstream vox-256 configuration (256 x 256 source, feature ``[bs, 32, 16, 64, 64]``, 15 keypoints, the occlusion head), seeded weights,
against the mirror module's front run by stock PyTorch on the same device with the same weights:

* the per-clip part, ``ops.appearance_feature`` against ``OcclusionAwareSPADEGenerator.source_feature``;
* the per-frame part, ``ops.generator_warp`` on the held feature at batch 1 and batch ``--batch``, eager and replayed from a captured graph, against the
  mirror's ``warp`` and against its whole ``front``, which is what one call of the reference's generator recomputes per driving frame;
* ``ops.deform_feature`` alone, batch 1 and ``--batch`` against one shared feature, with the bytes it reads and writes per second, against ``F.grid_sample``;
* with ``--trace``, the device time of every kernel of the two native passes, one after the other.

    python tools/time_generator_front.py [--batch 4] [--rounds 5] [--trace] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import torch.nn.functional as F

from e4s2024_amd import ops, seeded
from e4s2024_amd import ops_reenact as R
from time_reenact import show
from time_resunet import alternate, graphed, timed

dev = "cuda:0"
SEED = 19


def macs(structure, H, W):
    """(per-clip, per-frame without the dense-motion network) multiply-adds of one sample, from the layer shapes."""
    cin, k, bexp, down, maxf, rc, depth, nres, outf, _ = structure
    clip = k * k * cin * bexp * H * W
    h, w, c = H, W, bexp
    for d in down:
        clip += 9 * c * d * h * w
        h, w, c = h // 2, w // 2, d
    clip += c * maxf * h * w + nres * 2 * 27 * rc * rc * depth * h * w
    return clip, (9 * maxf * outf + outf * outf) * h * w


def trace(fn):
    """The device time of every entry point ``fn`` goes through, each timed alone."""
    stages = {}
    orig = R.lib().call

    def call(name, *args):
        stages.setdefault(name, []).append(timed(lambda: orig(name, *args), 3))
        return orig(name, *args)

    R.lib().call = call
    try:
        fn()
    finally:
        del R.lib().call
    return stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"face-vid2vid generator front at the upstream configuration, source 256 x 256, feature [bs, 32, 16, 64, 64], {doc['device']}")
    net = ops.OcclusionAwareSPADEGenerator().eval()
    net.decoder = torch.nn.Identity()                # stage 4; the front reads none of its keys
    template = {k: torch.empty(s, dtype=torch.long if k.endswith("num_batches_tracked") else torch.float32, device="meta")
                for k, s in ops.generator_front_structure_shapes(net.structure).items()}
    net.load_state_dict(seeded.seeded_generator_state_dict(template, SEED), strict=True)
    net = net.to(dev)
    K = net.structure[9][0]
    clip, frame = macs(net.structure, 256, 256)
    print(f"  per sample: the per-clip part {clip / 1e9:.1f} GMAC, third and fourth {frame / 1e9:.1f} GMAC", flush=True)

    source = torch.from_numpy(seeded.seeded_array(SEED, "source", (1, 3, 256, 256), 0.5, 0.25)).clamp_(0, 1).to(dev)
    f3 = ops.appearance_feature(source, net)
    off = float((f3 - net.source_feature(source)).abs().max())
    print(f"  appearance_feature against the mirror on stock PyTorch: {off:.2e} (max |feature| {float(f3.abs().max()):.2f})", flush=True)
    res = alternate({"hip": lambda: ops.appearance_feature(source, net), "torch": lambda: net.source_feature(source)}, a.rounds, 3)
    show(doc, "per clip: appearance_feature", res, f"   ({2 * clip / 1e9:.0f} GFLOP counted)")

    for bs in sorted({1, a.batch}):
        ks = torch.from_numpy(seeded.seeded_array(SEED, f"kp_s{bs}", (1, K, 3), 0.0, 0.3)).to(dev).expand(bs, -1, -1).contiguous()
        kd = (ks + torch.from_numpy(seeded.seeded_array(SEED, f"kp_d{bs}", (bs, K, 3), 0.0, 0.15)).to(dev)).contiguous()
        kd, ks = {"value": kd}, {"value": ks}
        got, want = ops.generator_warp(f3, kd, ks, net), net.warp(f3, kd, ks)
        print(f"  generator_warp batch {bs} against the mirror on stock PyTorch: " + ", ".join(f"{k} {float((got[k] - want[k]).abs().max()):.2e}" for k in got),
              flush=True)
        res = alternate({"hip": lambda: ops.generator_warp(f3, kd, ks, net), "torch": lambda: net.warp(f3, kd, ks),
                         "torch_front": lambda: net.front(source.expand(bs, -1, -1, -1), kd, ks)}, a.rounds, 3)
        show(doc, f"per frame: generator_warp batch {bs} (torch_front: the source part recomputed, as the reference does per frame)", res)
        res = alternate({"eager": lambda: ops.generator_warp(f3, kd, ks, net), "graph": graphed(lambda: ops.generator_warp(f3, kd, ks, net)),
                         "torch_graph": graphed(lambda: net.warp(f3, kd, ks))}, a.rounds, 3)
        show(doc, f"per frame: generator_warp batch {bs} replayed", res)
        grid = got["deformation"]
        n = f3[0].numel()
        moved = 4 * (n + bs * (n + 3 * grid[0].numel() // 3))                 # the shared volume once, per frame the grid and the output
        res = alternate({"hip": lambda: ops.deform_feature(f3, grid), "torch": lambda: F.grid_sample(f3.expand(bs, -1, -1, -1, -1), grid, align_corners=False)},
                        a.rounds, 5)
        show(doc, f"deform_feature batch {bs}", res)
        for k in ("hip", "torch"):
            med = sorted(res[k])[len(res[k]) // 2]
            print(f"  deform_feature batch {bs} {k:6s}: {moved / 1e6:.1f} MB read and written in the median round: {moved / 1e6 / med:.0f} GB/s", flush=True)
        if a.trace:
            doc.setdefault("trace_ms", {})[f"warp{bs}"] = stages = trace(lambda: ops.generator_warp(f3, kd, ks, net))
            for name, ms in stages.items():
                print(f"  trace warp batch {bs} {name:28s} {len(ms):2d} calls  {sum(ms):8.3f} ms", flush=True)
    if a.trace:
        doc["trace_ms"]["clip"] = stages = trace(lambda: ops.appearance_feature(source, net))
        for name, ms in stages.items():
            print(f"  trace per clip     {name:28s} {len(ms):2d} calls  {sum(ms):8.3f} ms", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_generator_front", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
