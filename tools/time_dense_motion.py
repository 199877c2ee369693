"""Row f18 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round: face-vid2vid's dense-motion
network at the upstream vox-256 configuration (15 keypoints, feature ``[bs, 32, 16, 64, 64]``, the occlusion head), seeded weights, against the mirror module
run by stock PyTorch on the same device with the same weights:

* ``ops.dense_motion_forward`` at batch 1 and batch ``--batch``, eager and replayed from a captured graph;
* the ``mask`` head alone (``ops.conv3d_k7`` on the hourglass output against ``nn.Conv3d``);
* with ``--trace``, the device time of every stage of the native pass, one after the other.

    python tools/time_dense_motion.py [--batch 4] [--rounds 5] [--trace] [--json out.json]

Each figure is the median over the rounds with the min .. max of the rounds beside it: the spread a difference has to exceed.  The multiply-adds of the
hourglass and of the two 7-tap heads are counted from the layer shapes and printed with the rate they give."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from e4s2024_amd import ops, seeded
from e4s2024_amd import ops_reenact as R
from time_reenact import show
from time_resunet import alternate, graphed, timed

dev = "cuda:0"
SEED = 18


def macs(structure, D, H, W):
    """(hourglass, mask head, occlusion head) multiply-adds of one sample, from the layer shapes."""
    K, _, _, down, up, occ = structure
    infe, outf, levels = R._dm_widths(structure)
    nb = len(down)
    hg = sum(27 * levels[i] * levels[i + 1] * D * (H >> i) * (W >> i) for i in range(nb))
    for j in range(nb):
        cin = levels[nb] if j == 0 else up[j - 1] + levels[nb - j]
        hg += 27 * cin * up[j] * D * (H >> (nb - 1 - j)) * (W >> (nb - 1 - j))
    hg += 27 * outf * outf * D * H * W
    return hg, 343 * outf * (K + 1) * D * H * W, 49 * outf * occ * H * W if occ else 0


def inputs(bs, structure, D, H, W):
    K, C = structure[0], structure[1]
    x = torch.from_numpy(seeded.seeded_array(SEED, f"feature{bs}", (bs, C, D, H, W), 0.0, 1.0, "normal")).to(dev)
    ks = torch.from_numpy(seeded.seeded_array(SEED, f"kp_s{bs}", (bs, K, 3), 0.0, 0.35)).to(dev)
    kd = ks + torch.from_numpy(seeded.seeded_array(SEED, f"kp_d{bs}", (bs, K, 3), 0.0, 0.2)).to(dev)
    return x, {"value": kd.contiguous()}, {"value": ks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"face-vid2vid dense motion at the upstream configuration, feature [bs, 32, 16, 64, 64], {doc['device']}")
    net = ops.DenseMotionNetwork().eval()
    with torch.device("meta"):
        template = ops.DenseMotionNetwork().state_dict()
    net.load_state_dict(seeded.seeded_dense_motion_state_dict(template, SEED), strict=True)
    net = net.to(dev)
    D, H, W = 16, 64, 64
    hg, mk, oc = macs(net.structure, D, H, W)
    print(f"  per sample: hourglass {hg / 1e9:.1f} GMAC, mask head {mk / 1e9:.1f} GMAC, occlusion head {oc / 1e9:.2f} GMAC", flush=True)

    for bs in sorted({1, a.batch}):
        x, kd, ks = inputs(bs, net.structure, D, H, W)
        got, want = ops.dense_motion_forward(x, kd, ks, net), net(x, kd, ks)
        off = {k: float((got[k] - want[k]).abs().max()) for k in got}
        print(f"  dense_motion_forward batch {bs} against the mirror on stock PyTorch: " + ", ".join(f"{k} {v:.2e}" for k, v in off.items()), flush=True)
        res = alternate({"hip": lambda: ops.dense_motion_forward(x, kd, ks, net), "torch": lambda: net(x, kd, ks)}, a.rounds, 3)
        show(doc, f"DenseMotionNetwork batch {bs}", res, f"   ({2 * bs * (hg + mk + oc) / 1e9:.0f} GFLOP counted)")
        res = alternate({"eager": lambda: ops.dense_motion_forward(x, kd, ks, net), "graph": graphed(lambda: ops.dense_motion_forward(x, kd, ks, net)),
                         "torch_graph": graphed(lambda: net(x, kd, ks))}, a.rounds, 3)
        show(doc, f"DenseMotionNetwork batch {bs} replayed", res)

    # the mask head alone, on an input of the hourglass output's shape
    outf = net.hourglass.out_filters
    pred = torch.relu(torch.from_numpy(seeded.seeded_array(SEED, "prediction", (1, outf, D, H, W), 0.0, 1.0, "normal")).to(dev))
    slabs, bias = R.prep_conv3d_k7(net.mask.weight), net.mask.bias
    off = float((ops.conv3d_k7(pred, slabs, bias) - net.mask(pred)).abs().max())
    print(f"  conv3d_k7 against nn.Conv3d on the mask head: {off:.2e}", flush=True)
    res = alternate({"hip": lambda: ops.conv3d_k7(pred, slabs, bias), "torch": lambda: net.mask(pred)}, a.rounds, 3)
    show(doc, "mask head batch 1", res, f"   ({2 * mk / 1e9:.0f} GFLOP)")

    if a.trace:                                 # every stage of the native pass timed alone, by wrapping the entry points the forward goes through
        x, kd, ks = inputs(1, net.structure, D, H, W)
        stages = {}
        orig = R.lib().call

        def call(name, *args):
            stages.setdefault(name, []).append(timed(lambda: orig(name, *args), 3))
            return orig(name, *args)

        R.lib().call = call
        try:
            ops.dense_motion_forward(x, kd, ks, net)
        finally:
            del R.lib().call
        doc["trace_ms"] = stages
        for name, ms in stages.items():
            print(f"  trace {name:32s} {len(ms):2d} calls  {sum(ms):8.3f} ms   " + " ".join(f"{v:.3f}" for v in ms), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_dense_motion", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
