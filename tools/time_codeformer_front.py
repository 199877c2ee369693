"""Row f21 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round: ``ops.codeformer_front`` at the
caller's configuration (dim_embd 512, 8 heads, 9 layers, 1024 codes, 512 x 512 faces), seeded weights, against the mirror module ``ops.CodeFormer.front`` on
stock PyTorch, same device, same weights:

* at ``[1, 3, 512, 512]`` and ``[--batch, 3, 512, 512]`` (8 by default), eager and replayed from a captured graph;
* the device time of every entry point of one native front, each timed alone, summed per source file: the share of csrc/codeformer.hip against csrc/conv.hip
  (conv_in and the logits head, on the exact kernel, count with conv.hip);
* both float32 paths against the mirror module in float64 on the device, and the codes that differ.

    python tools/time_codeformer_front.py [--batch 8] [--rounds 5] [--json out.json]

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

import codeformer_model as M
from e4s2024_amd import ops, seeded
from time_generator_front import trace
from time_reenact import show
from time_resunet import alternate, graphed

dev = "cuda:0"
SEED = 21
FILES = {"e4s_cf_": "codeformer.hip", "e4s_conv2d": "conv.hip"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"CodeFormer front (encoder, transformer, codes, codebook, AdaIN) at the caller's configuration, 512 x 512, {doc['device']}")
    net = ops.CodeFormer().eval()
    net.load_state_dict(seeded.seeded_codeformer_state_dict(SEED), strict=True)
    net = net.to(dev)
    net64 = copy.deepcopy(net).double()
    base = torch.from_numpy(M.case_input("CF-F")).to(dev)
    for bs in sorted({1, a.batch}):
        x = torch.cat([base.roll(17 * i, 3) for i in range(bs)]).contiguous()
        got, want = ops.codeformer_front(x, net), net.front(x)
        if bs == 1:
            want64 = net64.front(x.double())
            for k in ("lq_feat", "logits", "quant_feat"):
                print(f"  {k} against the mirror in float64: hip {float((got[k] - want64[k]).abs().max()):.2e}, torch {float((want[k] - want64[k]).abs().max()):.2e}")
            print(f"  codes that differ from the float64 mirror's: hip {int((got['idx'] != want64['idx']).sum())}, torch {int((want['idx'] != want64['idx']).sum())} "
                  f"of {got['idx'].numel()}; {len(got['idx'].unique())} distinct", flush=True)
            del want64
        res = alternate({"hip": lambda: ops.codeformer_front(x, net), "torch": lambda: net.front(x)}, a.rounds, 3)
        show(doc, f"front batch {bs}", res)
        res = alternate({"hip": graphed(lambda: ops.codeformer_front(x, net)), "torch": graphed(lambda: net.front(x))}, a.rounds, 3)
        show(doc, f"front batch {bs} replayed from a graph", res)
        stages = trace(lambda: ops.codeformer_front(x, net))
        per_file, total = {}, sum(sum(ms) for ms in stages.values())
        for name, ms in sorted(stages.items(), key=lambda kv: -sum(kv[1])):
            file = next((f for p, f in FILES.items() if name.startswith(p)), "other")
            per_file[file] = per_file.get(file, 0.0) + sum(ms)
            print(f"  trace batch {bs} {name:22s} {len(ms):4d} calls  {sum(ms):8.3f} ms", flush=True)
        doc.setdefault("trace_ms", {})[f"batch{bs}"] = {k: [len(v), sum(v)] for k, v in stages.items()}
        doc.setdefault("share", {})[f"batch{bs}"] = {f: t / total for f, t in per_file.items()}
        print(f"  kernel time by source file, batch {bs} (each entry point timed alone, {total:.3f} ms in all): "
              + ", ".join(f"{f} {t:.3f} ms = {100 * t / total:.0f} %" for f, t in sorted(per_file.items(), key=lambda kv: -kv[1])), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_codeformer_front", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
