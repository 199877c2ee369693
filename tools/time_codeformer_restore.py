"""Row f22 measurement, one process on the GPU, device events, every shape warmed, the alternatives alternated round by round: ``ops.codeformer_restore`` at the
caller's configuration (dim_embd 512, 8 heads, 9 layers, 1024 codes, 512 x 512 faces, ``w = 0.8, adain=True``), seeded weights, against the mirror module
``ops.CodeFormer`` called as ``net(x, w=0.8, adain=True)`` on stock PyTorch, same device, same weights:

* the whole restore and the generator half alone (``ops.codeformer_generate`` on a front made beforehand against the mirror's generator loop on the same
  front) at ``[1, 3, 512, 512]`` and ``[--batch, 3, 512, 512]`` (8 by default);
* the device time of every entry point of one native generator half, each timed alone, summed per source file;
* both float32 outputs against the mirror module in float64 on the device, at batch 1.

    python tools/time_codeformer_restore.py [--batch 8] [--rounds 5] [--json out.json]

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
from time_resunet import alternate

dev = "cuda:0"
SEED, W = 21, 0.8
FILES = {"e4s_cf_sft": "codeformer_gen.hip", "e4s_cf_image_u8": "codeformer_gen.hip", "e4s_cf_": "codeformer.hip", "e4s_conv2d": "conv.hip", "e4s_esr_": "rrdb.hip"}


def mirror_generate(net, front, w):
    """The generator half of the mirror module's ``forward`` on a front made beforehand."""
    x, fuse = front["quant_feat"], {net.fuse_generator_block[s]: s for s in net.connect_list}
    for i, block in enumerate(net.generator.blocks):
        x = block(x)
        if i in fuse and w > 0:
            x = net.fuse_convs_dict[fuse[i]](front["taps"][fuse[i]], x, w)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    doc = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "cases": {}}
    print(f"CodeFormer restore (front, generator with four SFT fuse blocks) at the caller's configuration, 512 x 512, w = {W}, {doc['device']}")
    net = ops.CodeFormer().eval()
    net.load_state_dict(seeded.seeded_codeformer_state_dict(SEED), strict=True)
    net = net.to(dev)
    base = torch.from_numpy(M.case_input("CF-F")).to(dev)
    for bs in sorted({1, a.batch}):
        x = torch.cat([base.roll(17 * i, 3) for i in range(bs)]).contiguous()
        front = ops.codeformer_front(x, net)
        got, want = ops.codeformer_restore(x, net, w=W)[0], net(x, w=W, adain=True)[0]
        assert torch.equal(got, ops.codeformer_generate(front, net, w=W))
        if bs == 1:
            want64 = copy.deepcopy(net).double()(x.double(), w=W, adain=True)[0]
            print(f"  out against the mirror in float64: hip {float((got - want64).abs().max()):.2e}, torch {float((want - want64).abs().max()):.2e}; "
                  f"std {float(want64.std()):.3f}, {100 * float((want64.abs() <= 1).double().mean()):.0f} % inside [-1, 1]", flush=True)
            del want64
        res = alternate({"hip": lambda: ops.codeformer_restore(x, net, w=W), "torch": lambda: net(x, w=W, adain=True)}, a.rounds, 3)
        show(doc, f"restore batch {bs}", res)
        res = alternate({"hip": lambda: ops.codeformer_generate(front, net, w=W), "torch": lambda: mirror_generate(net, front, W)}, a.rounds, 3)
        show(doc, f"generator half batch {bs}", res)
        stages = trace(lambda: ops.codeformer_generate(front, net, w=W))
        per_file, total = {}, sum(sum(ms) for ms in stages.values())
        for name, ms in sorted(stages.items(), key=lambda kv: -sum(kv[1])):
            file = next((f for p, f in FILES.items() if name.startswith(p)), "other")
            per_file[file] = per_file.get(file, 0.0) + sum(ms)
            print(f"  trace batch {bs} {name:22s} {len(ms):4d} calls  {sum(ms):8.3f} ms", flush=True)
        doc.setdefault("trace_ms", {})[f"batch{bs}"] = {k: [len(v), sum(v)] for k, v in stages.items()}
        doc.setdefault("share", {})[f"batch{bs}"] = {f: t / total for f, t in per_file.items()}
        print(f"  generator half, kernel time by source file, batch {bs} (each entry point timed alone, {total:.3f} ms in all): "
              + ", ".join(f"{f} {t:.3f} ms = {100 * t / total:.0f} %" for f, t in sorted(per_file.items(), key=lambda kv: -kv[1])), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
    print(json.dumps({"tool": "time_codeformer_restore", "ok": True}))


if __name__ == "__main__":
    with torch.no_grad():
        main()
