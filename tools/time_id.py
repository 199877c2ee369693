"""The ArcFace identity term of the PTI loss (ops_id, csrc/idloss.hip) at batch 1, 1024 x 1024: target forward + reconstruction forward + input
gradient, against the same term as a plain-PyTorch restatement on the GPU (MIOpen / rocBLAS) in the same process; the kernel launches the term
adds; one graph-replayed PTI step (pti.GraphedPTIStep) with L2 + LPIPS, with and without the term.  Seeded weights; prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import e4s2024_amd
import id_model as M              # tests/id_model.py: the plain-PyTorch restatement
from e4s2024_amd import ops_id, pti, seeded

dev = "cuda:0"
N = 20


def gpu_ms(fn, n=N):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def term(fn_loss, x, y):
    def run():
        xg = x.detach().requires_grad_(True)
        torch.autograd.grad(fn_loss(xg, y), xg)
    return run


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-pti", action="store_true", help="the term only")
    args = ap.parse_args()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    sd = {k: v.to(dev) for k, v in seeded.seeded_irse50_state_dict(41).items()}
    net = ops_id.IdNet()
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    x, y = (t.to(dev) for t in M.images(41, 1024, 1))
    native = term(lambda a, b: ops_id.id_loss(a, b, net), x, y)
    res = {"id_term_ms": gpu_ms(native), "id_term_launches": launches(native)}
    torch.backends.cudnn.benchmark = True
    res["id_term_pytorch_ms"] = gpu_ms(term(lambda a, b: M.id_loss(a, b, sd)[0], x, y))
    if not args.no_pti:
        e4s2024_amd.install()
        from criteria.lpips.lpips import LPIPS
        from models.networks import Net3
        lp = LPIPS().to(dev).eval()
        lp.load_state_dict({k: v.to(dev) for k, v in seeded.seeded_lpips_state_dict(31).items()})
        with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
            man = json.load(f)["net3_1024_rli13"]
        net_sd = seeded.seeded_state_dict({k: torch.empty(tuple(s), dtype=getattr(torch, d), device="meta") for k, (s, d) in man.items()}, 4, "net3")
        opts = argparse.Namespace(fsencoder_type="psp", remaining_layer_idx=13, num_seg_cls=12, out_size=1024, train_G=True,
                                  start_from_latent_avg=True, learn_in_w=False)
        vec = T(seeded.seeded_array(41, "vec", (1, 12, 1280), dist="normal")).to(dev)
        lab = T(seeded.blocky_labels(3, 1, 12, 512, 16)).to(dev).to(torch.uint8)
        target = torch.tanh(T(seeded.seeded_array(5, "img", (1, 3, 1024, 1024), dist="normal"))).to(dev)
        fg = pti.prepare_clip(lab)[1]
        for name, kw in (("pti_step_lpips_ms", {"lpips": lp}), ("pti_step_lpips_id_ms", {"lpips": lp, "id_loss": net})):
            g = Net3(opts)
            g.load_state_dict(net_sd)
            g = g.to(dev).train()
            g.latent_avg = seeded.seeded_latent_avg(2, 18).to(dev)
            opt = torch.optim.Adam(pti.trainable_parameters(g), lr=1e-4, capturable=True, fused=True)
            step = pti.GraphedPTIStep(g, opt, vec, lab, target, fg, warmup=2, **kw)
            res[name] = gpu_ms(lambda: step(vec, lab, target, fg))
            del step, g, opt
            torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
