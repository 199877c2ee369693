"""The LPIPS-AlexNet term of the PTI loss (ops_lpips, csrc/lpips.hip) at batch 1, 1024 x 1024: forward + input gradient over the three scales,
one graph-replayed PTI step (pti.GraphedPTIStep) with and without the term, and the same term as a plain-PyTorch restatement on the GPU
(MIOpen convolutions) for comparison.  Seeded weights; prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import e4s2024_amd
import lpips_model as M           # tests/lpips_model.py: the plain-PyTorch restatement
from e4s2024_amd import ops_lpips, pti, seeded

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


def term_ms(fn_loss, x, y):
    def run():
        xg = x.detach().requires_grad_(True)
        torch.autograd.grad(fn_loss(xg, y), xg)
    return gpu_ms(run)


def main():
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    sd = {k: v.to(dev) for k, v in seeded.seeded_lpips_state_dict(31).items()}
    e4s2024_amd.install()
    from criteria.lpips.lpips import LPIPS
    m = LPIPS().to(dev).eval()
    m.load_state_dict(sd)
    x, y = (t.to(dev) for t in M.images(31, 1024, 1))
    res = {"lpips_term_ms": term_ms(lambda a, b: ops_lpips.lpips_multiscale(a, b, m), x, y)}
    torch.backends.cudnn.benchmark = True
    res["lpips_term_pytorch_miopen_ms"] = term_ms(lambda a, b: M.multiscale(a, b, sd, 3), x, y)

    from models.networks import Net3
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        man = json.load(f)["net3_1024_rli13"]
    net_sd = seeded.seeded_state_dict({k: torch.empty(tuple(s), dtype=getattr(torch, d), device="meta") for k, (s, d) in man.items()}, 4, "net3")
    import argparse
    opts = argparse.Namespace(fsencoder_type="psp", remaining_layer_idx=13, num_seg_cls=12, out_size=1024, train_G=True,
                              start_from_latent_avg=True, learn_in_w=False)
    vec = T(seeded.seeded_array(41, "vec", (1, 12, 1280), dist="normal")).to(dev)
    lab = T(seeded.blocky_labels(3, 1, 12, 512, 16)).to(dev).to(torch.uint8)
    target = torch.tanh(T(seeded.seeded_array(5, "img", (1, 3, 1024, 1024), dist="normal"))).to(dev)
    fg = pti.prepare_clip(lab)[1]
    for name, kw in (("pti_step_ms", {}), ("pti_step_lpips_ms", {"lpips": m})):
        net = Net3(opts)
        net.load_state_dict(net_sd)
        net = net.to(dev).train()
        net.latent_avg = seeded.seeded_latent_avg(2, 18).to(dev)
        opt = torch.optim.Adam(pti.trainable_parameters(net), lr=1e-4, capturable=True, fused=True)
        step = pti.GraphedPTIStep(net, opt, vec, lab, target, fg, warmup=2, **kw)
        res[name] = gpu_ms(lambda: step(vec, lab, target, fg))
        del step, net, opt
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
