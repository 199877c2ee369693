"""The recolor term of PTI tuning at 1024 x 1024, batch 1, with all four loss terms (L2, LPIPS, ID, face parsing), as three graph-replayed steps
(pti.GraphedPTIStep) measured in one process:

    one_target    (i)   today's step: calc_loss against the driven frame only
    two_calls     (ii)  two targets through two calc_loss compositions on today's single-target kernels (the recolor term as extra_loss):
                        every loss network runs on the reconstruction twice and on both targets in every step
    shared_cached (iii) the shared step on the multi-target heads, the target side read from a TargetCache (tune_clip's default)
    shared        (iv)  the shared step computing the target features inside the step (tune_clip(cache_targets=False))

Each reports its time per step, its kernel launches per step (one eager step under the profiler) and, for (iii), the cache's build time and bytes
per frame.  Seeded weights and inputs; prints one JSON line.

    python tools/time_pti_recolor.py"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import e4s2024_amd
from e4s2024_amd import ops_fp, ops_id, ops_lpips, pti, seeded

dev = "cuda:0"
N = 20
RL = 5.0


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


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter).parse_args()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    e4s2024_amd.install()
    from criteria.lpips.lpips import LPIPS
    from models.networks import Net3
    lp = LPIPS().to(dev).eval()
    lp.load_state_dict({k: v.to(dev) for k, v in seeded.seeded_lpips_state_dict(31).items()})
    idn = ops_id.IdNet()
    idn.load_state_dict(seeded.seeded_irse50_state_dict(41))
    idn = idn.to(dev).eval()
    fpn = ops_fp.FaceParsingNet()
    fpn.load_state_dict(seeded.seeded_unet_state_dict(43))
    fpn = fpn.to(dev).eval()
    with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
        man = json.load(f)["net3_1024_rli13"]
    net_sd = seeded.seeded_state_dict({k: torch.empty(tuple(s), dtype=getattr(torch, d), device="meta") for k, (s, d) in man.items()}, 4, "net3")
    opts = argparse.Namespace(fsencoder_type="psp", remaining_layer_idx=13, num_seg_cls=12, out_size=1024, train_G=True,
                              start_from_latent_avg=True, learn_in_w=False)
    vec = T(seeded.seeded_array(41, "vec", (1, 12, 1280), dist="normal")).to(dev)
    lab = T(seeded.blocky_labels(3, 1, 12, 512, 16)).to(dev).to(torch.uint8)
    target = torch.tanh(T(seeded.seeded_array(5, "img", (1, 3, 1024, 1024), dist="normal"))).to(dev)
    recolor = (0.8 * target + 0.1 * torch.tanh(T(seeded.seeded_array(6, "recolor", (1, 3, 1024, 1024), dist="normal"))).to(dev)).clamp(-1, 1)
    fg = pti.prepare_clip(lab)[1]
    terms = dict(lpips=lp, id_loss=idn, face_parsing=fpn)

    def recolor_term(r, _t):                        # the second calc_loss on today's kernels (the pti defaults' lambdas)
        a, b = r * fg, recolor * fg
        return RL * (F.mse_loss(a, b) + 0.8 * ops_lpips.lpips_multiscale(a, b, lp) + 0.1 * ops_id.id_loss(a, b, idn) + 0.1 * ops_fp.fp_loss(a, b, fpn))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = pti.TargetCache([target, recolor], fg, **terms)
    torch.cuda.synchronize()
    res = {"cache_build_ms_per_frame": (time.perf_counter() - t0) * 1e3, "cache_bytes_per_frame": cache.nbytes}
    t0 = time.perf_counter()                        # again, with the weights prepared and the allocator warm
    pti.TargetCache([target, recolor], fg, **terms)
    torch.cuda.synchronize()
    res["cache_rebuild_ms_per_frame"] = (time.perf_counter() - t0) * 1e3

    variants = (("one_target", {}, {}),
                ("two_calls", {"extra_loss": recolor_term}, {}),
                ("shared_cached", {"target_cache": cache, "frame": 0}, {"frame": 0}),
                ("shared", {"recolor": recolor}, {"recolor": recolor}))
    for name, kw, call_kw in variants:
        g = Net3(opts)
        g.load_state_dict(net_sd)
        g = g.to(dev).train()
        g.latent_avg = seeded.seeded_latent_avg(2, 18).to(dev)
        opt = torch.optim.Adam(pti.trainable_parameters(g), lr=1e-4, capturable=True, fused=True)
        step = pti.GraphedPTIStep(g, opt, vec, lab, target, fg, warmup=2, **terms, **kw)
        res[f"{name}_ms"] = gpu_ms(lambda: step(vec, lab, target, fg, **call_kw))
        del step
        torch.cuda.empty_cache()
        eopt = torch.optim.Adam(pti.trainable_parameters(g), lr=1e-4, fused=True)

        def eager():
            eopt.zero_grad(set_to_none=True)
            if name == "shared_cached":
                loss, _ = pti._loss_recolor(g, vec, lab, target, fg, 1.0, None, True, lp, 0.8, idn, 0.1, fpn, 0.1, None, RL, cache)
            elif name == "shared":
                loss, _ = pti._loss_recolor(g, vec, lab, target, fg, 1.0, None, True, lp, 0.8, idn, 0.1, fpn, 0.1, recolor, RL)
            else:
                loss, _ = pti._loss(g, vec, lab, target, fg, 1.0, kw.get("extra_loss"), True, lp, 0.8, idn, 0.1, fpn, 0.1)
            loss.backward()
            eopt.step()
        res[f"{name}_launches"] = launches(eager)
        del g, opt, eopt
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
