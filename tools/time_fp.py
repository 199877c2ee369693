"""The face-parsing term of the PTI loss (ops_fp, csrc/fploss.hip) at batch 1, 1024 x 1024: target forward + reconstruction forward + input gradient,
against the same term as a plain-PyTorch restatement on the GPU (MIOpen) in the same process; the kernel launches the term adds; one
graph-replayed PTI step (pti.GraphedPTIStep) with L2 + LPIPS + ID, with and without the term.  Seeded weights; prints one JSON line.

    python tools/time_fp.py [--no-pti] [--breakdown OUT_DIR]

``--breakdown OUT_DIR``: afterwards, run the native term alone in a child process under ``rocprofv3 --kernel-trace --stats`` (results under
OUT_DIR) and add its per-kernel times per step to the JSON line (``breakdown``: name -> [calls per step, us per step])."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import e4s2024_amd
import fp_model as M              # tests/fp_model.py: the plain-PyTorch restatement
from e4s2024_amd import ops_fp, ops_id, pti, seeded

dev = "cuda:0"
N = 20
PROF_STEPS = 10


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


def _native(net):
    x, y = (t.to(dev) for t in M.images(43, 1024, 1))
    return term(lambda a, b: ops_fp.fp_loss(a, b, net), x, y), x, y


def _load_net():
    net = ops_fp.FaceParsingNet()
    net.load_state_dict({k: v.to(dev) for k, v in seeded.seeded_unet_state_dict(43).items()})
    return net.to(dev).eval()


def _short(name: str) -> str:
    """A kernel's name without its namespace and argument list."""
    if name.endswith(")") and "(" in name:
        name = name[:name.rfind("(")]
    return name.replace("(anonymous namespace)::", "")[:90]


def breakdown(out_dir):
    """Per-kernel time of the native term from a child process under rocprofv3: {name: [calls per step, us per step]}."""
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out_dir, "-o", "fp", "--", sys.executable, os.path.abspath(__file__), "--profiled-child"]
    with open(os.path.join(out_dir, "child.log"), "w") as log:
        rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=600).returncode
    if rc != 0:
        raise RuntimeError(f"rocprofv3 child failed with status {rc} (see {out_dir}/child.log)")
    dbs = sorted(glob.glob(os.path.join(out_dir, "**", "*_results.db"), recursive=True))
    if not dbs:
        raise RuntimeError(f"no rocprofv3 result database under {out_dir}")
    rows = [(_short(n), s, e) for n, s, e in sqlite3.connect(dbs[-1]).execute("select name, start, end from kernels order by start").fetchall()]
    # the child runs 3 warm-up steps (the first also prepares the weights), then PROF_STEPS timed ones; every step starts with the pooling of
    # y_hat and of y (two id_resample launches): keep the dispatches from the start of the first timed step on
    starts = [i for i, r in enumerate(rows) if r[0] == "id_resample_kernel"]
    rows = rows[starts[-2 * PROF_STEPS]:]
    agg = {}
    for name, s, e in rows:
        a = agg.setdefault(name, [0, 0.0])
        a[0] += 1
        a[1] += (e - s) / 1e3
    return {k: [v[0] // PROF_STEPS, round(v[1] / PROF_STEPS, 2)] for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-pti", action="store_true", help="the term only")
    ap.add_argument("--breakdown", metavar="OUT_DIR", help="per-kernel times of the term from a rocprofv3 child run")
    ap.add_argument("--profiled-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    net = _load_net()
    native, x, y = _native(net)
    if args.profiled_child:
        gpu_ms(native, PROF_STEPS)
        return
    res = {"fp_term_ms": gpu_ms(native), "fp_term_launches": launches(native)}
    sd = {k: v.to(dev) for k, v in seeded.seeded_unet_state_dict(43).items()}
    torch.backends.cudnn.benchmark = True
    res["fp_term_pytorch_ms"] = gpu_ms(term(lambda a, b: M.fp_loss(a, b, sd)[0], x, y))
    if not args.no_pti:
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        e4s2024_amd.install()
        from criteria.lpips.lpips import LPIPS
        from models.networks import Net3
        lp = LPIPS().to(dev).eval()
        lp.load_state_dict({k: v.to(dev) for k, v in seeded.seeded_lpips_state_dict(31).items()})
        idn = ops_id.IdNet()
        idn.load_state_dict({k: v.to(dev) for k, v in seeded.seeded_irse50_state_dict(41).items()})
        idn = idn.to(dev).eval()
        with open(os.path.join(ROOT, "tests", "golden", "manifest.json")) as f:
            man = json.load(f)["net3_1024_rli13"]
        net_sd = seeded.seeded_state_dict({k: torch.empty(tuple(s), dtype=getattr(torch, d), device="meta") for k, (s, d) in man.items()}, 4, "net3")
        opts = argparse.Namespace(fsencoder_type="psp", remaining_layer_idx=13, num_seg_cls=12, out_size=1024, train_G=True,
                                  start_from_latent_avg=True, learn_in_w=False)
        vec = T(seeded.seeded_array(41, "vec", (1, 12, 1280), dist="normal")).to(dev)
        lab = T(seeded.blocky_labels(3, 1, 12, 512, 16)).to(dev).to(torch.uint8)
        target = torch.tanh(T(seeded.seeded_array(5, "img", (1, 3, 1024, 1024), dist="normal"))).to(dev)
        fg = pti.prepare_clip(lab)[1]
        for name, kw in (("pti_step_lpips_id_ms", {"lpips": lp, "id_loss": idn}),
                         ("pti_step_lpips_id_fp_ms", {"lpips": lp, "id_loss": idn, "face_parsing": net})):
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
    if args.breakdown:
        res["breakdown"] = breakdown(args.breakdown)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
