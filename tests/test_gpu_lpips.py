"""LPIPS-AlexNet on the HIP kernels (e4s2024_amd/ops_lpips.py, csrc/lpips.hip): loss and input gradient against the float64 restatement of
tests/lpips_model.py and the fixture g14 (made from the reference's own criteria/lpips classes), determinism, and the LPIPS term of the PTI and
W-optimisation steps (eager and graph-captured) against the same steps with a plain-PyTorch LPIPS as ``extra_loss``."""
import numpy as np
import pytest
import torch

import lpips_model as M
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import ops_lpips, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def g14():
    return load_golden("g14_lpips")


def _images(g14, side, bs=1):
    return M.images(int(g14["seed"]), side, bs)


@pytest.fixture(scope="module")
def sd():
    return seeded.seeded_lpips_state_dict(int(load_golden("g14_lpips")["seed"]))


@pytest.fixture(scope="module")
def sd_dev(sd):
    return {k: v.to(DEV) for k, v in sd.items()}


def _module(sd):
    install_dropin()
    from criteria.lpips.lpips import LPIPS
    m = LPIPS(net_type="alex").to(DEV).eval()
    m.load_state_dict(sd)
    return m


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return ((a - b).norm() / b.norm()).item()


def cosine(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm())).item()


def _gpu_loss_grad(x, y, weights, factor=1, scales=None):
    xg = x.to(DEV).requires_grad_(True)
    yg = y.to(DEV)
    loss = ops_lpips.lpips_multiscale(xg, yg, weights, scales) if scales else ops_lpips.lpips(xg, yg, weights, factor)
    (g,) = torch.autograd.grad(loss, xg)
    return loss.detach(), g


@pytest.mark.parametrize("side,factor", [(64, 1), (64, 2), (128, 1), (128, 2), (128, 4)])
def test_lpips_scale_matches_float64(g14, sd_dev, side, factor):
    x, y = _images(g14, side)
    loss, g = _gpu_loss_grad(x, y, sd_dev, factor)
    want_l, want_g = float(g14[f"loss{side}_f{factor}"]), T(g14[f"grad{side}_f{factor}"])
    rl = abs(loss.item() - want_l) / abs(want_l)
    rg, cs = rel_l2(g, want_g), cosine(g, want_g)
    record_parity(f"lpips{side}_f{factor}.loss_rel", rl, 1e-5)
    record_parity(f"lpips{side}_f{factor}.grad_rel_l2", rg, 1e-3)
    assert rl <= 1e-5, (loss.item(), want_l)
    assert rg <= 1e-3 and cs >= 0.99999, (rg, cs)


def test_lpips_three_scales_1024_batch2(g14, sd, sd_dev):
    x, y = _images(g14, 1024, 2)
    loss, g = _gpu_loss_grad(x, y, sd_dev, scales=3)
    rl = abs(loss.item() - float(g14["loss1024"])) / abs(float(g14["loss1024"]))
    idx = T(g14["grad1024_idx"]).long()
    samp = g.detach().cpu().double().flatten()[idx]
    assert abs(g.double().norm().item() - float(g14["grad1024_norm"])) / float(g14["grad1024_norm"]) <= 1e-3
    assert rel_l2(samp, T(g14["grad1024_samples"])) <= 1e-3
    want_l, want_g = M.loss_and_grad(x, y, sd, scales=3)                  # the whole gradient, float64 on the CPU
    rg, cs = rel_l2(g, want_g), cosine(g, want_g)
    record_parity("lpips1024x3.loss_rel", rl, 1e-5)
    record_parity("lpips1024x3.grad_rel_l2", rg, 1e-3)
    assert rl <= 1e-5 and abs(want_l.item() - float(g14["loss1024"])) <= 1e-9
    assert rg <= 1e-3 and cs >= 0.99999, (rg, cs)


def test_lpips_identical_images_give_exact_zero(g14, sd_dev):
    x = _images(g14, 128)[0]
    loss, g = _gpu_loss_grad(x, x.clone(), sd_dev, scales=3)
    assert loss.item() == 0.0
    assert torch.count_nonzero(g).item() == 0


def test_lpips_batch_is_mean_of_singles_and_bit_identical(sd_dev):
    x = torch.tanh(T(seeded.seeded_array(61, "x", (3, 3, 128, 128), dist="normal")))
    y = torch.tanh(T(seeded.seeded_array(62, "y", (3, 3, 128, 128), dist="normal")))
    loss, g = _gpu_loss_grad(x, y, sd_dev, scales=3)
    loss2, g2 = _gpu_loss_grad(x, y, sd_dev, scales=3)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)
    singles = [_gpu_loss_grad(x[i:i + 1], y[i:i + 1], sd_dev, scales=3) for i in range(3)]
    mean = sum(s[0].item() for s in singles) / 3
    assert abs(loss.item() - mean) <= 1e-6 * abs(mean)
    for i, (_, gi) in enumerate(singles):              # the batch mean: d loss / d x_i = (d single_i / d x_i) / 3
        assert rel_l2(g[i:i + 1] * 3, gi) <= 1e-5


def test_lpips_gradient_for_both_images(g14, sd, sd_dev):
    x0, y0 = _images(g14, 128)
    x, y = x0.to(DEV).requires_grad_(True), y0.to(DEV).requires_grad_(True)
    loss = ops_lpips.lpips(x, y, sd_dev)
    gx, gy = torch.autograd.grad(loss, (x, y))
    assert rel_l2(gx, T(g14["grad128_f1"])) <= 1e-3
    _, want_gy = M.loss_and_grad(y0, x0, sd)           # symmetric in (x, y)
    assert rel_l2(gy, want_gy) <= 1e-3


def test_dropin_lpips_module(g14, sd):
    m = _module(sd)
    x0, y0 = _images(g14, 128)
    x, y = x0.to(DEV), y0.to(DEV)
    assert abs(m(x, y).item() - float(g14["loss128_f1"])) <= 1e-5 * abs(float(g14["loss128_f1"]))
    taps = m.net(x)
    want = [M.normalize(t) for t in M.taps(x0.double(), M.double_sd(sd))]
    for t, w in zip(taps, want):
        assert rel_l2(t, w) <= 1e-5


# ------------------------------------------------------------------------------------------------ the PTI / W-optimisation term
def _pti_setup(net3_sd):
    from conftest import default_opts
    install_dropin()
    from models.networks import Net3
    net = Net3(default_opts(train_G=True))
    net.load_state_dict(net3_sd)
    net = net.to(DEV).train()
    net.latent_avg = seeded.seeded_latent_avg(2, 18).to(DEV)
    vec = T(seeded.seeded_array(41, "vec", (1, 12, 1280), dist="normal")).to(DEV)
    lab = T(seeded.blocky_labels(3, 1, 12, 512, 16)).to(DEV).to(torch.uint8)
    target = torch.tanh(T(seeded.seeded_array(5, "img", (1, 3, 1024, 1024), dist="normal"))).to(DEV)
    fg = torch.ones((1, 1, 1024, 1024), device=DEV)
    fg[..., :320, :] = 0
    fg[..., :, 900:] = 0
    return net, vec, lab, target, fg


def _grads(params):
    return [p.grad.detach().clone() if p.grad is not None else None for p in params]


def test_pti_step_lpips_term_matches_plain_pytorch(net3_sd, sd, sd_dev):
    from e4s2024_amd import pti
    net, vec, lab, target, fg = _pti_setup(net3_sd)
    m = _module(sd)
    params = pti.trainable_parameters(net)
    opt = torch.optim.SGD(params, lr=0.0)
    torch.manual_seed(7)
    loss_a, _ = pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, lpips=m)
    ga = _grads(params)
    torch.manual_seed(7)
    loss_b, _ = pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg,
                             extra_loss=lambda r, t: 0.8 * M.multiscale(r, t, sd_dev, 3, mask=fg))
    gb = _grads(params)
    assert abs(loss_a.item() - loss_b.item()) <= 1e-4 * abs(loss_b.item())
    torch.manual_seed(7)
    loss_c, _ = pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg)
    gc = _grads(params)
    assert loss_a.item() > loss_c.item()                # the term is there
    worst, moved = 0.0, 0
    for a, b, c in zip(ga, gb, gc):
        assert (a is None) == (b is None)
        if a is None or b.norm() == 0:
            continue
        worst = max(worst, rel_l2(a, b))
        moved += int(rel_l2(c, b) > 1e-3)
    record_parity("pti1024_lpips.grad_worst_rel_l2", worst, 1e-3)
    assert worst <= 1e-3, worst
    assert moved > 0, "the LPIPS term should change the parameter gradients"


def test_style_vector_step_lpips_term_matches_plain_pytorch(net3_sd, sd, sd_dev):
    from e4s2024_amd import pti
    net, vec, lab, target, _ = _pti_setup(net3_sd)
    for p in net.parameters():
        p.requires_grad_(False)
    m = _module(sd)
    latent = vec.clone().requires_grad_(True)
    opt = torch.optim.SGD([latent], lr=0.0)
    pti.style_vector_step(net, opt, latent, lab, target, lpips=m, randomize_noise=False)
    ga = latent.grad.detach().clone()
    pti.style_vector_step(net, opt, latent, lab, target, randomize_noise=False, extra_loss=lambda r, t: 0.8 * M.multiscale(r, t, sd_dev, 3))
    gb = latent.grad.detach().clone()
    r = rel_l2(ga, gb)
    record_parity("w_optim1024_lpips.latent_grad_rel_l2", r, 1e-3)
    assert r <= 1e-3, r


def test_graphed_pti_step_with_lpips_follows_eager(net3_sd, sd):
    from e4s2024_amd import pti
    net_b, vec, lab, target, fg = _pti_setup(net3_sd)
    net_c = _pti_setup(net3_sd)[0]
    m = _module(sd)
    opt_b = torch.optim.Adam(pti.trainable_parameters(net_b), lr=1e-3, capturable=True, fused=True)
    opt_c = torch.optim.Adam(pti.trainable_parameters(net_c), lr=1e-3, capturable=True, fused=True)
    step = pti.GraphedPTIStep(net_b, opt_b, vec, lab, target, fg, randomize_noise=False, warmup=2, lpips=m)

    def eager():
        opt_c.zero_grad(set_to_none=True)
        loss, _ = pti._loss(net_c, vec, lab, target, fg, 1.0, None, False, m, 0.8)
        loss.backward()
        opt_c.step()
        return loss.item()

    for _ in range(2):
        eager()
    for _ in range(3):
        lb = step(vec, lab, target, fg)[0].item()
        lc = eager()
        assert abs(lb - lc) <= 1e-3 * abs(lc), (lb, lc)
    worst = max(rel_l2(pb, pc) for pb, pc in zip(pti.trainable_parameters(net_b), pti.trainable_parameters(net_c)) if pc.norm() > 0)
    assert worst <= 1e-3, worst
    m.load_state_dict(seeded.seeded_lpips_state_dict(5))        # new LPIPS weights after the capture: the graph would still read the old copies
    with pytest.raises(RuntimeError, match="changed after the capture"):
        step(vec, lab, target, fg)


def test_pti_step_refuses_unloaded_lpips(net3_sd):
    from e4s2024_amd import pti
    install_dropin()
    from criteria.lpips.lpips import LPIPS
    net, vec, lab, target, fg = _pti_setup(net3_sd)
    before = [p.detach().clone() for p in pti.trainable_parameters(net)[:4]]
    opt = torch.optim.Adam(pti.trainable_parameters(net), lr=1e-3, fused=True)
    with pytest.raises(RuntimeError, match="never loaded"):
        pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, lpips=LPIPS().to(DEV))
    assert all(torch.equal(a, p) for a, p in zip(before, pti.trainable_parameters(net)[:4]))


def test_pti_step_with_lpips_runs_no_library_convolution(net3_sd, sd):
    """The LPIPS term keeps the step free of library kernels (same assertion as test_gpu_backward's PTI step)."""
    from torch.profiler import profile, ProfilerActivity
    from e4s2024_amd import pti
    net, vec, lab, target, fg = _pti_setup(net3_sd)
    m = _module(sd)
    opt = torch.optim.Adam(pti.trainable_parameters(net), lr=1e-3, fused=True)
    pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, lpips=m)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, lpips=m)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad_ops = {"aten::mm", "aten::bmm", "aten::addmm", "aten::baddbmm", "aten::matmul", "aten::convolution", "aten::_convolution",
               "aten::convolution_backward", "aten::miopen_convolution", "aten::conv2d", "aten::conv_transpose2d", "aten::linear"}
    hit = [n for n in names if n in bad_ops or n.startswith("Cijk_") or "miopen" in n.lower() or "MIOpen" in n or "igemm" in n.lower()]
    assert not hit, hit
    assert any("lpips" in n for n in names), "the profile should show the LPIPS kernels"
