"""ArcFace identity loss on the HIP kernels (e4s2024_amd/ops_id.py, csrc/idloss.hip): loss and input gradient against the fixture g15 (made from
the reference's own criteria/id_loss.py) and the float64 restatement of tests/id_model.py, the near-converged cancellation case, determinism,
edge-case weights, the drop-in IDLoss, and the identity term of the PTI and W-optimisation steps (eager and graph-captured) against the same
steps with a plain-PyTorch identity loss as ``extra_loss``."""
import os
import types

import numpy as np
import pytest
import torch

import id_model as M
from conftest import install_dropin, load_golden, record_parity
from e4s2024_amd import ops_id, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_id")


@pytest.fixture(scope="module")
def sd(g15):
    return seeded.seeded_irse50_state_dict(int(g15["seed"]))


@pytest.fixture(scope="module")
def net(sd):
    m = ops_id.IdNet()
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return ((a - b).norm() / b.norm()).item()


def _gpu(x, y, weights, ms=True):
    xg = x.to(DEV).requires_grad_(True)
    loss, sim, per = ops_id.id_loss_terms(xg, y.to(DEV), weights, ms)
    (g,) = torch.autograd.grad(loss, xg)
    return loss.detach(), sim, per, g


@pytest.mark.parametrize("side", [112, 256, 1024])
@pytest.mark.parametrize("ms", [True, False])
def test_id_loss_matches_fixture(g15, net, side, ms):
    tag = "ms" if ms else "ss"
    x, y = M.images(int(g15["seed"]), side, 2)
    loss, sim, per, g = _gpu(x, y, net, ms)
    el = abs(loss.item() - float(g15[f"loss{side}_{tag}"]))
    es = abs(sim.item() - float(g15[f"sim{side}_{tag}"]))
    samp = g.detach().cpu().double().flatten()[T(g15[f"grad{side}_{tag}_idx"]).long()]
    rg = rel_l2(samp, T(g15[f"grad{side}_{tag}_samples"]))
    rn = abs(g.double().norm().item() - float(g15[f"grad{side}_{tag}_norm"])) / float(g15[f"grad{side}_{tag}_norm"])
    if side == 112 and ms:
        rg = max(rg, rel_l2(g, T(g15["grad112_ms"])))
    if ms:
        assert (per.cpu().double() - T(g15[f"per{side}"])).abs().max().item() <= 1e-5
    record_parity(f"id{side}_{tag}.loss_abs", el, 1e-5)
    record_parity(f"id{side}_{tag}.grad_rel_l2", rg, 1e-3)
    assert el <= 1e-5 and es <= 1e-5, (loss.item(), sim.item())
    assert rg <= 1e-3 and rn <= 1e-3, (rg, rn)


def test_id_loss_batch1_and_batch_mean(g15, sd, net):
    x, y = M.images(int(g15["seed"]), 256, 2)
    loss, _, _, g = _gpu(x, y, net)
    singles = [_gpu(x[i:i + 1], y[i:i + 1], net) for i in range(2)]
    wl, _, _, wg = M.loss_and_grad(x[:1], y[:1], sd)
    assert abs(singles[0][0].item() - wl.item()) <= 1e-5 and rel_l2(singles[0][3], wg) <= 1e-3
    assert abs(loss.item() - (singles[0][0].item() + singles[1][0].item()) / 2) <= 1e-6
    for i, s in enumerate(singles):
        assert rel_l2(g[i:i + 1] * 2, s[3]) <= 1e-4


def test_id_loss_near_converged_gradient(g15, sd, net):
    """y_hat = y + 0.01 noise: the gradient is a difference of nearly equal unit vectors, so forward error is amplified."""
    _, y = M.images(int(g15["seed"]), 256, 2)
    x = y + 0.01 * T(seeded.seeded_array(3, "id_noise", tuple(y.shape), dist="normal"))
    loss, _, _, g = _gpu(x, y, net)
    wl, _, _, wg = M.loss_and_grad(x, y, sd)
    rg = rel_l2(g, wg)
    record_parity("id256_near_converged.grad_rel_l2", rg, 5e-3)
    assert abs(loss.item() - wl.item()) <= 1e-6
    assert rg <= 5e-3, rg


def test_id_loss_identical_images_and_bit_identical_reruns(g15, net):
    x, y = M.images(int(g15["seed"]), 256, 2)
    loss, _, per, _ = _gpu(y, y.clone(), net)
    assert per.abs().max().item() <= 1e-6 and abs(loss.item()) <= 5e-6
    a = _gpu(x, y, net)
    b = _gpu(x, y, net)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])


def test_id_loss_edge_case_weights(g15, sd):
    """Negative and zero PReLU slopes and a zero BatchNorm gamma on a residual branch's input."""
    e = {k: v.clone() for k, v in sd.items()}
    e["input_layer.2.weight"][:8] = -0.2
    e["body.0.res_layer.2.weight"][:16] = 0.0
    e["body.5.res_layer.2.weight"][::3] = -0.1
    e["body.4.res_layer.0.weight"][7] = 0.0
    e["body.9.res_layer.0.weight"][:] = 0.0
    m = ops_id.IdNet()
    m.load_state_dict(e)
    m = m.to(DEV).eval()
    x, y = M.images(int(g15["seed"]), 112, 2)
    loss, _, _, g = _gpu(x, y, m)
    wl, _, _, wg = M.loss_and_grad(x, y, e)
    rg = rel_l2(g, wg)
    record_parity("id112_edge_weights.grad_rel_l2", rg, 1e-3)
    assert abs(loss.item() - wl.item()) <= 1e-5 and rg <= 1e-3, (loss.item(), wl.item(), rg)


def _dropin(sd, tmp_path, ms=True):
    install_dropin()
    from criteria.id_loss import IDLoss
    path = os.path.join(tmp_path, "ir_se50.pth")
    torch.save(sd, path)
    return IDLoss(types.SimpleNamespace(ir_se50_path=path, id_loss_multiscale=ms)).to(DEV).eval()


def test_dropin_idloss(g15, sd, tmp_path):
    x, y = M.images(int(g15["seed"]), 1024, 2)
    for ms, tag in ((True, "ms"), (False, "ss")):
        m = _dropin(sd, tmp_path, ms)
        loss, sim, logs = m(x.to(DEV), y.to(DEV))
        assert logs is None and isinstance(sim, float)
        assert abs(loss.item() - float(g15[f"loss1024_{tag}"])) <= 1e-5 and abs(sim - float(g15[f"sim1024_{tag}"])) <= 1e-5
    feats = m.extract_feats(x.to(DEV))
    want = M.backbone(M.preprocess(x.double()), M.double_sd(sd), False)
    assert len(feats) == 1 and rel_l2(feats[0], want[0]) <= 1e-5


def test_refuses_unloaded_and_training_mode(g15, net):
    x, y = M.images(int(g15["seed"]), 112, 1)
    with pytest.raises(RuntimeError, match="never loaded"):
        ops_id.id_loss(x.to(DEV), y.to(DEV), ops_id.IdNet().to(DEV).eval())
    net.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            ops_id.id_loss(x.to(DEV), y.to(DEV), net)
    finally:
        net.eval()


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


def _plain_id(sd_dev, mask=None):
    def f(r, t):
        if mask is not None:
            r, t = r * mask, t * mask
        return 0.1 * M.id_loss(r, t, sd_dev)[0]
    return f


def test_pti_step_id_term_matches_plain_pytorch(net3_sd, sd, net):
    from e4s2024_amd import pti
    sd_dev = {k: v.to(DEV) for k, v in sd.items()}
    pnet, vec, lab, target, fg = _pti_setup(net3_sd)
    params = pti.trainable_parameters(pnet)
    opt = torch.optim.SGD(params, lr=0.0)
    torch.manual_seed(7)
    loss_a, _ = pti.pti_step(pnet, opt, vec, lab, target, foreground_mask=fg, id_loss=net)
    ga = _grads(params)
    torch.manual_seed(7)
    loss_b, _ = pti.pti_step(pnet, opt, vec, lab, target, foreground_mask=fg, extra_loss=_plain_id(sd_dev, fg))
    gb = _grads(params)
    assert abs(loss_a.item() - loss_b.item()) <= 1e-4 * abs(loss_b.item())
    torch.manual_seed(7)
    loss_c, _ = pti.pti_step(pnet, opt, vec, lab, target, foreground_mask=fg)
    gc = _grads(params)
    assert loss_a.item() > loss_c.item()
    worst, moved = 0.0, 0
    for a, b, c in zip(ga, gb, gc):
        assert (a is None) == (b is None)
        if a is None or b.norm() == 0:
            continue
        worst = max(worst, rel_l2(a, b))
        moved += int(rel_l2(c, b) > 1e-4)
    record_parity("pti1024_id.grad_worst_rel_l2", worst, 1e-3)
    assert worst <= 1e-3, worst
    assert moved > 0, "the identity term should change the parameter gradients"


def test_style_vector_step_id_term_matches_plain_pytorch(net3_sd, sd, net):
    from e4s2024_amd import pti
    sd_dev = {k: v.to(DEV) for k, v in sd.items()}
    pnet, vec, lab, target, _ = _pti_setup(net3_sd)
    for p in pnet.parameters():
        p.requires_grad_(False)
    latent = vec.clone().requires_grad_(True)
    opt = torch.optim.SGD([latent], lr=0.0)
    pti.style_vector_step(pnet, opt, latent, lab, target, id_loss=net, randomize_noise=False)
    ga = latent.grad.detach().clone()
    pti.style_vector_step(pnet, opt, latent, lab, target, randomize_noise=False, extra_loss=_plain_id(sd_dev))
    gb = latent.grad.detach().clone()
    pti.style_vector_step(pnet, opt, latent, lab, target, randomize_noise=False)
    gc = latent.grad.detach().clone()
    r = rel_l2(ga, gb)
    record_parity("w_optim1024_id.latent_grad_rel_l2", r, 1e-3)
    assert r <= 1e-3, r
    assert rel_l2(gc, gb) > 1e-4


def test_graphed_pti_step_with_id_follows_eager(net3_sd, sd, tmp_path):
    from e4s2024_amd import pti
    net_b, vec, lab, target, fg = _pti_setup(net3_sd)
    net_c = _pti_setup(net3_sd)[0]
    m = _dropin(sd, tmp_path)
    opt_b = torch.optim.Adam(pti.trainable_parameters(net_b), lr=1e-3, capturable=True, fused=True)
    opt_c = torch.optim.Adam(pti.trainable_parameters(net_c), lr=1e-3, capturable=True, fused=True)
    step = pti.GraphedPTIStep(net_b, opt_b, vec, lab, target, fg, randomize_noise=False, warmup=2, id_loss=m)

    def eager():
        opt_c.zero_grad(set_to_none=True)
        loss, _ = pti._loss(net_c, vec, lab, target, fg, 1.0, None, False, id_loss=m)
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
    m.facenet.load_state_dict(seeded.seeded_irse50_state_dict(5))     # new weights after the capture: the graph would still read the old copies
    with pytest.raises(RuntimeError, match="changed after the capture"):
        step(vec, lab, target, fg)


def test_pti_step_refuses_unloaded_id_net(net3_sd):
    from e4s2024_amd import pti
    pnet, vec, lab, target, fg = _pti_setup(net3_sd)
    before = [p.detach().clone() for p in pti.trainable_parameters(pnet)[:4]]
    opt = torch.optim.Adam(pti.trainable_parameters(pnet), lr=1e-3, fused=True)
    with pytest.raises(RuntimeError, match="never loaded"):
        pti.pti_step(pnet, opt, vec, lab, target, foreground_mask=fg, id_loss=ops_id.IdNet().to(DEV).eval())
    assert all(torch.equal(a, p) for a, p in zip(before, pti.trainable_parameters(pnet)[:4]))


def test_pti_step_with_lpips_and_id_runs_no_library_kernel(net3_sd, net):
    from torch.profiler import profile, ProfilerActivity
    from e4s2024_amd import pti
    install_dropin()
    from criteria.lpips.lpips import LPIPS
    lp = LPIPS(net_type="alex").to(DEV).eval()
    lp.load_state_dict(seeded.seeded_lpips_state_dict(31))
    pnet, vec, lab, target, fg = _pti_setup(net3_sd)
    opt = torch.optim.Adam(pti.trainable_parameters(pnet), lr=1e-3, fused=True)
    pti.pti_step(pnet, opt, vec, lab, target, foreground_mask=fg, lpips=lp, id_loss=net)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        pti.pti_step(pnet, opt, vec, lab, target, foreground_mask=fg, lpips=lp, id_loss=net)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad_ops = {"aten::mm", "aten::bmm", "aten::addmm", "aten::baddbmm", "aten::matmul", "aten::convolution", "aten::_convolution",
               "aten::convolution_backward", "aten::miopen_convolution", "aten::conv2d", "aten::conv_transpose2d", "aten::linear"}
    hit = [n for n in names if n in bad_ops or n.startswith("Cijk_") or "miopen" in n.lower() or "MIOpen" in n or "igemm" in n.lower()]
    assert not hit, hit
    assert any("id_head_partial" in n for n in names) and any("id_se_dot" in n for n in names), "the profile should show the ID kernels"
    assert any("lpips" in n for n in names)
