"""The recolor guidance term of PTI tuning (video_swap_ft_coach.py:274-287): the multi-target heads of csrc/lpips.hip, idloss.hip, fploss.hip and
pixloss.hip against sums of today's single-target losses, the frame-indexed target cache, the shared two-target PTI step against the naive
composition of two ``calc_loss`` calls on today's kernels, and ``tune_clip`` with recolor frames (graphed, eager, cached, uncached)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import install_dropin
from e4s2024_amd import ops_fp, ops_id, ops_lpips, ops_multi, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return ((a - b).norm() / b.norm()).item()


def _img(seed, bs=1, side=128):
    return torch.tanh(T(seeded.seeded_array(seed, "recolor_img", (bs, 3, side, side), dist="normal"))).to(DEV)


@pytest.fixture(scope="module")
def nets():
    install_dropin()
    from criteria.lpips.lpips import LPIPS
    lp = LPIPS(net_type="alex").to(DEV).eval()
    lp.load_state_dict(seeded.seeded_lpips_state_dict(31))
    idn = ops_id.IdNet()
    idn.load_state_dict(seeded.seeded_irse50_state_dict(7))
    fpn = ops_fp.FaceParsingNet()
    fpn.load_state_dict(seeded.seeded_unet_state_dict(9))
    return lp, idn.to(DEV).eval(), fpn.to(DEV).eval()


def _single(kind, nets, x, y):
    lp, idn, fpn = nets
    if kind == "lpips":
        return ops_lpips.lpips_multiscale(x, y, lp)
    if kind == "id":
        return ops_id.id_loss(x, y, idn)
    return ops_fp.fp_loss(x, y, fpn)


def _multi(kind, nets, x, ys, tw, frame=None):
    lp, idn, fpn = nets
    if kind == "lpips":
        return ops_lpips.lpips_multiscale_multi(x, [ops_lpips.target_features(y, lp) for y in ys], tw, lp, frame)
    if kind == "id":
        return ops_id.id_loss_multi(x, [ops_id.target_features(y, idn) for y in ys], tw, idn, True, frame)
    return ops_fp.fp_loss_multi(x, [ops_fp.target_features(y, fpn) for y in ys], tw, fpn, frame)


def _loss_grad(fn, x):
    xg = x.clone().requires_grad_(True)
    loss = fn(xg)
    (g,) = torch.autograd.grad(loss, xg)
    return loss.detach().double().item(), g


@pytest.mark.parametrize("kind", ["lpips", "id", "fp"])
def test_multi_target_heads_match_sum_of_singles(nets, kind):
    x, y1, y2 = _img(1, 2), _img(2, 2), _img(3, 2)
    w1, w2 = 0.7, 2.3
    l_m, g_m = _loss_grad(lambda xg: _multi(kind, nets, xg, [y1, y2], [w1, w2]), x)
    l_1, g_1 = _loss_grad(lambda xg: _single(kind, nets, xg, y1), x)
    l_2, g_2 = _loss_grad(lambda xg: _single(kind, nets, xg, y2), x)
    want_l, want_g = w1 * l_1 + w2 * l_2, w1 * g_1.double() + w2 * g_2.double()
    assert abs(l_m - want_l) <= 1e-6 * abs(want_l), (l_m, want_l)
    assert (g_m.double() - want_g).abs().max().item() <= 1e-5 * want_g.abs().max().item()
    l_k1, g_k1 = _loss_grad(lambda xg: _multi(kind, nets, xg, [y1], [1.0]), x)      # k = 1, w = 1: today's function
    assert abs(l_k1 - l_1) <= 1e-6 * abs(l_1), (l_k1, l_1)
    assert (g_k1 - g_1).abs().max().item() <= 1e-6 * g_1.abs().max().item()


def test_pixel_term_matches_masked_mse():
    x, y1, y2 = _img(4, 2, 64), _img(5, 2, 64), _img(6, 2, 64)
    fg = (torch.rand((2, 1, 64, 64), generator=torch.Generator().manual_seed(3)) > 0.3).float().to(DEV)
    w1, w2 = 1.0, 5.0
    l_m, g_m = _loss_grad(lambda xg: ops_multi.mse_multi(xg, fg, [y1 * fg, y2 * fg], [w1, w2]), x)
    l_r, g_r = _loss_grad(lambda xg: w1 * F.mse_loss(xg * fg, y1 * fg) + w2 * F.mse_loss(xg * fg, y2 * fg), x)
    assert abs(l_m - l_r) <= 1e-6 * abs(l_r)
    assert (g_m - g_r).abs().max().item() <= 1e-5 * g_r.abs().max().item()


@pytest.mark.parametrize("kind", ["lpips", "id", "fp"])
def test_frame_index_reads_the_cached_frame(nets, kind):
    """Features of a 3-frame clip, frame 2 selected on the device: the same bits as that frame's features passed directly."""
    x = _img(7)
    clip1, clip2 = _img(8, 3), _img(9, 3)
    frame = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    l_c, g_c = _loss_grad(lambda xg: _multi(kind, nets, xg, [clip1, clip2], [1.0, 5.0], frame), x)
    l_d, g_d = _loss_grad(lambda xg: _multi(kind, nets, xg, [clip1[2:], clip2[2:]], [1.0, 5.0]), x)
    assert l_c == l_d and torch.equal(g_c, g_d)


# ------------------------------------------------------------------------------------------------ the PTI objective
def _pti_setup(net3_sd, frames=1):
    from conftest import default_opts
    install_dropin()
    from models.networks import Net3
    net = Net3(default_opts(train_G=True))
    net.load_state_dict(net3_sd)
    net = net.to(DEV).train()
    net.latent_avg = seeded.seeded_latent_avg(2, 18).to(DEV)
    vec = T(seeded.seeded_array(41, "vec", (frames, 12, 1280), dist="normal")).to(DEV)
    lab = T(seeded.blocky_labels(3, frames, 12, 512, 16)).to(DEV).to(torch.uint8)
    target = torch.tanh(T(seeded.seeded_array(5, "img", (frames, 3, 1024, 1024), dist="normal"))).to(DEV)
    recolor = (target * 0.8 + 0.1 * torch.tanh(T(seeded.seeded_array(6, "recolor", (frames, 3, 1024, 1024), dist="normal"))).to(DEV)).clamp(-1, 1)
    return net, vec, lab, target, recolor


def _fg(lab):
    from e4s2024_amd import pti
    return pti.prepare_clip(lab)[1]


def test_first_pti_step_matches_two_calc_loss_calls(net3_sd, nets):
    """The shared two-target step against the naive composition: today's step on the driven frame + recolor_lambda x today's terms on the recoloured
    frame (as extra_loss), all on today's single-target kernels."""
    from e4s2024_amd import pti
    lp, idn, fpn = nets
    net, vec, lab, target, recolor = _pti_setup(net3_sd)
    fg = _fg(lab)
    params = pti.trainable_parameters(net)
    opt = torch.optim.SGD(params, lr=0.0)
    kw = dict(lpips=lp, id_loss=idn, face_parsing=fpn)
    torch.manual_seed(7)
    loss_a, _ = pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, recolor=recolor, recolor_lambda=5.0, **kw)
    ga = [p.grad.detach().clone() if p.grad is not None else None for p in params]

    def recolor_term(r, _t):
        a, b = r * fg, recolor * fg
        return 5.0 * (F.mse_loss(a, b) + 0.8 * ops_lpips.lpips_multiscale(a, b, lp) + 0.1 * ops_id.id_loss(a, b, idn) + 0.1 * ops_fp.fp_loss(a, b, fpn))
    torch.manual_seed(7)
    loss_b, _ = pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, extra_loss=recolor_term, **kw)
    gb = [p.grad.detach().clone() if p.grad is not None else None for p in params]
    assert abs(loss_a.item() - loss_b.item()) <= 1e-5 * abs(loss_b.item()), (loss_a.item(), loss_b.item())
    worst = 0.0
    for a, b in zip(ga, gb):
        assert (a is None) == (b is None)
        if a is not None and b.norm() > 0:
            worst = max(worst, rel_l2(a, b))
    assert worst <= 1e-5, worst
    torch.manual_seed(7)
    loss_z, _ = pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, recolor=recolor, recolor_lambda=0.0, **kw)
    torch.manual_seed(7)
    loss_n, _ = pti.pti_step(net, opt, vec, lab, target, foreground_mask=fg, **kw)
    assert abs(loss_z.item() - loss_n.item()) <= 1e-6 * abs(loss_n.item()), (loss_z.item(), loss_n.item())


def test_pti_step_recolor_without_foreground_mask(net3_sd, nets):
    """No foreground_mask: the driven term is unmasked, the recolor term uses the foreground weight of the map (video_swap_ft_coach.py:284, 286)."""
    from e4s2024_amd import pti
    lp = nets[0]
    net, vec, lab, target, recolor = _pti_setup(net3_sd)
    fg = _fg(lab)
    opt = torch.optim.SGD(pti.trainable_parameters(net), lr=0.0)
    torch.manual_seed(3)
    loss_a, _ = pti.pti_step(net, opt, vec, lab, target, recolor=recolor, lpips=lp)
    torch.manual_seed(3)
    loss_b, _ = pti.pti_step(net, opt, vec, lab, target, lpips=lp, extra_loss=lambda r, _t: 5.0 * (
        F.mse_loss(r * fg, recolor * fg) + 0.8 * ops_lpips.lpips_multiscale(r * fg, recolor * fg, lp)))
    assert abs(loss_a.item() - loss_b.item()) <= 1e-5 * abs(loss_b.item())


def _tune(net3_sd, nets, frames=3, passes=2, **kw):
    from e4s2024_amd import pti
    lp, idn, fpn = nets
    net, vec, lab, target, recolor = _pti_setup(net3_sd, frames)
    opt = torch.optim.Adam(pti.trainable_parameters(net), lr=1e-3, capturable=True, fused=True)
    rec = kw.pop("recolor", recolor)
    return pti.tune_clip(net, opt, target, lab, vec, passes, erode_radius=None, randomize_noise=False, lpips=lp, id_loss=idn, face_parsing=fpn,
                         recolor=rec, **kw)


def test_tune_clip_recolor_graphed_eager_cached(net3_sd, nets):
    graphed = _tune(net3_sd, nets, graphed=True)
    eager = _tune(net3_sd, nets, graphed=False)
    uncached = _tune(net3_sd, nets, graphed=False, cache_targets=False)
    np.testing.assert_allclose(graphed, eager, rtol=3e-3)
    np.testing.assert_allclose(uncached, eager, rtol=1e-6, atol=0)
    without = _tune(net3_sd, nets, graphed=True, recolor=None)
    zero = _tune(net3_sd, nets, graphed=True, recolor_lambda=0.0)
    # Not bit-identical: the fused pixel term sums in another order than ATen's mse_loss, and Adam's first updates are about lr x sign(g) for every
    # parameter, so a 1-ulp change in a near-zero gradient moves it by up to lr (measured 7.8e-6; the first step's loss is held to 1e-6 below)
    np.testing.assert_allclose(zero, without, rtol=1e-4, atol=0)
    assert all(g > w for g, w in zip(graphed, without))           # the term is there


def test_tune_clip_recolor_graphed_without_cache_follows_eager(net3_sd, nets):
    """The captured step with a static recolor buffer: the target features are computed inside the graph on every replay."""
    graphed = _tune(net3_sd, nets, graphed=True, cache_targets=False)
    eager = _tune(net3_sd, nets, graphed=False, cache_targets=False)
    np.testing.assert_allclose(graphed, eager, rtol=3e-3)


def test_graphed_recolor_step_without_foreground_mask_follows_eager(net3_sd, nets):
    """No foreground weight: the recolor term's weight comes from the region map inside the captured graph (prepare_clip under capture)."""
    from e4s2024_amd import pti
    lp = nets[0]
    net_b, vec, lab, target, recolor = _pti_setup(net3_sd)
    net_c = _pti_setup(net3_sd)[0]
    opt_b = torch.optim.Adam(pti.trainable_parameters(net_b), lr=1e-3, capturable=True, fused=True)
    opt_c = torch.optim.Adam(pti.trainable_parameters(net_c), lr=1e-3, capturable=True, fused=True)
    step = pti.GraphedPTIStep(net_b, opt_b, vec, lab, target, None, randomize_noise=False, warmup=2, lpips=lp, recolor=recolor)

    def eager():
        opt_c.zero_grad(set_to_none=True)
        loss, _ = pti._loss_recolor(net_c, vec, lab, target, None, 1.0, None, False, lp, 0.8, None, 0.1, None, 0.1, recolor, 5.0)
        loss.backward()
        opt_c.step()
        return loss.item()

    for _ in range(2):
        eager()
    for _ in range(3):
        lb = step(vec, lab, target, recolor=recolor)[0].item()
        lc = eager()
        assert abs(lb - lc) <= 1e-3 * abs(lc), (lb, lc)


def test_graphed_step_refusals(net3_sd, nets):
    from e4s2024_amd import pti
    lp = nets[0]
    net, vec, lab, target, recolor = _pti_setup(net3_sd)
    fg = _fg(lab)
    opt = torch.optim.Adam(pti.trainable_parameters(net), lr=1e-3, capturable=True, fused=True)
    step = pti.GraphedPTIStep(net, opt, vec, lab, target, fg, randomize_noise=False, warmup=1, lpips=lp)
    with pytest.raises(ValueError, match="recolor"):
        step(vec, lab, target, fg, recolor=recolor)
    cache = pti.TargetCache([target, recolor], fg, lpips=lp)
    step_c = pti.GraphedPTIStep(net, opt, vec, lab, target, fg, randomize_noise=False, warmup=1, lpips=lp, target_cache=cache, frame=0)
    step_c(vec, lab, target, fg, frame=0)
    with pytest.raises(ValueError, match="frame"):
        step_c(vec, lab, target, fg)
    lp.load_state_dict(seeded.seeded_lpips_state_dict(5))         # new weights: the cached target features are stale
    try:
        with pytest.raises(RuntimeError, match="changed"):
            step_c(vec, lab, target, fg, frame=0)
        with pytest.raises(RuntimeError, match="changed"):
            cache.check(lp, None, None)
    finally:
        lp.load_state_dict(seeded.seeded_lpips_state_dict(31))


def test_two_target_step_runs_no_library_kernel(net3_sd, nets):
    from torch.profiler import profile, ProfilerActivity
    from e4s2024_amd import pti
    lp, idn, fpn = nets
    net, vec, lab, target, recolor = _pti_setup(net3_sd)
    fg = _fg(lab)
    opt = torch.optim.Adam(pti.trainable_parameters(net), lr=1e-3, fused=True)
    kw = dict(foreground_mask=fg, recolor=recolor, lpips=lp, id_loss=idn, face_parsing=fpn)
    pti.pti_step(net, opt, vec, lab, target, **kw)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        pti.pti_step(net, opt, vec, lab, target, **kw)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    bad_ops = {"aten::mm", "aten::bmm", "aten::addmm", "aten::baddbmm", "aten::matmul", "aten::convolution", "aten::_convolution",
               "aten::convolution_backward", "aten::miopen_convolution", "aten::conv2d", "aten::conv_transpose2d", "aten::linear"}
    hit = [n for n in names if n in bad_ops or n.startswith("Cijk_") or "miopen" in n.lower() or "MIOpen" in n or "igemm" in n.lower()]
    assert not hit, hit
    for k in ("lpips_head_multi", "id_head_partial_multi", "fp_tap_bwd_multi", "pix_mse_multi"):
        assert any(k in n for n in names), f"the profile should show {k}"


# ------------------------------------------------------------------------------------------------ the reference's objective (g17)
def _g17():
    import os
    import sys
    from conftest import GOLDEN, load_golden
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_pti_recolor as G          # the fixture's seeded inputs (the reference itself is not read here)
    return G, load_golden("g17_pti_recolor")


def test_two_target_objective_matches_g17():
    """The whole objective of train_e4s :277-287 (the reference's calc_loss twice, its LPIPS / IDLoss / FaceParsingLoss in float64) at 1024^2:
    total within 1e-5 relative, the eight terms within 1e-5 (relative for L2 and LPIPS, absolute for the 1 - cos sums of ID and face parsing, as
    for g15 / g16), d loss / d recon at 4096 positions within 5e-3 relative L2 (the face-parsing bar)."""
    from e4s2024_amd import pti
    G, g = _g17()
    install_dropin()
    from criteria.lpips.lpips import LPIPS
    s_lp, s_id, s_fp = (int(v) for v in g["seeds"])
    lp = LPIPS(net_type="alex").to(DEV).eval()
    lp.load_state_dict(seeded.seeded_lpips_state_dict(s_lp))
    idn = ops_id.IdNet()
    idn.load_state_dict(seeded.seeded_irse50_state_dict(s_id))
    idn = idn.to(DEV).eval()
    fpn = ops_fp.FaceParsingNet()
    fpn.load_state_dict(seeded.seeded_unet_state_dict(s_fp))
    fpn = fpn.to(DEV).eval()
    recon, driven, recolor, fg = (t.to(DEV) for t in G.inputs())
    lam = [float(v) for v in g["lambdas"]]
    rl = float(g["recolor_lambda"])
    want, idx, samples = float(g["loss"]), T(g["grad_idx"]).long(), T(g["grad_samples"])
    for cached in (False, True):
        cache = pti.TargetCache([driven, recolor], fg, lp, idn, fpn) if cached else None
        x = recon.clone().requires_grad_(True)
        loss = pti.recolor_objective(x, driven, recolor, fg, None, lam[0], lp, lam[1], idn, lam[2], fpn, lam[3], rl, cache=cache)
        (gx,) = torch.autograd.grad(loss, x)
        assert abs(loss.item() - want) <= 1e-5 * abs(want), (cached, loss.item(), want)
        r = rel_l2(gx.detach().cpu().double().flatten()[idx], samples)
        assert r <= 5e-3, (cached, r)
    a = recon * fg
    for j, y in enumerate((driven, recolor)):
        b = y * fg
        got = [ops_multi.mse_multi(recon, fg, [b], [1.0]).item(),
               ops_lpips.lpips_multiscale_multi(a, [ops_lpips.target_features(b, lp)], [1.0], lp).item(),
               ops_id.id_loss_multi(a, [ops_id.target_features(b, idn)], [1.0], idn).item(),
               ops_fp.fp_loss_multi(a, [ops_fp.target_features(b, fpn)], [1.0], fpn).item()]
        for t, (v, w) in enumerate(zip(got, g["terms"][j])):
            bar = 1e-5 * abs(w) if t < 2 else 1e-5          # ID and face parsing are sums of 1 - cos: absolute bars, as for g15 / g16
            assert abs(v - w) <= bar, (j, t, v, float(w))
