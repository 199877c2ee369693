"""GPU parity of the region-aware synthesis path against the golden fixtures (outputs of the
reference) and the faithful 12-pass CPU oracle, through the drop-in modules -> ctypes -> libe4s_hip.so."""
import numpy as np
import pytest
import torch

from conftest import load_golden, install_dropin, template_from_manifest, record_parity
from e4s2024_amd import seeded
from oracle import e4s_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
PIXEL_TOL = 1e-3   # BASELINE.json north_star: <= 1e-3 max-abs fp32 on generated pixels
# Single layers: the default split-bf16 arithmetic (3 bf16 MFMAs per fp32 product, fp32 accumulate) carries ~2^-16 relative
# error per layer (outputs here are O(5)); E4S_MODCONV=f32 (exact fp32 MFMA) meets 3e-5 on the same fixtures.
from e4s2024_amd import ops as _ops
LAYER_TOL = 2e-4 if _ops.MODCONV_MODE == "sb" else 3e-5


def maxdiff(a, b):
    return (a.detach().double().cpu() - torch.as_tensor(b).double()).abs().max().item()


@pytest.fixture(scope="module")
def sg2():
    install_dropin()
    from models.stylegan2 import model
    return model


def _load(m, g, prefix):
    sd = {k[len(prefix):]: T(g[k]) for k in g.files if k.startswith(prefix)}
    m.load_state_dict(sd)
    return m.to(DEV)


def test_g3_modulated_conv(sg2):
    g = load_golden("g3_modconv")
    for name, kw in (("same", dict(kernel_size=3)), ("up", dict(kernel_size=3, upsample=True)), ("rgb", dict(kernel_size=1, demodulate=False))):
        m = sg2.ModulatedConv2d(16, 3 if name == "rgb" else 24, kw.pop("kernel_size"), 512, **kw)
        with torch.no_grad():
            m.weight.copy_(T(g[f"{name}.w"]))
            m.modulation.weight.copy_(T(g[f"{name}.mw"]))
            m.modulation.bias.copy_(T(g[f"{name}.mb"]))
        m = m.to(DEV)
        with torch.no_grad():
            y = m(T(g[f"{name}.x"]).to(DEV), T(g[f"{name}.s"]).to(DEV))
        assert tuple(y.shape) == g[f"{name}.y"].shape
        assert maxdiff(y, g[f"{name}.y"]) <= LAYER_TOL, name


def test_g4_masked_layers_incl_empty_region(sg2):
    g = load_golden("g4_styled")
    mask = seeded.labels_to_onehot(g["labels"], 5).to(DEV)
    with torch.no_grad():
        for name, up in (("same", False), ("up", True)):
            m = _load(sg2.StyledConv(16, 24, 3, 512, upsample=up, mask_op=True), g, f"{name}.sd.")
            y = m(T(g[f"{name}.x"]).to(DEV), T(g[f"{name}.s"]).to(DEV), mask, noise=T(g[f"{name}.nz"]).to(DEV))
            assert maxdiff(y, g[f"{name}.y"]) <= LAYER_TOL, name
        m = _load(sg2.ToRGB(16, 512, upsample=True, mask_op=True), g, "rgb.sd.")
        y = m(T(g["rgb.x"]).to(DEV), T(g["rgb.s"]).to(DEV), mask, T(g["rgb.skip"]).to(DEV))
        assert maxdiff(y, g["rgb.y"]) <= 3e-5                      # ToRGB is fp32 VALU in both modes


def test_forward_only_kernels_refuse_backward(sg2):
    """The encoder's fused units have no backward of any kind yet and must fail loudly; the synthesis layers back-propagate through
    the stock-PyTorch form (tests/test_gpu_backward.py)."""
    install_dropin()
    from models.encoders.psp_encoders import SEModule
    m = SEModule(32, 16).to(DEV)
    x = torch.randn(1, 32, 8, 8, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        m(x).sum().backward()
    c = sg2.StyledConv(16, 24, 3, 512, mask_op=False).to(DEV)
    x = torch.randn(1, 16, 8, 8, device=DEV, requires_grad=True)
    c(x, torch.randn(1, 512, device=DEV), None, noise=torch.zeros(1, 1, 8, 8, device=DEV)).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


@pytest.mark.parametrize("tag,man", [("s64", "generator_64_rli5"), ("s256", "generator_256_rli13")])
def test_g5_small_generators(sg2, manifest, tag, man):
    g = load_golden("g5_generator_small")
    size, rli, ncls, bs = (int(v) for v in g[tag + ".cfg"])
    lab = seeded.blocky_labels(22, bs, ncls, 64, cells=8)
    lab[:, 5:9, 3:40] = (lab[:, 5:9, 3:40] + 1) % ncls
    n_latent = int(np.log2(size)) * 2 - 2
    codes = seeded.seeded_codes(23, bs, ncls, n_latent, seeded.seeded_latent_avg(2, n_latent))
    sd = seeded.seeded_state_dict(template_from_manifest(manifest[man]), 21, "net3")
    gen = sg2.Generator(size, 512, 8, split_layer_idx=5, remaining_layer_idx=rli)
    gen.load_state_dict({k[2:]: v for k, v in sd.items()})
    gen = gen.to(DEV).eval()
    with torch.no_grad():
        img, none, feats = gen([codes.to(DEV)], None, seeded.labels_to_onehot(lab, ncls).to(DEV), input_is_latent=True, randomize_noise=False)
    assert none is None
    d = maxdiff(img, g[tag + ".image"])
    record_parity(f"g5.generator{size}.pixels_vs_reference_golden[{_ops.MODCONV_MODE}]", d, 5e-4)
    assert d <= 5e-4
    f = feats.flatten().cpu()
    assert maxdiff(f[:: max(1, f.numel() // 4096)], g[tag + ".feats_sample"]) <= 5e-4


def test_generator512_default_settings_vs_oracle(sg2):
    """A size-512 generator (its last stage is 64 -> 64 @512 AND the last layer: the split-plane chain must stop one stage earlier there — the round-2
    advisor's crash) under the default settings against the oracle's twelve-pass forward (models/stylegan2/model.py:607-698)."""
    size, rli, ncls, bs = 512, 13, 12, 1
    gen = sg2.Generator(size, 512, 8, split_layer_idx=5, remaining_layer_idx=rli)
    seeded.apply_seeded(gen, 21, "net3", prefix="G.")
    sd = {"G." + k: v.clone() for k, v in gen.state_dict().items()}
    n_latent = int(np.log2(size)) * 2 - 2
    lab = seeded.blocky_labels(31, bs, ncls, 512, cells=16)
    codes = seeded.seeded_codes(23, bs, ncls, n_latent, seeded.seeded_latent_avg(2, n_latent))
    mask = seeded.labels_to_onehot(lab, ncls)
    ref, _ = O.generator_forward(sd, codes, mask, None, size=size, remaining_layer_idx=rli, split_layer_idx=5)
    gen = gen.to(DEV).eval()
    with torch.no_grad():
        img, _, _ = gen([codes.to(DEV)], None, mask.to(DEV), input_is_latent=True, randomize_noise=False)
    assert tuple(img.shape) == (bs, 3, size, size)
    d = maxdiff(img, ref)
    record_parity(f"generator512.pixels_vs_oracle[{_ops.MODCONV_MODE}]", d, 1e-3)
    assert d <= 1e-3


def _config2_inputs(bs, seed_labels=3, iid=False):
    la = seeded.seeded_latent_avg(2, 18)
    codes = seeded.seeded_codes(1, bs, 12, 18, la)
    lab = seeded.iid_labels(9, bs, 12, 512) if iid else seeded.blocky_labels(seed_labels, bs, 12, 512, cells=16)
    return codes, seeded.labels_to_onehot(lab, 12)


def test_g6_gen_img_1024_golden(gpu_net3):
    g = load_golden("g6_gen1024")
    codes, mask = _config2_inputs(1)
    with torch.no_grad():
        img, minus1, feats = gpu_net3.gen_img(torch.zeros(1, 512, 32, 32, device=DEV), codes.to(DEV), mask.to(DEV), randomize_noise=False)
    assert minus1 == -1 and tuple(img.shape) == (1, 3, 1024, 1024) and tuple(feats.shape) == (1, 512, 16, 16)
    ic = img.cpu()
    d = max(maxdiff(ic.flatten()[g["pix_idx"]], g["pix"]), maxdiff(ic[0, :, 480:544, 480:544], g["crop"]), maxdiff(ic[0, :, 777, :], g["row"]))
    record_parity(f"g6.gen_img1024_blocky.pixels_vs_reference_golden[{_ops.MODCONV_MODE}]", d, PIXEL_TOL)
    assert d <= PIXEL_TOL
    assert maxdiff(feats.flatten().cpu()[::32], g["feats_sample"]) <= PIXEL_TOL
    assert abs(ic.double().mean().item() - g["stats"][0]) < 1e-4


def test_g6_gen_img_1024_iid_labels_golden(gpu_net3):
    """Adversarial masks: every tile mixes all 12 regions."""
    g = load_golden("g6_gen1024_iid")
    codes, mask = _config2_inputs(1, iid=True)
    with torch.no_grad():
        img, _, _ = gpu_net3.gen_img(torch.zeros(1, 512, 32, 32, device=DEV), codes.to(DEV), mask.to(DEV), randomize_noise=False)
    ic = img.cpu()
    d = max(maxdiff(ic.flatten()[g["pix_idx"]], g["pix"]), maxdiff(ic[0, :, 448:576, 448:576], g["crop"]))
    record_parity(f"g6.gen_img1024_iid.pixels_vs_reference_golden[{_ops.MODCONV_MODE}]", d, PIXEL_TOL)
    assert d <= PIXEL_TOL


def test_gen_img_batch4_properties(gpu_net3):
    """BASELINE config 2 size (bs=4): samples are independent (sample b of the batch == the single-sample run up to the
    re-association of the split-K reduction, whose slice count depends on the launch size), the run is bit-deterministic,
    and explicit noise == registered buffers."""
    codes, mask = _config2_inputs(4)
    codes, mask = codes.to(DEV), mask.to(DEV)
    with torch.no_grad():
        img4, _, f4 = gpu_net3.gen_img(None, codes, mask, randomize_noise=False)
        img4b, _, _ = gpu_net3.gen_img(None, codes, mask, randomize_noise=False)
        assert torch.equal(img4, img4b)
        # With the f16 + MX-fp6 arithmetic of the masked layers (E4S_MX=2) a last-bit difference upstream — the 4^2-32^2 layers' split-K slice count
        # depends on the launch size — can move a value across an f16 rounding boundary or a block's power-of-two scale, i.e. two evaluations differ
        # by up to the arithmetic's own error (2e-4 on the pixels), not by the perturbation: the bound follows the arithmetic, not 1e-4.
        tol = 5e-4 if _ops.mx_arith() == 1 else 1e-4
        for b in (0, 3):
            img1, _, f1 = gpu_net3.gen_img(None, codes[b:b + 1], mask[b:b + 1].contiguous(), randomize_noise=False)
            d_img, d_f = (img1[0] - img4[b]).abs().max().item(), (f1[0] - f4[b]).abs().max().item()
            record_parity(f"gen1024.batch4_face{b}_vs_alone.pixels", d_img, tol)
            assert d_img <= tol and d_f <= 1e-4, (d_img, d_f)
        noise = [getattr(gpu_net3.G.noises, f"noise_{i}") for i in range(17)]
        img_n, _, _ = gpu_net3.gen_img(None, codes, mask, noise=noise)
        assert torch.equal(img_n, img4)
        # randomize_noise=True draws fresh noise: different output, same statistics
        img_r, _, _ = gpu_net3.gen_img(None, codes, mask)
        assert not torch.equal(img_r, img4) and abs(img_r.mean().item() - img4.mean().item()) < 0.3
    g = load_golden("g6_gen1024")          # sample 0 of the batch uses the golden's codes / labels
    assert maxdiff(img4[0].flatten().cpu()[g["pix_idx"]], g["pix"]) <= PIXEL_TOL


def test_g8_cal_style_codes(gpu_net3):
    g = load_golden("g8_style_codes")
    with torch.no_grad():
        codes = gpu_net3.cal_style_codes(T(g["vectors"]).to(DEV))
    assert tuple(codes.shape) == tuple(g["shape"])
    assert maxdiff(codes.flatten().cpu()[g["idx"]], g["codes_sample"]) <= 2e-5
    assert maxdiff(codes[0, 7, 13:].cpu(), seeded.seeded_latent_avg(2, 18)[13:]) == 0
    # bs = 3 against the oracle
    v = T(seeded.seeded_array(41, "vec3", (3, 12, 1280), dist="normal"))
    with torch.no_grad():
        c3 = gpu_net3.cal_style_codes(v.to(DEV))
    sd = {k: p.detach().cpu() for k, p in gpu_net3.state_dict().items() if k.startswith("MLPs.")}
    assert maxdiff(c3, O.cal_style_codes(sd, v, seeded.seeded_latent_avg(2, 18), 13)) <= 5e-5


def test_fused_torgb_epilogue_matches_separate_launch(gpu_net3):
    """The optional fusion of the single-region ToRGBs (256/512/1024) into the conv epilogue — and with it the channel-blocked hand-overs
    of the 512x512 / 1024x1024 stages, which are only taken together with the fused ToRGBs — gives the same image up to the rounding of the
    split products (both variants are 6e-5 from the oracle; the parity bar is 1e-3)."""
    if _ops.MODCONV_MODE != "sb":
        pytest.skip("fused ToRGB exists on the split-bf16 kernel only")
    codes, mask = _config2_inputs(2)
    codes, mask = codes.to(DEV), mask.to(DEV)
    old = _ops.FUSE_RGB
    try:
        with torch.no_grad():
            _ops.FUSE_RGB = False
            a, _, _ = gpu_net3.gen_img(None, codes, mask, randomize_noise=False)
            _ops.FUSE_RGB = True
            b, _, _ = gpu_net3.gen_img(None, codes, mask, randomize_noise=False)
    finally:
        _ops.FUSE_RGB = old
    # (2e-4: with E4S_SP_CHAIN=0 the unfused route runs the 512 / 1024 stages on the split-bf16 kernels and the fused one on f16 + fp6 — two
    #  roundings of the same products, 1.05e-4 apart on this input; each is 6e-5..1.1e-4 from the oracle against the 1e-3 bar)
    assert (a - b).abs().max().item() <= 2e-4


@pytest.mark.parametrize("links", ["all", "c", "c7", "u6,c6"])
def test_channels_last_chain_gives_the_same_image(gpu_net3, links):
    """The single-region layers hand their activations over channel-blocked, [bs, C/8, H, W, 8] (kernel variants of csrc/modconv_sb.hip and
    csrc/modconv_upfused.hip; default: the "c" links).  Same image as with channels-first hand-overs up to the rounding of the split
    products, for the whole chain and for partial chains (every mix of layouts at the kernel boundaries)."""
    if _ops.MODCONV_MODE != "sb":
        pytest.skip("split-bf16 kernels only")
    codes, mask = _config2_inputs(2)
    codes, mask = codes.to(DEV), mask.to(DEV)
    old = (_ops.NHWC_CHAIN, _ops.NHWC_LINKS, _ops.region_modconv3x3, _ops.modconv_up_single)
    old_sp, _ops.SP_CHAIN = _ops.SP_CHAIN, False        # the blocked route is what runs when the split-plane chain (tests/test_gpu_chain.py) is off
    blocked_calls = []

    def counting(fn):
        def wrapper(*args, **kw):
            if kw.get("x_nhwc") or kw.get("out_nhwc"):
                blocked_calls.append((fn.__name__, bool(kw.get("x_nhwc")), bool(kw.get("out_nhwc"))))
            return fn(*args, **kw)
        return wrapper
    try:
        with torch.no_grad():
            _ops.NHWC_CHAIN = False
            a, _, _ = gpu_net3.gen_img(None, codes, mask, randomize_noise=False)
            _ops.NHWC_CHAIN, _ops.NHWC_LINKS = True, links
            _ops.region_modconv3x3, _ops.modconv_up_single = counting(old[2]), counting(old[3])
            b, _, _ = gpu_net3.gen_img(None, codes, mask, randomize_noise=False)
    finally:
        _ops.NHWC_CHAIN, _ops.NHWC_LINKS, _ops.region_modconv3x3, _ops.modconv_up_single = old
        _ops.SP_CHAIN = old_sp
    # (two routes through different kernels: the same products in other summation orders and, since round 5, the 128 -> 256 layer's region-uniform blocks on f16 + fp6
    #  in one route and the composed split-bf16 kernel in the other — 1.05e-4 measured; the bar that counts is 1e-3 against the reference goldens)
    d = (a - b).abs().max().item()
    record_parity(f"channels_last_chain.{links}.pixels_vs_channels_first", d, 2e-4)
    assert a.shape == b.shape and d <= 2e-4
    assert len(blocked_calls) >= 2, blocked_calls        # the blocked route was really taken (a producer and a consumer at least)


@pytest.mark.parametrize("shape", [(2, 20, 40, 9, 13), (1, 16, 24, 8, 8), (3, 48, 33, 30, 17), (1, 64, 32, 64, 64)])
def test_up_fused_matches_two_stage_and_oracle(sg2, shape):
    """Single-region up layer: the one-launch kernel (pre-blur tile kept in LDS) against the tconv + blur-epilogue pair and the
    oracle's ModulatedConv2d upsample branch (model.py:287-301), incl. ragged sizes, cout not a multiple of 32, per-sample noise.
    (Per-kernel bars against the emulation of each kernel's own arithmetic: tests/test_gpu_modconv_variants.py.)"""
    if _ops.MODCONV_MODE != "sb":
        pytest.skip("split-bf16 kernels only")
    bs, cin, cout, h, w = shape
    rs = np.random.RandomState(1234 + cin)
    m = sg2.StyledConv(cin, cout, 3, 512, upsample=True, mask_op=False)
    with torch.no_grad():
        m.conv.weight.copy_(T(rs.standard_normal(m.conv.weight.shape).astype(np.float32)))
        m.conv.modulation.weight.copy_(T(rs.standard_normal(m.conv.modulation.weight.shape).astype(np.float32)))
        m.noise.weight.fill_(0.37)
        m.activate.bias.copy_(T(0.1 * rs.standard_normal(cout).astype(np.float32)))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV)
    x = T(rs.standard_normal((bs, cin, h, w)).astype(np.float32))
    st = T(rs.standard_normal((bs, 512)).astype(np.float32))
    nz = T(rs.standard_normal((bs, 1, 2 * h, 2 * w)).astype(np.float32))
    old = _ops.UP_FUSED
    try:
        with torch.no_grad():
            _ops.UP_FUSED = True
            a = m(x.to(DEV), st.to(DEV), None, noise=nz.to(DEV))
            _ops.UP_FUSED = False
            b = m(x.to(DEV), st.to(DEV), None, noise=nz.to(DEV))
    finally:
        _ops.UP_FUSED = old
    ref = O.styled_conv(sd, "", x, st, None, nz, masked=False, upsample=True)
    scale = max(1.0, float(ref.abs().max()))
    assert tuple(a.shape) == tuple(ref.shape)
    assert (a - b).abs().max().item() <= 2e-5 * scale
    assert maxdiff(a, ref) <= LAYER_TOL * scale


RAGGED = [  # (bs, cin, cout, h, w, nreg, label_h, label_w)
    (1, 7, 5, 5, 9, 3, 5, 9),            # tiny, channels far from any tile multiple
    (2, 20, 40, 13, 21, 12, 32, 32),     # label map at another resolution, non-integer nearest ratio
    (1, 48, 33, 40, 35, 7, 64, 64),      # crosses a 32-wide tile boundary, Cout = 32 + 1
    (3, 130, 70, 6, 6, 2, 6, 6),         # small map with a long K (split-K path), Cin not a multiple of 16
    (1, 16, 136, 34, 70, 12, 70, 140),   # Cout > 128 on a wide map (the 512-thread masked tile + a channel tail)
]


@pytest.mark.parametrize("shape", RAGGED)
@pytest.mark.parametrize("upsample", [False, True])
def test_masked_layers_ragged_shapes_against_oracle(sg2, shape, upsample):
    """StyledConv (masked, same / up) and ToRGB on ragged sizes: odd spatial sizes, channel tails, few regions, pixels that belong to
    no region (label 255 -> zero, like the reference's masked sum), label maps at a different resolution than the features.
    (Which tile and kernel variant a shape reaches, and per-kernel bars against the emulation of its arithmetic: tests/test_gpu_modconv_variants.py.)"""
    bs, cin, cout, h, w, nreg, lh, lw = shape
    rs = np.random.RandomState(100 * cin + h + (7 if upsample else 0))
    lab = rs.randint(0, nreg, (bs, lh, lw)).astype(np.uint8)
    lab[:, : max(1, lh // 7), : max(1, lw // 5)] = 255                       # a corner that belongs to no region
    onehot = torch.zeros(bs, nreg, lh, lw)
    for c in range(nreg):
        onehot[:, c] = T((lab == c).astype(np.float32))
    m = sg2.StyledConv(cin, cout, 3, 512, upsample=upsample, mask_op=True)
    with torch.no_grad():
        m.conv.weight.copy_(T(rs.standard_normal(m.conv.weight.shape).astype(np.float32)))
        m.conv.modulation.weight.copy_(T(rs.standard_normal(m.conv.modulation.weight.shape).astype(np.float32)))
        m.noise.weight.fill_(0.21)
        m.activate.bias.copy_(T(0.1 * rs.standard_normal(cout).astype(np.float32)))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = T(rs.standard_normal((bs, cin, h, w)).astype(np.float32))
    st = T(rs.standard_normal((bs, nreg, 512)).astype(np.float32))
    ho, wo = (2 * h, 2 * w) if upsample else (h, w)
    nz = T(rs.standard_normal((bs, 1, ho, wo)).astype(np.float32))
    m = m.to(DEV)
    with torch.no_grad():
        y = m(x.to(DEV), st.to(DEV), T(lab).to(DEV), noise=nz.to(DEV))
    ref = O.styled_conv(sd, "", x, st, onehot, nz, masked=True, upsample=upsample)
    scale = max(1.0, float(ref.abs().max()))
    assert tuple(y.shape) == tuple(ref.shape)
    assert maxdiff(y, ref) <= LAYER_TOL * scale, (shape, upsample, maxdiff(y, ref), scale)
    if not upsample:
        rgb = sg2.ToRGB(cin, 512, upsample=False, mask_op=True)
        with torch.no_grad():
            rgb.conv.weight.copy_(T(rs.standard_normal(rgb.conv.weight.shape).astype(np.float32)))
            rgb.conv.modulation.weight.copy_(T(rs.standard_normal(rgb.conv.modulation.weight.shape).astype(np.float32)))
            rgb.bias.copy_(T(0.1 * rs.standard_normal((1, 3, 1, 1)).astype(np.float32)))
        sdr = {k: v.detach().clone() for k, v in rgb.state_dict().items()}
        rgb = rgb.to(DEV)
        with torch.no_grad():
            yr = rgb(x.to(DEV), st.to(DEV), T(lab).to(DEV), None)
        refr = O.to_rgb(sdr, "", x, st, onehot, None, masked=True)
        assert maxdiff(yr, refr) <= 3e-5 * max(1.0, float(refr.abs().max()))


@pytest.mark.parametrize("shape", [(2, 32, 128, 32, 32, 5, 64, 64), (1, 64, 136, 40, 32, 12, 160, 128), (1, 32, 128, 32, 48, 3, 32, 48), (1, 96, 192, 64, 32, 12, 128, 64)])
def test_masked_up_layer_uniform_blocks_against_oracle_and_composed_form(sg2, shape):
    """Masked up-sampling StyledConv with the region-uniform 16 x 16 output blocks in the transposed-conv form (``e4s_masked_upconv_blocks_mx``) and
    the mixed ones in the composed form: label maps made of uniform blocks, mixed blocks, blocks without a region and a label map at another
    resolution — against the oracle, against the all-composed route, and every block computed by exactly one of the two kernels."""
    if _ops.mx_arith() != 1:
        pytest.skip("the block path is the f16 + fp6 route (csrc/modconv_upblock_mx.hip); the split-bf16 arithmetic runs the whole layer in the composed form")
    bs, cin, cout, h, w, nreg, lh, lw = shape
    rs = np.random.RandomState(17 * cin + h)
    # region maps built at block granularity: every 16 x 16 output block gets one region, then one row of blocks gets per-pixel noise in its left half
    # (mixed blocks: the whole 64-pixel tile row falls back to the composed form) and the last block row a corner that belongs to no region
    ho, wo = 2 * h, 2 * w
    cy, cx = 16 * lh // ho, 16 * lw // wo                                     # a block in label pixels
    cells = rs.randint(0, nreg, (bs, ho // 16, wo // 16)).astype(np.uint8)
    lab = np.repeat(np.repeat(cells, cy, axis=1), cx, axis=2)
    lab[:, cy:2 * cy, : lw // 2] = rs.randint(0, nreg, (bs, cy, lw // 2))       # second row of 16 x 16 blocks: noise
    lab[:, lh - cy // 2:, lw - cx // 2:] = 255                                  # no region
    onehot = torch.zeros(bs, nreg, lh, lw)
    for c in range(nreg):
        onehot[:, c] = T((lab == c).astype(np.float32))
    m = sg2.StyledConv(cin, cout, 3, 512, upsample=True, mask_op=True)
    with torch.no_grad():
        m.conv.weight.copy_(T(rs.standard_normal(m.conv.weight.shape).astype(np.float32)))
        m.conv.modulation.weight.copy_(T(rs.standard_normal(m.conv.modulation.weight.shape).astype(np.float32)))
        m.noise.weight.fill_(0.21)
        m.activate.bias.copy_(T(0.1 * rs.standard_normal(cout).astype(np.float32)))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = T(rs.standard_normal((bs, cin, h, w)).astype(np.float32))
    st = T(rs.standard_normal((bs, nreg, 512)).astype(np.float32))
    nz = T(rs.standard_normal((bs, 1, 2 * h, 2 * w)).astype(np.float32))
    m = m.to(DEV)
    labd = T(lab).to(DEV)
    blocks, sub = (t.cpu().numpy() for t in _ops.uniform_blocks(labd, 2 * h, 2 * w, nreg))
    assert (blocks < nreg).any() and (blocks == 255).any()                    # uniform and mixed blocks are present
    assert sub.shape == (bs, blocks.shape[1] * 2, blocks.shape[2] * 2)
    old, old_w, old_pc = _ops.UP_BLOCKS, _ops.UP_BLOCKS_MIN_WIDTH, (_ops.UP_BLOCKS_MIN_PERCENT, _ops.UP_BLOCKS_MIN_PERCENT_SMALL)
    _ops.UP_BLOCKS_MIN_WIDTH = 32                                             # (the default tries the path from width 128 up only)
    _ops.UP_BLOCKS_MIN_PERCENT = _ops.UP_BLOCKS_MIN_PERCENT_SMALL = 1        # ... and only where most tiles qualify: here both kernels must run
    try:
        with torch.no_grad():
            _ops.UP_BLOCKS = True
            y = m(x.to(DEV), st.to(DEV), labd, noise=nz.to(DEV))
            y2 = m(x.to(DEV), st.to(DEV), labd, noise=nz.to(DEV))
            # single writer: the output NaN-prefilled, each kernel of the pair alone — every element is written by exactly one of them
            _ops.UP_BLOCKS_ONLY_ONE_KERNEL = "blocks"
            yb = m(x.to(DEV), st.to(DEV), labd, noise=nz.to(DEV))
            _ops.UP_BLOCKS_ONLY_ONE_KERNEL = "composed"
            ym = m(x.to(DEV), st.to(DEV), labd, noise=nz.to(DEV))
            _ops.UP_BLOCKS_ONLY_ONE_KERNEL = None
            _ops.UP_BLOCKS = False
            yc = m(x.to(DEV), st.to(DEV), labd, noise=nz.to(DEV))
    finally:
        _ops.UP_BLOCKS, _ops.UP_BLOCKS_MIN_WIDTH, _ops.UP_BLOCKS_ONLY_ONE_KERNEL = old, old_w, None
        _ops.UP_BLOCKS_MIN_PERCENT, _ops.UP_BLOCKS_MIN_PERCENT_SMALL = old_pc
    wb, wm = torch.isfinite(yb), torch.isfinite(ym)
    assert wb.any() and wm.any(), "both kernels of the pair must have work here"
    assert not (wb & wm).any(), "an output element written by both kernels"
    assert (wb | wm).all(), "an output element written by neither kernel"
    # ... in whole 16 x 16 blocks of all channels, and what each wrote is what the pair writes together
    wb16 = wb.reshape(bs, cout, ho // 16, 16, wo // 16, 16)
    assert (wb16.all(dim=(1, 3, 5)) | (~wb16).all(dim=(1, 3, 5))).all()
    assert torch.equal(torch.where(wb, yb, ym), y)
    ref = O.styled_conv(sd, "", x, st, onehot, nz, masked=True, upsample=True)
    scale = max(1.0, float(ref.abs().max()))
    assert torch.equal(y, y2)
    d_or, d_co = maxdiff(y, ref), (y - yc).abs().max().item()
    record_parity(f"masked_up_blocks.{cin}to{cout}_{h}x{w}.vs_oracle", d_or / scale, LAYER_TOL)
    # block route against composed route: two kernels on the same f16 + fp6 arithmetic with different block-scale groupings and summation orders
    # (measured 2e-5 .. 5e-5 of the output scale: a bound tighter than the bar against the oracle)
    assert d_or <= LAYER_TOL * scale and d_co <= 1e-4 * scale, (shape, d_or, d_co, scale)


def test_batched_style_tables_match_the_one_layer_launches():
    """``ops.style_demod_plan`` (every layer's modulation / demodulation table in two launches: EqualLinear of model.py:262-274 and the demodulation of :276-285; the
    32 dot products of a block reduced by one transposing butterfly — bit-identical to 32 wave sums: tools/probes/wave_sum_probe.hip — the style rows of the
    demodulation staged in LDS) against ``ops.style_demod`` layer by layer, to an ulp or two (the two kernels' per-lane products contract into FMAs differently) — ragged channel counts, strided style views (one W+ index of a [bs, regions, 18, 512] latent), a layer without demodulation, 13 (batch, region) rows."""
    from e4s2024_amd import ops
    g = torch.Generator(device=DEV).manual_seed(5)
    bs, nreg = 3, 7
    latent = torch.randn(bs, nreg, 18, 512, device=DEV, generator=g)
    layers = [(512, 512, 0), (512, 256, 3), (72, 40, 5), (30, 3, 7), (256, 128, 9), (1024, 64, 11)]
    jobs, want = [], {}
    for i, (cin, cout, widx) in enumerate(layers):
        styles = latent[:, :, widx]                                 # strided view, unit inner stride
        mw = torch.randn(cin, 512, device=DEV, generator=g)
        mb = torch.randn(cin, device=DEV, generator=g)
        wsq = None if i == 3 else torch.rand(cin, cout, device=DEV, generator=g) + 0.1
        jobs.append((i, styles, mw, mb, wsq, cout))
        want[i] = ops.style_demod(styles, mw, mb, wsq, cout)
    ops.style_demod_plan(jobs)
    for i, (cin, cout, widx) in enumerate(layers):
        s, d = ops.style_demod_planned(i, jobs[i][1])
        assert float((s - want[i][0]).abs().max()) <= 2e-6 * float(want[i][0].abs().max()), (i, float((s - want[i][0]).abs().max()))
        assert (d is None) == (want[i][1] is None)
        if d is not None:
            assert float(((d - want[i][1]) / want[i][1]).abs().max()) <= 2e-6, i
