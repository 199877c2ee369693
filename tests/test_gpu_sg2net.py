"""The argument combinations of ``sg2net.modconv`` that neither generator reaches through it: no noise at batch 2 (GPEN runs batch 1, the inpainting network
always has noise), and a per-sample and a shared noise map at batch 2, each on the same-resolution, composed-up and fused-up routes in both arithmetics
(``f32`` has no fused route), with one map on each side of ``SPLITK_MAX_OUT_FLOATS``: below it the samples run one by one with the split-K workspace, above it
in one call without.  Bit for bit: a batch of two equals its two samples run singly, and equals the library entry called here with its arguments written out."""
import pytest
import torch

from e4s2024_amd import ops, sg2net
from e4s2024_amd._lib import lib
from e4s2024_amd.ops import _p, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUT = 24
# (cin, h, bias and activation in the entry): a ragged second channel chunk on a small map; a map of 24 x 296 x 296 floats, just past the split-K limit
SMALL, LARGE = (20, 9, True), (16, 296, False)
ROUTES = [("same", "sb"), ("same", "f32"), ("composed", "sb"), ("composed", "f32"), ("fused", "sb")]
# the fused entry takes no workspace, so the large map would add nothing there
CASES = [(r, a, shape) for r, a in ROUTES for shape in (SMALL, LARGE) if not (r == "fused" and shape == LARGE)]


def randn(seed, *shape, std=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std).to(DEV)


def layer(route, arith, cin):
    W = randn(1, 1, COUT, cin, 3, 3)
    blur = sg2net.fir(4.0, torch.device(DEV))
    wt, wsq = sg2net.prep_styled(W, blur, route == "composed", arith == "sb")
    return dict(wt=wt, wsq=wsq, nw=torch.tensor([0.21], device=DEV), up=route != "same", composed=route == "composed", cin=cin, cout=COUT), blur


def direct(route, sb, L, blur, x, out, s, d, noise, bias, act, n, h, ws, wsn):
    """The library entry of ``route`` with every argument written out."""
    cin, cout = L["cin"], L["cout"]
    nz, nb, nw = (None, 0, None) if noise is None else (_p(noise), noise.shape[0], _p(L["nw"]))
    up = 0 if route == "same" else 1
    if route == "fused":
        lib().call("e4s_modconv_up_fused_sb", _p(out), _p(x), _p(L["wt"][0]), _p(L["wt"][1]), _p(s), _p(d), _p(blur), nz, nb, nw, _p(bias), act, n, cin, cout, h, h,
                   None, _stream())
    elif sb:
        lib().call("e4s_region_modconv3x3_sb", _p(out), _p(x), _p(L["wt"][0]), _p(L["wt"][1]), _p(s), _p(d), None, 0, 0, nz, nb, nw, _p(bias), act, n, cin, cout, h, h,
                   1, up, _p(ws), wsn, None, None, None, None, None, None, None, None, None, _stream())
    else:
        lib().call("e4s_region_modconv3x3", _p(out), _p(x), _p(L["wt"]), _p(s), _p(d), None, 0, 0, nz, nb, nw, _p(bias), act, n, cin, cout, h, h, 1, up, _p(ws), wsn,
                   _stream())


@pytest.mark.parametrize("noise_kind", ["none", "per_sample", "shared"])
@pytest.mark.parametrize("route,arith,shape", CASES, ids=[f"{r}_{a}_{'small' if shape == SMALL else 'large'}" for r, a, shape in CASES])
def test_modconv_batch_of_two(route, arith, shape, noise_kind):
    cin, h, epilogue = shape
    if route != "same":
        h = (h + 1) // 2                                                                      # the output side is the one the workspace rule reads
    ho = h if route == "same" else 2 * h
    large = COUT * ho * ho > ops.SPLITK_MAX_OUT_FLOATS
    assert large == (shape == LARGE)
    sb = arith == "sb"
    with torch.no_grad():
        L, blur = layer(route, arith, cin)
    bs = 2
    x = randn(2, bs, cin, h, h)
    s = (randn(3, bs * cin, std=0.3) + 1).contiguous()
    d = torch.rsqrt(s.view(bs, cin).pow(2) @ L["wsq"] + 1e-8).reshape(-1).contiguous()
    noise = {"none": None, "per_sample": randn(4, bs, 1, ho, ho), "shared": randn(4, 1, 1, ho, ho)}[noise_kind]
    bias, act = (randn(5, COUT, std=0.1), 1) if epilogue else (None, 0)
    empty = lambda n: torch.full((n, COUT, ho, ho), float("nan"), device=DEV)               # noqa: E731  (a plane left unwritten fails torch.equal)
    kw = dict(sb=sb, blur=blur, bias=bias, act=act, h=h, st=_stream())

    got = empty(bs)
    sg2net.modconv(L, x, got, s, d, noise=noise, bs=bs, **kw)
    single = empty(bs)
    for b in range(bs):
        nz = noise[b:b + 1] if noise_kind == "per_sample" else noise
        sg2net.modconv(L, x[b:b + 1], single[b:b + 1], s[b * cin:(b + 1) * cin], d[b * COUT:(b + 1) * COUT], noise=nz, bs=1, **kw)
    want = empty(bs)
    if route == "fused" or large:
        direct(route, sb, L, blur, x, want, s, d, noise, bias, act, bs, h, None, 0)
    else:
        wsn = 16 * COUT * ho * ho
        ws = ops._workspace(x.device, wsn)
        for b in range(bs):
            nz = noise[b:b + 1] if noise_kind == "per_sample" else noise
            direct(route, sb, L, blur, x[b:b + 1], want[b:b + 1], s[b * cin:(b + 1) * cin], d[b * COUT:(b + 1) * COUT], nz, bias, act, 1, h, ws, wsn)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all().item()
    assert torch.equal(got, single)
    assert torch.equal(got, want)
