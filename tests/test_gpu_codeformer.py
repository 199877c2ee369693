"""Row f21 on the GPU: the kernels of csrc/codeformer.hip alone against float64 (the bar of every comparison is ``4 e32``, ``e32`` the float32 restatement's own
distance from float64 on the same input), the head with its codes, gather and AdaIN, then ``codeformer_front`` on the three cases of
tests/golden/g31_codeformer.npz against the float64 model's stored outputs under ``4 e32.<name>`` (the reference's own float32 error), its bit-for-bit
properties and the taps.  Every figure is printed and recorded before it is asserted."""
import numpy as np
import pytest
import torch

import codeformer_model as M
from conftest import load_golden, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def golden():
    return load_golden("g31_codeformer")


@pytest.fixture(scope="module")
def ops():
    from e4s2024_amd import ops
    return ops


def _rand(seed, *shape, std=1.0, mean=0.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * std + mean).astype(np.float32))


def _err(got, want):
    return float((got.detach().cpu().double() - want.double()).abs().max())


def _check(name, got, want64, want32):
    """``got`` (device) against the float64 ``want64`` under 4 x the float32 restatement's own distance from it."""
    err, e32 = _err(got, want64), _err(want32, want64)
    record_parity(name, err, 4 * e32)
    print(f"{name}: err {err:.3e}, e32 {e32:.3e}, err / e32 {err / e32 if e32 else float(err > 0):.2f}")
    assert err <= 4 * e32
    return err


_NETS = {}


def _net(ops, tag):
    if tag not in _NETS:
        net = ops.CodeFormer(*M.CASES[tag]["cfg"]).eval()
        net.load_state_dict(M.case_weights(tag), strict=True)
        _NETS[tag] = net.to(DEV)
    return _NETS[tag]


# ------------------------------------------------------------------------------------------------ GroupNorm + swish
@pytest.mark.parametrize("swish", [True, False], ids=["swish", "plain"])
@pytest.mark.parametrize("shape,mean", [((2, 64, 1, 1), 0.0), ((1, 64, 7, 5), 0.0), ((1, 96, 33, 17), 0.0), ((1, 512, 16, 16), 0.0), ((1, 64, 128, 128), 100.0)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"mean{v:g}")
def test_group_norm_swish(ops, shape, mean, swish):
    C = shape[1]
    x, g, b = _rand(sum(shape), *shape, mean=mean), _rand(C, C, std=0.2, mean=1.0), _rand(C + 1, C, std=0.3)
    got = ops.group_norm_swish(x.to(DEV), g.to(DEV), b.to(DEV), swish=swish)
    assert got.shape == x.shape and got.dtype == torch.float32
    want = M.group_norm(x.double(), g.double(), b.double(), swish)
    _check(f"cf_group_norm.{'x'.join(map(str, shape))}.{'swish' if swish else 'plain'}", got, want, M.group_norm(x, g, b, swish))
    assert ops.group_norm_swish(x[:0].to(DEV), g.to(DEV), b.to(DEV)).shape == (0,) + shape[1:]


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("heads,d,tokens", [(8, 64, 1), (8, 64, 5), (2, 32, 33), (8, 64, 256), (1, 512, 256), (1, 512, 6), (8, 64, 1024)], ids=lambda v: str(v))
def test_attention(ops, heads, d, tokens):
    bs, C = 2, heads * d
    q, k, v = (_rand(heads + d + tokens + i, bs, C, tokens) for i in range(3))
    if tokens == 33:                                  # one score row whose maximum, 90, lies more than 80 above the rest: expf overflows without the max subtraction
        k[0, :d, 7] = q[0, :d, 3] * (90.0 / (d ** -0.5) / float((q[0, :d, 3] ** 2).sum()))
    scale = d ** -0.5
    got = ops.attention_cm(q.to(DEV), k.to(DEV), v.to(DEV), heads)
    assert got.shape == (bs, C, tokens)
    want = M.attention(q.double(), k.double(), v.double(), heads, scale)
    if tokens == 33:
        s = torch.einsum("c,cj->j", q[0, :d, 3].double(), k[0, :d].double()) * scale
        assert float(s[7]) > 89 and float(s[7] - s[torch.arange(33) != 7].max()) > 80
    _check(f"cf_attention.{heads}x{d}x{tokens}", got, want, M.attention(q, k, v, heads, scale))
    # operands that are channel slices of one tensor (a batch stride of 3 C T), as the AttnBlock's q | k | v convolution gives them
    qkv = torch.cat([q, k, v], 1).to(DEV)
    assert torch.equal(ops.attention_cm(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], heads), got)
    # a sample of the batch gets the bits it gets alone
    assert torch.equal(ops.attention_cm(q[1:].to(DEV), k[1:].to(DEV), v[1:].to(DEV), heads), got[1:])


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("tokens", [1, 6, 256])
def test_layer_norm(ops, C, tokens):
    bs = 2
    x, g, b, pos = _rand(C + tokens, bs, C, tokens, std=1.5, mean=0.3), _rand(C, C, std=0.2, mean=1.0), _rand(C + 1, C, std=0.3), _rand(C + 2, C, tokens, std=0.5)
    y = ops.layer_norm_cm(x.to(DEV), g.to(DEV), b.to(DEV))
    y2, yp = ops.layer_norm_cm(x.to(DEV), g.to(DEV), b.to(DEV), pos=pos.to(DEV))
    assert torch.equal(y, y2) and y.shape == x.shape == yp.shape
    want = M.layer_norm_cm(x.double(), g.double(), b.double())
    want32 = M.layer_norm_cm(x, g, b)
    _check(f"cf_layer_norm.{C}x{tokens}", y, want, want32)
    _check(f"cf_layer_norm.{C}x{tokens}.pos", yp, want + pos.double(), want32 + pos)


# ------------------------------------------------------------------------------------------------ head, codes, gather, AdaIN
@pytest.mark.parametrize("bs,E,K,hw", [(2, 64, 40, (2, 3)), (1, 512, 1024, (16, 16))], ids=["CF-S-sizes", "T256-K1024"])
def test_head_codes_gather_adain(ops, bs, E, K, hw):
    from e4s2024_amd import ops_codeformer as OC
    from e4s2024_amd.lossnet import conv_exact, prep_exact
    h, w = hw
    tokens = h * w
    t, g, b = _rand(E + K, bs, E, tokens, std=1.3), _rand(E, E, std=0.2, mean=1.0), _rand(E + 1, E, std=0.2)
    W = _rand(K, K, E, std=4.0 / np.sqrt(E))
    emb, lq = _rand(K + 1, K, 256), _rand(K + 2, bs, 256, h, w, std=0.9, mean=0.2)
    emb[:, 5] = 0.75                                  # a channel whose values are all equal: variance 0, eps alone divides
    ln = ops.layer_norm_cm(t.to(DEV), g.to(DEV), b.to(DEV))
    cm = conv_exact(ln.view(bs, E, h, w), prep_exact(W.view(K, E, 1, 1).to(DEV))[0], None, k=1)
    logits = cm.view(bs, K, tokens).transpose(1, 2)
    lin = lambda x, wt: torch.einsum("oc,bct->bto", wt, x)                                    # noqa: E731
    want = lin(M.layer_norm_cm(t.double(), g.double(), b.double()), W.double())
    want32 = lin(M.layer_norm_cm(t, g, b), W)
    _check(f"cf_head.logits.{E}x{K}x{tokens}", logits, want, want32)
    idx = ops.codeformer_codes(logits)
    assert idx.dtype == torch.int64 and idx.shape == (bs, tokens)
    assert torch.equal(idx, ops.codeformer_codes(logits.contiguous()))
    top = want.topk(2, dim=2)[0]
    close = T(M.close_tokens(top[..., 0].numpy(), top[..., 1].numpy(), _err(want32, want)))
    print(f"cf_head.codes: {int(close.sum())} close of {close.numel()} tokens")
    assert close.sum() <= M.CLOSE_SHARE * close.numel()
    assert torch.equal(idx.cpu()[~close], want.argmax(2)[~close])
    assert len(idx.unique()) > 1
    # an exact tie goes to the lower index, in both layouts
    tie = logits.contiguous().clone()
    tie[:, :, 3] = tie[:, :, K - 2] = tie.max() + 1
    assert bool((ops.codeformer_codes(tie) == 3).all()) and bool((ops.codeformer_codes(tie.transpose(1, 2).contiguous().transpose(1, 2)) == 3).all())
    # gather and AdaIN on the device's own codes
    q = OC._quant(idx, lq.to(DEV), emb.to(DEV), True)
    plain = OC._quant(idx, lq.to(DEV), emb.to(DEV), False)
    quant = emb[idx.cpu().reshape(-1)].reshape(bs, h, w, 256).permute(0, 3, 1, 2)
    assert torch.equal(plain.cpu(), quant)
    _check(f"cf_quant.adain.{tokens}", q, M.adain(quant.double(), lq.double()), M.adain(quant, lq))
    assert bool(torch.isfinite(q).all()) and bool((q[:, 5] == q[:, 5, :1, :1]).all())        # the constant channel comes out as the style's mean, a constant


# ------------------------------------------------------------------------------------------------ end to end
_FRONTS = {}


def _front(ops, tag):
    if tag not in _FRONTS:
        _FRONTS[tag] = ops.codeformer_front(T(M.case_input(tag)).to(DEV), _net(ops, tag))
    return _FRONTS[tag]


@pytest.mark.parametrize("tag", list(M.CASES))
def test_front_against_the_fixture(ops, golden, tag):
    E, n_head, n_layers, K, tokens = M.CASES[tag]["cfg"]
    n = M.CASES[tag]["shape"][0]
    f = _front(ops, tag)
    assert f["logits"].shape == (n, tokens, K) and f["idx"].shape == (n, tokens) and f["quant_feat"].shape == f["lq_feat"].shape == (n, 256) + f["lq_feat"].shape[2:]
    assert set(f["taps"]) == set(M.CONNECT)
    close = M.close_tokens(golden[f"{tag}.top1"], golden[f"{tag}.top2"], golden[f"{tag}.e32.logits"])
    print(f"{tag}: {int(close.sum())} close of {close.size} tokens")
    assert close.sum() <= M.CLOSE_SHARE * close.size
    got = dict(lq_feat=f["lq_feat"], logits=f["logits"], quant_feat=f["quant_feat"], **{"tap" + s: f["taps"][s] for s in M.CONNECT})
    worst = {}
    for name in M.NAMES:
        want, e32 = golden[f"{tag}.m.{name}"].astype(np.float64), float(golden[f"{tag}.e32.{name}"])
        have = M.stored(tag, name, got[name].cpu().numpy())
        assert have.shape == want.shape, (name, have.shape, want.shape)
        diff = np.abs(have.astype(np.float64) - want)
        if name == "quant_feat":                      # on the tokens whose code was compared
            stride = int(golden[f"{tag}.stride.{name}"])
            flat = np.arange(have.size) * stride if stride > 1 else np.arange(have.size)
            keep = ~close.reshape(-1)[(flat // (256 * tokens)) * tokens + flat % tokens]
            diff = diff.reshape(-1)[keep]
        err = float(diff.max())
        worst[name] = err / e32
        record_parity(f"cf_front.{tag}.{name}", err, 4 * e32)
        print(f"{tag}.{name}: err {err:.3e}, e32 {e32:.3e}, err / e32 {err / e32:.2f}")
    idx = f["idx"].cpu().numpy()
    assert (idx == golden[f"{tag}.ref_idx"])[~close].all()
    assert all(v <= 4 for v in worst.values()), worst


def test_front_reproducible_and_capturable(ops):
    tag = "CF-S"
    net, x = _net(ops, tag), T(M.case_input(tag)).to(DEV)
    eager = _front(ops, tag)
    flat = lambda f: [f["quant_feat"], f["logits"], f["lq_feat"], f["idx"]] + [f["taps"][s] for s in M.CONNECT]   # noqa: E731
    again = ops.codeformer_front(x, net)
    assert all(torch.equal(a, b) for a, b in zip(flat(again), flat(eager)))
    for i in range(x.shape[0]):                       # a sample of the batch gets the bits it gets alone
        alone = ops.codeformer_front(x[i:i + 1].contiguous(), net)
        assert all(torch.equal(a, b[i:i + 1]) for a, b in zip(flat(alone), flat(eager)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.codeformer_front(x, net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                     # single stream: no parallel branches
        out = ops.codeformer_front(x, net)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(flat(out), flat(eager)))


def test_taps_are_not_aliased_and_the_parts_compose(ops):
    tag = "CF-S"
    net, x = _net(ops, tag), T(M.case_input(tag)).to(DEV)
    full = _front(ops, tag)
    lq, taps = ops.codeformer_encode(x, net)
    kept = {s: t.clone() for s, t in taps.items()}
    logits = ops.codeformer_logits(lq, net)
    idx = ops.codeformer_codes(logits)
    quant = ops.codeformer_quant(idx, lq, net, adain=True)
    torch.cuda.synchronize()
    assert all(torch.equal(taps[s], kept[s]) and torch.equal(taps[s], full["taps"][s]) for s in M.CONNECT)      # compared after the whole front has run
    assert len({t.data_ptr() for t in list(taps.values()) + [lq, quant]}) == 6
    assert torch.equal(lq, full["lq_feat"]) and torch.equal(logits, full["logits"]) and torch.equal(idx, full["idx"]) and torch.equal(quant, full["quant_feat"])
    plain = ops.codeformer_quant(idx, lq, net, adain=False)
    assert torch.equal(plain.flatten(2).transpose(1, 2), net.quantize.embedding.weight[idx.reshape(-1)].view(idx.shape + (256,)))


def test_pipeline_codeformer_front(ops):
    from e4s2024_amd import pipeline
    tag = "CF-F"
    net = _net(ops, tag)
    u8 = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(1, 3, 512, 512), dtype=np.uint8)).to(DEV)
    got = pipeline.codeformer_front(net, u8)
    want = ops.codeformer_front(((u8.float() / 255.0) - 0.5) / 0.5, net)
    assert torch.equal(got["quant_feat"], want["quant_feat"]) and torch.equal(got["idx"], want["idx"]) and got["quant_feat"].shape == (1, 256, 16, 16)
