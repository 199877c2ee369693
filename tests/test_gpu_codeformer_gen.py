"""Row f22 on the GPU: the two kernels of csrc/codeformer_gen.hip bit for bit against their float32 statements, one ``Fuse_sft_block`` against the float64 model
(the bar of every comparison is ``4 e32``, ``e32`` the float32 restatement's own distance from float64 on the same input), then ``codeformer_generate`` on the
three cases of tests/golden/g32_codeformer_gen.npz against the float64 model's stored outputs under ``4 e32.<name>`` (the reference's own float32 error), with
the per-block features that locate a miss, its bit-for-bit properties, its capture in a graph, and the compositions ``codeformer_restore`` and
``pipeline.codeformer_restore``.  Every figure is printed and recorded before it is asserted."""
import numpy as np
import pytest
import torch

import codeformer_gen_model as G
import codeformer_model as M
from conftest import load_golden, record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
SMALL = ("CF-S", "CF-T")


@pytest.fixture(scope="module")
def golden():
    return load_golden("g32_codeformer_gen")


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


# ------------------------------------------------------------------------------------------------ the SFT kernel
@pytest.mark.parametrize("w", [0.8, 1.0, 0.0])
@pytest.mark.parametrize("shape", [(1, 32, 1, 1), (2, 32, 5, 7), (1, 128, 16, 24)], ids=lambda v: "x".join(map(str, v)))
def test_sft_fuse_bits(ops, shape, w):
    dec, scale, shift = _rand(sum(shape), *shape, std=3.0), _rand(sum(shape) + 1, *shape, std=0.7), _rand(sum(shape) + 2, *shape, std=1.5, mean=0.1)
    want = dec + w * (dec * scale + shift)                                                    # float32 on the CPU, one rounding per operation
    got = ops.sft_fuse(dec.to(DEV), scale.to(DEV), shift.to(DEV), w)
    assert got.shape == dec.shape and got.dtype == torch.float32
    diff = _err(got, want)
    record_parity(f"cf_sft.{'x'.join(map(str, shape))}.w{w:g}", diff, 0.0)
    print(f"cf_sft {shape} w {w:g}: max abs difference from the float32 expression {diff:.3e}")
    assert torch.equal(got.cpu(), want)
    if w == 0.0:
        assert torch.equal(got.cpu(), dec)
    # a view that is not contiguous is taken as its values; an offset view (4-byte aligned only) takes the scalar path with the same bits
    big = torch.cat([dec, scale, shift], 1).to(DEV)
    C = shape[1]
    assert torch.equal(ops.sft_fuse(big[:, :C], big[:, C:2 * C], big[:, 2 * C:], w), got)
    flat = torch.cat([dec.reshape(-1), scale.reshape(-1), shift.reshape(-1)]).to(DEV)
    off = torch.zeros(flat.numel() + 1, device=DEV)
    off[1:] = flat
    n = dec.numel()
    assert torch.equal(ops.sft_fuse(*(off[1 + i * n:1 + (i + 1) * n].view(shape) for i in range(3)), w), got)
    # a sample of the batch gets the bits it gets alone
    assert torch.equal(ops.sft_fuse(dec[-1:].to(DEV), scale[-1:].to(DEV), shift[-1:].to(DEV), w), got[-1:])
    assert ops.sft_fuse(dec[:0].to(DEV), scale[:0].to(DEV), shift[:0].to(DEV), w).shape == (0,) + shape[1:]


# ------------------------------------------------------------------------------------------------ the uint8 tail
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 64, 96)], ids=lambda v: "x".join(map(str, v)))
def test_image_u8_bits(ops, shape):
    x = (np.random.RandomState(sum(shape)).standard_normal(shape) * 1.2).astype(np.float32)
    flat = x.reshape(-1)
    edges = np.array([np.float32(-1 + (2 * k + 1) / 255) for k in range(255)], dtype=np.float32)          # nearest each rounding boundary k + 0.5
    ends = np.array([-1.0, 1.0, -1.5, 1.5, -7.0, 9.0, 0.0, -0.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(-1), np.float32(0))], dtype=np.float32)
    near = np.concatenate([edges, np.nextafter(edges, np.float32(2)), np.nextafter(edges, np.float32(-2))])
    room = flat.size // 2 - ends.size
    special = np.concatenate([ends, near[:: -(-near.size // room)] if near.size > room else near])              # the small shape takes every k-th boundary value
    flat[:special.size] = special
    assert np.isfinite(x).all() and (np.abs(x) > 1).any() and (x == 1).any() and (x == -1).any()
    want = G.image_u8(x)
    got = ops.image_u8(T(x).to(DEV))
    assert got.dtype == torch.uint8 and got.shape == shape
    diff = int(np.abs(got.cpu().numpy().astype(np.int32) - want.astype(np.int32)).max())
    record_parity(f"cf_image_u8.{'x'.join(map(str, shape))}", float(diff), 0.0)
    print(f"cf_image_u8 {shape}: max abs difference from the float32 formula {diff}, values {want.min()} .. {want.max()}, {len(np.unique(want))} distinct")
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.min() == 0 and want.max() == 255
    if flat.size >= 3 * 255:
        assert len(np.unique(want)) == 256
    assert torch.equal(ops.image_u8(T(x).to(DEV)[-1:]), got[-1:])
    assert ops.image_u8(T(x).to(DEV)[:0]).shape == (0,) + shape[1:]


# ------------------------------------------------------------------------------------------------ one fuse block
@pytest.mark.parametrize("size,shape", [("32", (2, 256, 3, 5)), ("256", (1, 128, 6, 10))], ids=["32", "256"])
def test_fuse_block_against_float64(ops, size, shape):
    tag = "CF-S"
    net, sd = _net(ops, tag), M.case_weights(tag)
    enc, dec = _rand(int(size), *shape, std=1.4, mean=0.2), _rand(int(size) + 1, *shape, std=2.0)
    P64 = {k: v.double() for k, v in sd.items() if k.startswith("fuse_convs_dict.")}
    want, want32 = G.fuse(P64, size, enc.double(), dec.double(), G.W), G.fuse({k: v for k, v in sd.items() if k.startswith("fuse_convs_dict.")}, size, enc, dec, G.W)
    got = ops.codeformer_fuse(enc.to(DEV), dec.to(DEV), net, size, G.W)
    assert got.shape == shape and got.dtype == torch.float32
    _check(f"cf_fuse.{size}.{'x'.join(map(str, shape))}", got, want, want32)
    assert float((want - dec.double()).abs().max()) > 64 * _err(want32, want)                 # the block does something
    assert torch.equal(ops.codeformer_fuse(enc.to(DEV), dec.to(DEV), net, size, 0).cpu(), dec)
    assert torch.equal(ops.codeformer_fuse(enc[-1:].to(DEV), dec[-1:].to(DEV), net, size, G.W), got[-1:])


# ------------------------------------------------------------------------------------------------ the generator
_FRONTS = {}


def _front(ops, golden, tag):
    """The device's front with ``quant_feat`` looked up on the fixture's reference codes: a close token can neither cause nor hide a failure."""
    if tag not in _FRONTS:
        net = _net(ops, tag)
        f = dict(ops.codeformer_front(T(M.case_input(tag)).to(DEV), net))
        f["quant_feat"] = ops.codeformer_quant(T(golden[f"{tag}.ref_idx"]).to(DEV), f["lq_feat"], net, adain=True)
        _FRONTS[tag] = f
    return _FRONTS[tag]


def _flat(out, feats):
    return [out] + [feats[s] for s in M.CONNECT]


@pytest.mark.parametrize("tag", list(M.CASES))
def test_generate_against_the_fixture(ops, golden, tag):
    n, _, H, W = M.CASES[tag]["shape"]
    net, f = _net(ops, tag), _front(ops, golden, tag)
    out, feats = ops.codeformer_generate(f, net, w=G.W, return_feats=True)
    assert out.shape == (n, 3, H, W) and out.dtype == torch.float32 and list(feats) == list(M.CONNECT)
    for k, s in enumerate(M.CONNECT, 1):
        assert feats[s].shape == (n, G.CHANNELS[s], (H // 32) << k, (W // 32) << k)
    got = dict(out=out, **{"dec" + s: feats[s] for s in M.CONNECT})
    if tag in SMALL:
        got["out_w0"] = ops.codeformer_generate(f, net, w=0)
        assert torch.equal(ops.codeformer_generate(dict(quant_feat=f["quant_feat"]), net, w=0), got["out_w0"])        # no tap is read at w <= 0
        assert torch.equal(ops.codeformer_generate(dict(quant_feat=f["quant_feat"]), net, w=-1.0), got["out_w0"])
    worst = {}
    for name, have in got.items():
        want, e32 = golden[f"{tag}.m.{name}"].astype(np.float64), float(golden[f"{tag}.e32.{name}"])
        have = M.stored(tag, name, have.cpu().numpy())
        assert have.shape == want.shape, (name, have.shape, want.shape)
        err = float(np.abs(have.astype(np.float64) - want).max())
        worst[name] = err / e32
        record_parity(f"cf_generate.{tag}.{name}", err, 4 * e32)
        print(f"{tag}.{name}: err {err:.3e}, e32 {e32:.3e}, err / e32 {err / e32:.2f}")
    assert all(v <= 4 for v in worst.values()), worst


def test_generate_reproducible_and_capturable(ops, golden):
    tag = "CF-S"
    net, f = _net(ops, tag), _front(ops, golden, tag)
    eager = _flat(*ops.codeformer_generate(f, net, return_feats=True))
    assert all(torch.equal(a, b) for a, b in zip(_flat(*ops.codeformer_generate(f, net, return_feats=True)), eager))
    for i in range(f["quant_feat"].shape[0]):         # a sample of the batch gets the bits it gets alone
        one = dict(quant_feat=f["quant_feat"][i:i + 1].contiguous(), taps={s: t[i:i + 1].contiguous() for s, t in f["taps"].items()})
        assert all(torch.equal(a, b[i:i + 1]) for a, b in zip(_flat(*ops.codeformer_generate(one, net, return_feats=True)), eager))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.codeformer_generate(f, net)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                     # single stream: no parallel branches
        out = _flat(*ops.codeformer_generate(f, net, return_feats=True))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_restore_composes(ops):
    tag = "CF-S"
    net, x = _net(ops, tag), T(M.case_input(tag)).to(DEV)
    f = ops.codeformer_front(x, net)
    out, logits, lq = ops.codeformer_restore(x, net, w=G.W, adain=True)
    assert torch.equal(out, ops.codeformer_generate(f, net, w=G.W)) and torch.equal(logits, f["logits"]) and torch.equal(lq, f["lq_feat"])
    plain = ops.codeformer_restore(x, net, w=0, adain=False)
    assert torch.equal(plain[0], ops.codeformer_generate(ops.codeformer_front(x, net, adain=False), net, w=0)) and torch.equal(plain[1], logits)
    assert not torch.equal(plain[0], out)


def test_pipeline_codeformer_restore(ops):
    from e4s2024_amd import pipeline
    tag = "CF-F"
    net = _net(ops, tag)
    u8 = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(1, 3, 512, 512), dtype=np.uint8)).to(DEV)
    got = pipeline.codeformer_restore(net, u8, w=G.W)
    want = ops.image_u8(ops.codeformer_restore(((u8.float() / 255.0) - 0.5) / 0.5, net, w=G.W, adain=True)[0])
    assert got.dtype == torch.uint8 and got.shape == (1, 3, 512, 512) and torch.equal(got, want)
    assert 8 < len(got.unique())
