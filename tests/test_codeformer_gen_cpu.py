"""Row f22 (CodeFormer, stage 2: the generator and its SFT fusion) without a GPU: the entry points as the header declares them, the names the row adds, the
documents that name it, the redirect table it leaves alone, the float64 model against the fixture and the mirror module against the model, the fixture's
conditions on the seeded decoder stream, every refusal before any launch, the mutants of the model, and the stage-1 weights the new seeded rule leaves alone."""
import os
import re

import numpy as np
import pytest
import torch

import codeformer_gen_model as G
import codeformer_model as M
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_cf_sft": 8, "e4s_cf_image_u8": 4}
NAMES = ("PreparedCodeFormerGenerator", "GENERATOR_PLAN", "CF_FUSE_BLOCKS", "sft_fuse", "image_u8", "codeformer_fuse", "codeformer_generate", "codeformer_restore")
SMALL = ("CF-S", "CF-T")


@pytest.fixture(scope="module")
def golden():
    return load_golden("g32_codeformer_gen")


_MADE = {}


def _case(golden, tag):
    """(mirror module with the case's seeded weights, input, weights, the float64 front on the fixture's codes, the float64 generator's outputs) of a small
    case, made once."""
    if tag not in _MADE:
        from e4s2024_amd import ops
        sd, x = M.case_weights(tag), M.case_input(tag)
        net = ops.CodeFormer(*M.CASES[tag]["cfg"]).eval()
        net.load_state_dict(sd, strict=True)
        front = M.front(sd, x, M.CASES[tag]["cfg"], idx=golden[f"{tag}.ref_idx"])
        m64 = G.generate(sd, front)
        m64["out_w0"] = G.generate(sd, front, w=0)["out"]
        _MADE[tag] = (net, x, sd, front, m64)
    return _MADE[tag]


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert {n: len(_lib._PROTOS[n]) for n in ENTRY_POINTS} == ENTRY_POINTS
    assert "/* f22:" in src and _lib.ABI_VERSION == 1
    cdll = _lib.lib().cdll
    assert all(hasattr(cdll, name) for name in ENTRY_POINTS)


def test_names_documents_and_the_redirect_table():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_codeformer, ops_codeformer_gen, pipeline
    for name in NAMES:
        assert name in ops_codeformer_gen.__all__ and getattr(ops, name) is getattr(ops_codeformer_gen, name), name
    assert callable(pipeline.codeformer_restore)
    assert ops.GENERATOR_PLAN == tuple(ops_codeformer._plan(True)) == tuple(G.generator_plan()) and len(ops.GENERATOR_PLAN) == 25
    assert {b: s for s, b in ops.CF_FUSE_BLOCKS.items()} == G.FUSE_BLOCKS == {b: s for s, b in ops.CodeFormer(64, 2, 1, 40, 6).fuse_generator_block.items() if s in M.CONNECT}
    for s, b in ops.CF_FUSE_BLOCKS.items():                                                   # the fuse block follows a ResBlock that ends at its channel count
        assert ops.GENERATOR_PLAN[b][0] == "res" and ops.GENERATOR_PLAN[b][2] == ops_codeformer.CF_CHANNELS[s] == G.CHANNELS[s]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "SURVEY.md"):
        assert re.search(r"\bf22\b", open(os.path.join(ROOT, doc)).read()), doc
    assert "## 4n." in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = e4s2024_amd._redirected()                                                         # no drop-in in this stage either: the table is the parent's
    assert len(table) == 30 and not any("codeformer" in m or ".archs" in m for m in table)
    assert not os.path.exists(os.path.join(ROOT, "e4s2024_amd", "dropin", "swap_face_fine", "archs"))
    assert not re.search(r"^\s*(from|import)\s+basicsr", open(ops_codeformer_gen.__file__).read(), flags=re.M)


@pytest.mark.parametrize("tag", SMALL)
def test_model_equals_the_fixture_and_the_module_the_model(golden, tag):
    """The bar on the mirror module is 4 e32, the project's device bar, not stage 1's 2: ``e32`` is the reference's error on the CPU that made the fixture, and
    the module's float32 forward runs on whatever host runs the suite (the stage-1 test's docstring records up to 2.15 e32 for identical code on another host)."""
    net, x, sd, front, m64 = _case(golden, tag)
    for name in G.NAMES + ("out_w0",):
        want = golden[f"{tag}.m.{name}"]
        have = M.stored(tag, name, m64[name].numpy())
        assert have.shape == want.shape and int(golden[f"{tag}.stride.{name}"]) == M.sample_stride(m64[name].numel()), (name, have.shape, want.shape)
        assert np.abs(have - want.astype(np.float64)).max() <= 2.0 ** -22 * np.abs(want).max(), name
    got, hooks = {}, []
    for s in M.CONNECT:
        hooks.append(net.fuse_convs_dict[s].register_forward_hook(lambda m, i, o, s=s: got.__setitem__("dec" + s, o)))
    with torch.no_grad():
        got["out"], logits, lq = net(T(x), w=G.W, adain=True)
        for h in hooks:
            h.remove()
        got["out_w0"] = net(T(x), w=0, adain=True)[0]
        idx = net.front(T(x))["idx"]
    assert np.array_equal(idx.numpy(), golden[f"{tag}.ref_idx"])                              # the small cases have no close tokens
    n, _, H, W = x.shape
    assert got["out"].shape == got["out_w0"].shape == (n, 3, H, W) and logits.shape[:2] == (n, M.CASES[tag]["cfg"][4]) and lq.shape == (n, 256, H // 32, W // 32)
    worst = {}
    for name in G.NAMES + ("out_w0",):
        e32 = float(golden[f"{tag}.e32.{name}"])
        err = float((got[name].double() - m64[name]).abs().max())
        worst[name] = err / e32
        print(f"{tag}.{name}: module err {err:.3e}, e32 {e32:.3e}, err / e32 {err / e32:.2f}")
    assert all(v <= 4 for v in worst.values()), worst


def test_conditions_on_the_seeded_decoder_stream(golden):
    for tag in M.CASES:
        growth, ratio, inside = golden[f"{tag}.growth"], golden[f"{tag}.term_ratio"], float(golden[f"{tag}.inside"])
        print(f"{tag}: growth {np.round(growth, 3)}, term / dec {np.round(ratio, 3)}, inside {inside:.3f}")
        assert growth.shape == ratio.shape == (4,)
        assert np.allclose(growth, golden[f"{tag}.after_std"] / golden[f"{tag}.before_std"], rtol=1e-12)
        assert growth.max() <= 2 and ratio.min() >= 0.1 and 0.2 <= inside <= 0.95, tag
        names = G.NAMES + (("out_w0",) if tag in SMALL else ())
        assert all(float(golden[f"{tag}.e32.{name}"]) > 0 for name in names)
        assert f"{tag}.e32.out_w0" in golden.files if tag in SMALL else f"{tag}.e32.out_w0" not in golden.files
        assert golden[f"{tag}.ref_idx"].shape == (M.CASES[tag]["shape"][0], M.CASES[tag]["cfg"][4])
    assert golden["CF-F.m.out"].shape == golden["CF-F.m.dec256"].shape == (M.SAMPLES,)
    assert not any("weight" in k or "bias" in k for k in golden.files)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g32_codeformer_gen.npz")) < 1_000_000


def test_refusals_before_any_launch(golden):
    from e4s2024_amd import ops, pipeline
    net, x, sd, front64, _ = _case(golden, "CF-S")
    x = T(x)
    n, h, w = x.shape[0], x.shape[2] // 32, x.shape[3] // 32
    front = dict(quant_feat=front64["quant_feat"].float(), taps={s: front64["tap" + s].float() for s in M.CONNECT})
    gen = lambda f=front, net=net, **k: ops.codeformer_generate(f, net, **k)                  # noqa: E731
    u8 = torch.zeros(1, 3, 512, 512, dtype=torch.uint8)
    full = ops.CodeFormer(64, 2, 1, 40, 256).eval()
    enc, dec = front["taps"]["32"], torch.zeros(n, 256, 2 * h, 2 * w)
    net.train()
    try:
        for call in (gen, lambda: ops.codeformer_restore(x, net), lambda: ops.codeformer_fuse(enc, dec, net, "32", 0.8)):
            with pytest.raises(RuntimeError, match="training mode"):
                call()
    finally:
        net.eval()
    full.train()
    with pytest.raises(RuntimeError, match="training mode"):
        pipeline.codeformer_restore(full, u8)
    full.eval()
    # w
    for call in (lambda w: gen(w=w), lambda w: ops.codeformer_restore(x, net, w=w), lambda w: ops.codeformer_fuse(enc, dec, net, "32", w),
                 lambda w: ops.sft_fuse(dec, dec, dec, w), lambda w: pipeline.codeformer_restore(full, u8, w=w)):
        for bad in (torch.tensor(0.8), np.float32(0.8), "0.8", None, True):
            with pytest.raises(TypeError, match="Python real"):
                call(bad)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                call(bad)
    # front
    with pytest.raises(TypeError, match="codeformer_front returns"):
        gen(f=front["quant_feat"])
    with pytest.raises(TypeError, match="codeformer_front returns"):
        gen(f=dict(taps=front["taps"]))
    other = lambda **k: dict(front, **k)                                                      # noqa: E731
    with pytest.raises(ValueError, match="float32"):
        gen(f=other(quant_feat=front["quant_feat"].double()))
    with pytest.raises(ValueError, match=r"\[n, 256, h, w\]"):
        gen(f=other(quant_feat=front["quant_feat"][:, :255]))
    with pytest.raises(ValueError, match=r"\[n, 256, h, w\]"):
        gen(f=other(quant_feat=front["quant_feat"][0]))
    with pytest.raises(ValueError, match="at most 1024"):
        gen(f=other(quant_feat=torch.zeros(1, 256, 1, 1).expand(1, 256, 33, 32)), w=0)
    with pytest.raises(ValueError, match="bs C <= 65535"):
        gen(f=other(quant_feat=torch.zeros(1, 256, 1, 1).expand(128, 256, h, w)), w=0)
    with pytest.raises(ValueError, match="bs C <= 65535"):
        ops.codeformer_restore(x[:1].expand(128, 3, 64, 96), net)
    with pytest.raises(ValueError, match="bs C <= 65535"):
        ops.codeformer_fuse(torch.zeros(1, 1, 1, 1).expand(256, 256, 2, 2), torch.zeros(1, 1, 1, 1).expand(256, 256, 2, 2), net, "32", 0.8)
    with pytest.raises(ValueError, match="at most 127 faces"):
        pipeline.codeformer_restore(full, u8.expand(128, 3, 512, 512))
    # taps, read with w > 0 only
    less = lambda s: {k: v for k, v in front["taps"].items() if k != s}                       # noqa: E731
    with pytest.raises(KeyError, match="lacks '64'"):
        gen(f=other(taps=less("64")))
    with pytest.raises(KeyError, match="lacks '32'"):
        gen(f=dict(quant_feat=front["quant_feat"]))
    with pytest.raises(ValueError, match=r"taps\['128'\].*float32"):
        gen(f=other(taps=dict(front["taps"], **{"128": front["taps"]["128"].double()})))
    with pytest.raises(ValueError, match=rf"taps\['256'\].*\[{n}, 128, {16 * h}, {16 * w}\]"):
        gen(f=other(taps=dict(front["taps"], **{"256": front["taps"]["256"][:, :, :-1]})))
    with pytest.raises(ValueError, match=rf"taps\['32'\].*\[{n}, 256, {2 * h}, {2 * w}\]"):
        gen(f=other(taps=dict(front["taps"], **{"32": front["taps"]["64"]})))
    with pytest.raises(RuntimeError, match=r"device mismatch: taps\['64'\] on meta"):
        gen(f=other(taps=dict(front["taps"], **{"64": front["taps"]["64"].to("meta")})))
    # one fuse block
    with pytest.raises(ValueError, match="size '512' is not in the connect_list"):
        ops.codeformer_fuse(enc, dec, net, "512", 0.8)
    with pytest.raises(ValueError, match="size '64' is not in the connect_list"):
        ops.codeformer_fuse(enc, dec, ops.CodeFormer(64, 2, 1, 40, 6, connect_list=["32"]).eval(), "64", 0.8)
    with pytest.raises(ValueError, match=r"dec_feat.*\[n, 128, h, w\]"):
        ops.codeformer_fuse(enc, dec, net, "128", 0.8)
    with pytest.raises(ValueError, match="enc_feat"):
        ops.codeformer_fuse(enc[:, :, :-1], dec, net, "32", 0.8)
    with pytest.raises(ValueError, match="float32"):
        ops.codeformer_fuse(enc.double(), dec, net, "32", 0.8)
    # the kernels alone, restore's image, the pipeline's faces
    with pytest.raises(ValueError, match="scale is"):
        ops.sft_fuse(dec, dec[:, :8], dec, 0.8)
    with pytest.raises(ValueError, match="float32"):
        ops.sft_fuse(dec, dec, dec.half(), 0.8)
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.sft_fuse(dec.numpy(), dec, dec, 0.8)
    with pytest.raises(ValueError, match=r"\[n, 3, H, W\]"):
        ops.image_u8(torch.zeros(1, 4, 8, 8))
    with pytest.raises(ValueError, match="float32"):
        ops.image_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.codeformer_restore(x[:, :, :, :80], net)
    with pytest.raises(ValueError, match="latent_size = 6"):
        ops.codeformer_restore(x[:, :, :, :64], net)
    with pytest.raises(ValueError, match="uint8"):
        pipeline.codeformer_restore(full, u8.float())
    with pytest.raises(TypeError, match="mapping"):
        gen(net=3)
    # everything accepted gets as far as the placement check, the last refusal
    for call in (gen, lambda: gen(w=1), lambda: gen(w=0), lambda: gen(f=dict(quant_feat=front["quant_feat"]), w=0), lambda: gen(f=dict(quant_feat=front["quant_feat"]), w=-1.5),
                 lambda: gen(return_feats=True), lambda: ops.codeformer_restore(x, net), lambda: ops.codeformer_restore(x, net, w=0, adain=False),
                 lambda: ops.codeformer_fuse(enc, dec, net, "32", 0.8), lambda: ops.codeformer_fuse(enc, dec, net, "64", 0), lambda: ops.sft_fuse(dec, dec, dec, 0.8),
                 lambda: ops.image_u8(x), lambda: pipeline.codeformer_restore(full, u8), lambda: pipeline.codeformer_restore(full, u8[:, :, :64, :64], w=0)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()


def test_mutants_move_the_outputs(golden):
    tag = "CF-S"
    _, x, sd, front, m64 = _case(golden, tag)
    where = {"sft_no_product": "out", "cat_dec_first": "out", "fuse_one_block_early": "out", "up_after_conv": "out", "leaky_as_relu": "out", "w_ignored": "out"}
    assert set(where) == set(G.MUTANTS)
    for mutant, name in where.items():
        got = G.generate(sd, front, mutant=mutant)
        bars = float((got[name] - m64[name]).abs().max()) / float(golden[f"{tag}.e32.{name}"])
        print(f"mutant {mutant} moves {tag}.{name} by {bars:.0f} e32")
        assert bars > 16, (mutant, bars)
    u8 = G.image_u8(np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 3.0], dtype=np.float32))
    assert u8.dtype == np.uint8 and u8.tolist() == [0, 0, 64, 128, 191, 255, 255]             # 63.75 -> 64; 127.5 -> 128, half to even; 191.25 -> 191


def test_the_new_seeded_rule_leaves_every_other_key_alone():
    from e4s2024_amd import seeded
    seed = 211
    sd = seeded.seeded_codeformer_state_dict(seed, 64, 2, 2, 40, 6)
    fan = lambda k, gain: seeded.seeded_array(seed, k, tuple(sd[k].shape), 0.0, gain / np.sqrt(np.prod(sd[k].shape[1:])))    # noqa: E731
    flat = lambda k, mean, std: seeded.seeded_array(seed, k, tuple(sd[k].shape), mean, std)                                   # noqa: E731
    old = {"encoder.blocks.0.weight": fan("encoder.blocks.0.weight", 1.2), "encoder.blocks.0.bias": flat("encoder.blocks.0.bias", 0.0, 0.1),
           "encoder.blocks.1.norm1.weight": flat("encoder.blocks.1.norm1.weight", 1.0, 0.2), "encoder.blocks.14.conv2.weight": fan("encoder.blocks.14.conv2.weight", 1.2),
           "ft_layers.1.self_attn.in_proj_weight": fan("ft_layers.1.self_attn.in_proj_weight", 1.0), "ft_layers.0.linear2.weight": fan("ft_layers.0.linear2.weight", 1.2),
           "idx_pred_layer.1.weight": fan("idx_pred_layer.1.weight", 4.0), "quantize.embedding.weight": flat("quantize.embedding.weight", 0.0, 1.0),
           "position_emb": flat("position_emb", 0.0, 0.5), "feat_emb.bias": flat("feat_emb.bias", 0.0, 0.1),
           # the generator's keys and the fuse blocks' other keys too
           "generator.blocks.24.weight": fan("generator.blocks.24.weight", 1.2), "fuse_convs_dict.32.scale.0.weight": fan("fuse_convs_dict.32.scale.0.weight", 1.2),
           "fuse_convs_dict.256.shift.0.bias": flat("fuse_convs_dict.256.shift.0.bias", 0.0, 0.1),
           "fuse_convs_dict.64.encode_enc.conv_out.weight": fan("fuse_convs_dict.64.encode_enc.conv_out.weight", 1.2)}
    for k, want in old.items():
        assert np.array_equal(sd[k].numpy(), np.asarray(want, dtype=np.float32).reshape(sd[k].shape)), k
    for s in M.CONNECT:
        for b in ("scale", "shift"):
            k = f"fuse_convs_dict.{s}.{b}.2."
            assert np.array_equal(sd[k + "weight"].numpy(), fan(k + "weight", 1.2 * 0.1).reshape(sd[k + "weight"].shape))
            assert np.array_equal(sd[k + "bias"].numpy(), flat(k + "bias", 0.0, 0.1 * 0.1))
            assert 0.08 < float(sd[k + "weight"].std() / fan(k + "weight", 1.2).std()) < 0.12
