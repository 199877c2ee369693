"""Row f19 (face-vid2vid's generator in front of its decoder, and the mirror of the whole generator) without a GPU: the reference's stored outputs against the
float64 restatement ``vid2vid_gen_model``, the conditions that keep a pass from being empty, the bars of the GPU tests pinned from the other side by
single-change mutants, the mirror module's keys against the reference's, the mirror on stock PyTorch (the decoder included), the seeded weights, and the
argument errors that must raise before any launch.

The bar of a case and output is ``max(8 e32, 2e-7 max|want|)``, ``e32`` the model in float32 against itself in float64 — never the code under test."""
import numpy as np
import pytest
import torch

import vid2vid_gen_model as M
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_v2v_deform": 11, "e4s_v2v_bn_relu": 8, "e4s_v2v_occlude": 7}
TAGS = list(M.CASES)
UPSTREAM_KEYS, UPSTREAM_PARAMS = 386, 100_988_176
BUFFERS = ("running_mean", "running_var", "num_batches_tracked", "weight_u", "weight_v")


@pytest.fixture(scope="module")
def golden():
    return load_golden("g30_vid2vid_gen")


def _stored(golden, tag):
    return {k: golden[f"{tag}.{k}"] for k in M.OUTPUTS if f"{tag}.{k}" in golden.files}


_NETS = {}


def _net(tag):
    if tag not in _NETS:
        net = M.make_module(tag)
        net.load_state_dict(M.case(tag)["sd"], strict=True)
        _NETS[tag] = net
    return _NETS[tag]


@pytest.mark.parametrize("tag", TAGS)
def test_reference_outputs_lie_within_the_bound_of_the_model(tag, golden):
    c = M.case(tag)
    for k in ("kp_d", "kp_s", "jac_d", "jac_s"):                                              # the same seeded inputs as when the fixture was made
        assert (c[k] is None and f"{tag}.{k}" not in golden.files) or np.array_equal(golden[f"{tag}.{k}"], c[k])
    ref = _stored(golden, tag)
    assert set(ref) == {k for k in M.STORED[tag] if k in c["out64"]}
    assert ("occlusion_map" in c["out64"]) == M.CASES[tag][0]["estimate_occlusion_map"]
    for k, got in ref.items():
        want = c["out64"][k]
        assert got.dtype == np.float32 and got.shape == want.shape
        e = M.max_err(got, want)
        print(f"{tag}.{k}: the reference against the model {e:.3e} = {e / c['e32'][k]:.2f} e32, std {want.std():.3f}")
        assert e <= M.bound(c["e32"][k], want)
    assert not any(f.endswith((".source", ".weight")) for f in golden.files)                  # neither weights nor images are stored


def test_shapes_of_the_cases():
    want = {"G-A": ((2, 8, 4, 8, 8), (2, 32, 8, 8)), "G-B": ((1, 5, 3, 8, 24), (1, 20, 8, 24)), "G-C": ((1, 8, 4, 8, 8), (1, 32, 8, 8)),
            "G-D": ((1, 8, 4, 8, 8), (3, 32, 8, 8)), "G-E": ((1, 32, 4, 8, 8), (1, 256, 8, 8))}
    for tag, (f3, feature) in want.items():
        c = M.case(tag)
        assert c["out64"]["feature_3d"].shape == f3 and c["out64"]["feature"].shape == feature
        n, d, h, w = feature[0], f3[2], f3[3], f3[4]
        assert c["out64"]["deformation"].shape == (n, d, h, w, 3)
        assert ("occlusion_map" not in c["out64"]) or c["out64"]["occlusion_map"].shape == (n, 1, h, w)
    assert M.case("G-E")["out64"]["prediction"].shape == (1, 3, 32, 32) and "prediction" not in M.case("G-A")["out64"]
    assert M.case("G-B")["sd"]["third.conv.weight"].shape == (20, 15, 3, 3)                   # the ragged Cin / Cout
    assert np.array_equal(M.case("G-D")["source"], M.case("G-A")["source"][:1])               # G-D: G-A's first source, three keypoint sets
    assert not any(k.startswith("decoder.") for k in M.case("G-A")["sd"]) and any(k.startswith("decoder.") for k in M.case("G-E")["sd"])


@pytest.mark.parametrize("tag", TAGS)
def test_conditions_that_keep_a_pass_from_being_empty(tag, golden):
    """On the model's outputs and on the reference's stored ones: 5 % .. 50 % of the deformation's sample points outside the volume, every occlusion map over at
    least 0.2 .. 0.8, 20 % .. 80 % zeros behind every norm1 + ReLU, both signs on at least 20 % each in front of third's LeakyReLU, every output well conditioned
    (e32 <= 1e-4 of its deviation) and, for G-E, no plane the instance norm sees with a variance below 1e-3 of its layer's mean."""
    ref_stats = {k: golden[f"{tag}.ref.{k}"] for k in M.REF_STATS if f"{tag}.ref.{k}" in golden.files}      # the reference's own intermediates, from hooks
    assert set(ref_stats) == {"norm1_zero", "third"} | ({"plane_var"} if M.CASES[tag][6] else set())
    print(tag, M.check_conditions(tag, M.case(tag)["out64"]), M.check_conditions(tag, _stored(golden, tag), ref_stats))


def test_every_mutant_is_a_hundred_bars_from_the_fixture_on_its_case(golden):
    assert set(M.MUTANTS) >= {"bn_eps_1e3", "relu_before_norm1", "residual_dropped", "pool_before_relu", "second_bias_missing", "view_depth_channel",
                              "deformation_zyx", "align_corners_true", "border_padding", "output_depth_major", "leaky_slope_02", "relu_in_third",
                              "occlusion_before_fourth", "occlusion_not_applied"}
    assert M.MUTANT_MARGIN == 100.0
    for m, (tag, name) in M.MUTANTS.items():
        c = M.case(tag)
        bars = M.max_err(M.mutant_output(m), golden[f"{tag}.{name}"]) / M.bound(c["e32"][name], c["out64"][name])
        print(f"mutant {m} on {tag}.{name}: {bars:.0f} bars from the fixture")
        assert bars >= M.MUTANT_MARGIN, m


def _want_keys(golden):
    lines = str(golden["keys.gen"]).split("\n")
    return [(ln.split("|")[0], tuple(int(d) for d in ln.split("|")[1].split("x") if d)) for ln in lines]


def test_mirror_has_the_reference_keys_in_order(golden):
    from e4s2024_amd import ops
    want = _want_keys(golden)
    with torch.device("meta"):
        sd = ops.OcclusionAwareSPADEGenerator().state_dict()
    assert len(want) == UPSTREAM_KEYS and [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert list(ops.generator_state_dict_shapes().items()) == want                            # what a mapping's keys are checked against
    assert sum(int(np.prod(s)) for k, s in want if not k.endswith(BUFFERS)) == UPSTREAM_PARAMS
    assert all(v.dtype == (torch.long if k.endswith("num_batches_tracked") else torch.float32) for k, v in sd.items())
    w = dict(want)
    assert w["second.weight"] == (512, 256, 1, 1) and w["third.conv.weight"] == (256, 512, 3, 3) and w["resblocks_3d.3dr5.conv2.weight"] == (32, 32, 3, 3, 3)
    assert w["decoder.G_middle_0.conv_0.weight_orig"] == (512, 512, 3, 3) and w["decoder.up_0.conv_s.weight_v"] == (512,)
    assert w["dense_motion_network.mask.weight"] == (16, 112, 7, 7, 7)
    front = ops.generator_front_structure_shapes(ops.generator_structure())
    assert list(front.items()) == [kv for kv in want if not kv[0].startswith("decoder.")]
    with torch.device("meta"):
        dec = ops.SPADEDecoder().state_dict()
    assert [("decoder." + k, tuple(v.shape)) for k, v in dec.items()] == [kv for kv in want if kv[0].startswith("decoder.")]
    assert list(ops.spade_decoder_state_dict_shapes().items()) == [(k, tuple(v.shape)) for k, v in dec.items()]
    for tag in TAGS:                                                                          # at the cases' configurations, and read off a mapping
        structure = ops.generator_structure(**M.config(tag))
        shapes = ops.generator_structure_shapes(structure, decoder=M.CASES[tag][6])
        assert list(shapes.items()) == [(k, tuple(v.shape)) for k, v in M.case(tag)["sd"].items()]
        assert ops.generator_structure_of_keys(M.case(tag)["sd"]) == structure == _net(tag).structure


def test_seeded_weights():
    from e4s2024_amd import seeded
    assert "seeded_generator_state_dict" in seeded.__all__
    sd = M.case("G-E")["sd"]
    template = {k: torch.empty(v.shape, dtype=v.dtype, device="meta") for k, v in sd.items()}
    a = seeded.seeded_generator_state_dict(template, M.WEIGHT_SEED)
    assert list(a) == list(template) and all(torch.equal(a[k], sd[k]) for k in a)               # reproducible
    assert not torch.equal(a["second.weight"], seeded.seeded_generator_state_dict({"second.weight": template["second.weight"]}, M.WEIGHT_SEED + 1)["second.weight"])
    dm = "dense_motion_network."                                                              # f18's function under the prefix
    inner = seeded.seeded_dense_motion_state_dict({k[len(dm):]: v for k, v in template.items() if k.startswith(dm)}, M.WEIGHT_SEED)
    assert len(inner) > 20 and all(torch.equal(a[dm + k], v) for k, v in inner.items())
    front = {k: v for k, v in a.items() if not k.startswith((dm, "decoder."))}
    scales = [v for k, v in front.items() if ".norm" in k and k.endswith(".weight")]
    assert len(scales) == 7 and all(int((v == 0).sum()) == 1 and float(v.abs().max()) <= 1.5 and float(v.min()) < 0 < float(v.max()) for v in scales)
    assert all(float(v.min()) >= 0.5 for k, v in front.items() if k.endswith("running_var"))
    assert all(float(v.abs().max()) > 0.05 for k, v in front.items() if k.endswith(("running_mean", ".bias")))
    assert all(v.dtype == torch.long for k, v in a.items() if k.endswith("num_batches_tracked"))
    sigmas = []
    for k, v in a.items():                                                                    # the decoder: unit v, u = normalize(W v), so sigma = |W v|
        if k.endswith(".weight_v"):
            W, u = a[k[:-2] + "_orig"].double(), a[k[:-2] + "_u"].double()
            Wv = W.reshape(W.shape[0], -1) @ v.double()
            assert abs(float(v.double().norm()) - 1) < 1e-6 and abs(float(u.norm()) - 1) < 1e-6 and M.max_err(u.numpy(), (Wv / Wv.norm()).numpy()) < 1e-6
            sigmas.append(float(u @ Wv))
    assert len(sigmas) == 18 and min(sigmas) > 0.5, min(sigmas)                                 # no sigma near zero


@pytest.mark.parametrize("tag", TAGS)
def test_mirror_on_the_cpu_against_the_model(tag):
    c = M.case(tag)
    net = _net(tag)
    kd, ks = M.kp_dicts(tag)
    f3 = net.source_feature(T(c["source"]))
    out = net.front(T(c["source"]), kd, ks)
    out["feature_3d"] = f3
    whole = net(T(c["source"]), kd, ks)
    assert list(whole) == ["mask"] + (["occlusion_map"] if "occlusion_map" in c["out64"] else []) + ["prediction"]      # the reference's output_dict
    if M.CASES[tag][6]:
        out["prediction"] = whole["prediction"]
    else:
        assert torch.equal(whole["prediction"], out["feature"])                               # decoder = nn.Identity(): the warped feature
    assert set(out) == set(c["out64"])
    for k, got in out.items():
        e = M.max_err(got.numpy(), c["out64"][k])
        print(f"{tag}.{k}: the mirror against the model {e:.3e} = {e / c['e32'][k]:.2f} e32")
        assert got.dtype == torch.float32 and e <= M.bound(c["e32"][k], c["out64"][k]), k
    net.train()
    try:
        with pytest.raises(NotImplementedError, match="eval"):
            net(T(c["source"]), kd, ks)
    finally:
        net.eval()


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_reenact, pipeline
    for name in ("OcclusionAwareSPADEGenerator", "SPADEDecoder", "PreparedGeneratorFront", "generator_state_dict_shapes", "generator_structure_of_keys",
                 "appearance_feature", "bn_relu", "deform_feature", "occlude", "generator_warp", "generator_front_forward"):
        assert name in ops_reenact.__all__ and getattr(ops, name) is getattr(ops_reenact, name)
    assert callable(pipeline.reenact_source_feature) and callable(pipeline.reenact_warp)
    assert not any(m.endswith(("sync_batchnorm", "modules.util", "modules.generator")) for m in e4s2024_amd._redirected())      # the drop-in is stage 4
    assert ops.LEAKY_SLOPE == 0.01


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert {n: len(_lib._PROTOS[n]) for n in ENTRY_POINTS} == ENTRY_POINTS
    assert "f19" in src and _lib.ABI_VERSION == 1
    cdll = _lib.lib().cdll
    assert all(hasattr(cdll, name) for name in ENTRY_POINTS)


def test_a_mapping_without_decoder_keys_is_accepted():
    """Everything up to the placement check passes for a module, a bare mapping, a mapping without the decoder's keys and the checkpoint file's dict."""
    from e4s2024_amd import ops, pipeline
    c = M.case("G-E")
    x = T(c["source"])
    kd, ks = M.kp_dicts("G-E")
    bare = {k: v for k, v in c["sd"].items() if not k.startswith("decoder.")}
    assert len(bare) < len(c["sd"])
    f3 = T(c["out64"]["feature_3d"].astype(np.float32))
    from e4s2024_amd import ops_reenact as R
    from e4s2024_amd.netweights import _validated
    for w in (_net("G-E"), c["sd"], bare, {"generator": c["sd"], "kp_detector": {}}, {"generator." + k: v for k, v in bare.items()},
              {"module." + k: v for k, v in bare.items()}):
        # what generator_warp hands on to dense_motion_forward, a module's dense_motion_network or the validated bare mapping, is something that function takes
        checked = R._generator_checked("t", w)[1]
        dmw = w.dense_motion_network if isinstance(w, torch.nn.Module) else checked[0]
        assert _validated("t", dmw, R._dm_net_of(dmw))[1] == checked[1][9]
        for call in (lambda: ops.appearance_feature(x, w), lambda: ops.generator_warp(f3, kd, ks, w), lambda: ops.generator_front_forward(x, kd, ks, w),
                     lambda: pipeline.reenact_source_feature(w, x), lambda: pipeline.reenact_warp(w, f3, kd, ks)):
            with pytest.raises(RuntimeError, match="CUDA"):                                   # a CPU tensor: the last refusal
                call()


def test_refusals_by_name_before_any_launch():
    from e4s2024_amd import ops
    c = M.case("G-B")
    x = T(c["source"])
    kd, ks = M.kp_dicts("G-B")
    f3 = T(c["out64"]["feature_3d"].astype(np.float32))
    net = M.make_module("G-B")
    with pytest.raises(RuntimeError, match="never loaded"):
        ops.generator_front_forward(x, kd, ks, net)
    net = _net("G-B")
    src = lambda x=x, w=net: ops.appearance_feature(x, w)                                     # noqa: E731
    warp = lambda f3=f3, kd=kd, ks=ks, w=net: ops.generator_warp(f3, kd, ks, w)               # noqa: E731
    with pytest.raises(ValueError, match="float32"):
        src(x=x.double())
    with pytest.raises(ValueError, match="three colour channels"):
        src(x=torch.zeros(1, 4, 16, 48))
    with pytest.raises(ValueError, match="num_down_blocks"):                                  # an odd side with one down block
        src(x=torch.zeros(1, 3, 17, 48))
    with pytest.raises(ValueError, match="num_blocks"):                                       # 8 x 22 features: the dense-motion network's two blocks need multiples of 4
        src(x=torch.zeros(1, 3, 16, 44))
    with pytest.raises(ValueError, match="at least 2"):
        ops.appearance_feature(torch.zeros(1, 3, 4, 8), _net("G-A"))                          # a 1 x 2 feature plane
    with pytest.raises(ValueError, match="float32"):
        warp(f3=f3.double())
    with pytest.raises(ValueError, match="reshape_channel"):
        warp(f3=torch.zeros(1, 5, 4, 8, 24))
    with pytest.raises(ValueError, match="num_blocks"):
        warp(f3=torch.zeros(1, 5, 3, 8, 22))
    with pytest.raises(ValueError, match="shared"):
        warp(f3=torch.zeros(2, 5, 3, 8, 24))
    with pytest.raises(ValueError, match="float32"):
        warp(kd=dict(kd, value=kd["value"].double()))
    with pytest.raises(ValueError, match="do not fit"):
        warp(kd=dict(kd, value=kd["value"][:, :2]))
    with pytest.raises(ValueError, match="only one"):
        warp(ks={"value": ks["value"]})
    with pytest.raises(TypeError, match="keypoint dict"):
        warp(kd=kd["value"])
    net.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            src()
    finally:
        net.eval()
    with pytest.raises(TypeError, match="mapping"):
        src(w=3)
    with pytest.raises(KeyError, match="first.conv.weight"):
        src(w={"second.weight": torch.zeros(15, 15, 1, 1)})
    sd = dict(c["sd"])
    del sd["resblocks_3d.3dr0.norm1.running_var"]
    with pytest.raises(KeyError, match="running_var"):
        src(w=sd)
    sd = dict(c["sd"])
    sd["fourth.bias"] = sd["fourth.bias"].double()
    with pytest.raises(ValueError, match="fourth.bias"):
        src(w=sd)
    # configurations: the view needs max_features == reshape_channel * reshape_depth; no generator without a dense-motion network
    with pytest.raises(ValueError, match="reshape_channel \\* reshape_depth"):
        ops.OcclusionAwareSPADEGenerator(max_features=256)
    with pytest.raises(ValueError, match="reshape_channel \\* reshape_depth"):
        ops.generator_state_dict_shapes(reshape_depth=8)
    with pytest.raises(ValueError, match="block_expansion"):
        ops.generator_structure(block_expansion=1024)
    with pytest.raises(ValueError, match="feature_channel"):
        ops.generator_structure(feature_channel=16)
    with pytest.raises(TypeError, match="first_kernel"):                                      # `first` is 3 x 3, as the reference builds it
        ops.generator_structure(first_kernel=7)
    with pytest.raises(ValueError, match="3 x 3"):
        src(w=dict(c["sd"], **{"first.conv.weight": torch.zeros(10, 3, 7, 7)}))
    none = ops.OcclusionAwareSPADEGenerator(**dict(M.config("G-B"), dense_motion_params=None))
    none.decoder = torch.nn.Identity()
    assert none.dense_motion_network is None and not any(k.startswith("dense_motion_network.") for k in none.state_dict())
    none.load_state_dict({k: v for k, v in c["sd"].items() if not k.startswith("dense_motion_network.")}, strict=True)
    with pytest.raises(ValueError, match="dense_motion_params"):
        src(w=none.eval())
    with pytest.raises(ValueError, match="dense_motion_params"):
        warp(w={k: v for k, v in c["sd"].items() if not k.startswith("dense_motion_network.")})
    with pytest.raises(ValueError, match="dense_motion_params"):
        none(x, kd, ks)
    # the ops: a size mismatch names both shapes, no resize is built
    with pytest.raises(ValueError, match=r"\(1, 3, 8, 12, 3\).*\(1, 5, 3, 8, 24\)"):
        ops.deform_feature(f3, torch.zeros(1, 3, 8, 12, 3))
    with pytest.raises(ValueError, match="float32"):
        ops.deform_feature(f3, torch.zeros(1, 3, 8, 24, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="batch"):
        ops.deform_feature(torch.zeros(2, 5, 3, 8, 24), torch.zeros(3, 3, 8, 24, 3))
    with pytest.raises(ValueError, match="out"):
        ops.deform_feature(f3, torch.zeros(1, 3, 8, 24, 3), out=torch.zeros(1, 15, 8, 25))
    with pytest.raises(ValueError, match=r"\(1, 1, 4, 12\).*\(1, 20, 8, 24\)"):
        ops.occlude(torch.zeros(1, 20, 8, 24), torch.zeros(1, 1, 4, 12))
    with pytest.raises(ValueError, match="float32"):
        ops.occlude(torch.zeros(1, 20, 8, 24).half(), torch.zeros(1, 1, 8, 24))
    with pytest.raises(ValueError, match="scale"):
        ops.bn_relu(torch.zeros(1, 5, 3, 8, 24), torch.zeros(4), torch.zeros(5))
    with pytest.raises(ValueError, match="float32"):
        ops.bn_relu(torch.zeros(1, 5, 3, 8, 24).double(), torch.zeros(5), torch.zeros(5))
    for call in (lambda: ops.deform_feature(f3, torch.zeros(1, 3, 8, 24, 3)), lambda: ops.occlude(torch.zeros(1, 20, 8, 24), torch.zeros(1, 1, 8, 24)),
                 lambda: ops.bn_relu(f3, torch.zeros(5), torch.zeros(5)), src, warp, lambda: ops.generator_front_forward(x, kd, ks, net)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
