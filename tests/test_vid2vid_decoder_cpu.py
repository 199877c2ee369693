"""Row f20 (face-vid2vid's SPADEDecoder and whole frames) without a GPU: the two new entry points as the header declares them, the names the row adds, the
documents that name it, the module that stays unredirected, and every argument error that must raise before any launch (on CPU tensors the last refusal, the
placement check, is the proof that all the others passed)."""
import os
import re

import numpy as np
import pytest
import torch

import vid2vid_gen_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_v2v_spade_norm": 13, "e4s_v2v_image_head": 9}
NAMES = ("PreparedSPADEDecoder", "spade_norm", "image_head", "spade_decoder_forward", "generator_frames", "generator_forward", "NativeSPADEGenerator",
         "make_animation")

_NETS = {}


def _net():
    if not _NETS:
        net = M.make_module("G-E")
        net.load_state_dict(M.case("G-E")["sd"], strict=True)
        _NETS["G-E"] = net
    return _NETS["G-E"]


def _feature():
    return T(M.case("G-E")["out64"]["feature"].astype(np.float32))


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)
    assert {n: len(_lib._PROTOS[n]) for n in ENTRY_POINTS} == ENTRY_POINTS
    assert "/* f20:" in src and _lib.ABI_VERSION == 1 and "#define E4S_ABI_VERSION 1" in src
    cdll = _lib.lib().cdll
    assert all(hasattr(cdll, name) for name in ENTRY_POINTS)


def test_names_and_the_module_that_is_not_redirected():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_reenact_frames, pipeline
    for name in NAMES:                                                                        # the stage module's __all__, re-exported through ops
        assert name in ops_reenact_frames.__all__ and getattr(ops, name) is getattr(ops_reenact_frames, name), name
    assert callable(pipeline.reenact_frames) and callable(pipeline.reenact_clip)
    assert not any(m.endswith("modules.generator") for m in e4s2024_amd._redirected())
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## 4l."):]
    section = section[:section.index("\n## ", 4)]
    assert "modules.generator" in section and "not redirected" in section and "NativeSPADEGenerator" in section
    assert "until stage 4" not in text


def test_documents_name_the_row():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert re.search(r"\bf20\b", open(os.path.join(ROOT, doc)).read()), doc


def test_decoder_refusals_before_any_launch():
    from e4s2024_amd import ops
    net, f = _net(), _feature()
    dec = lambda f=f, w=net: ops.spade_decoder_forward(f, w)                                  # noqa: E731
    with pytest.raises(ValueError, match="float32"):
        dec(f=f.double())
    with pytest.raises(ValueError, match="256 channels"):
        dec(f=f[:, :255])
    with pytest.raises(ValueError, match="at least 2"):                                       # one element per plane: nothing for the instance norm
        dec(f=f[:, :, :1, :1])
    with pytest.raises(ValueError, match="16384"):
        dec(f=torch.zeros(1, 256, 2, 4097))
    with pytest.raises(TypeError, match="torch.Tensor"):
        dec(f=f.numpy())
    sd = M.case("G-E")["sd"]
    bare = {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}
    with pytest.raises(KeyError, match="up_0.norm_s.mlp_beta.bias"):
        dec(w={k: v for k, v in bare.items() if k != "up_0.norm_s.mlp_beta.bias"})
    with pytest.raises(KeyError, match="fc.weight"):                                          # a generator mapping without the decoder's keys
        dec(w={k: v for k, v in sd.items() if not k.startswith("decoder.")})
    with pytest.raises(ValueError, match="conv_img.bias"):
        dec(w=dict(bare, **{"conv_img.bias": bare["conv_img.bias"].double()}))
    with pytest.raises(TypeError, match="mapping"):
        dec(w=3)
    net.train()
    try:
        with pytest.raises(NotImplementedError, match="training mode"):
            dec()
        with pytest.raises(NotImplementedError, match="training mode"):
            dec(w=net.decoder)
    finally:
        net.eval()
    fresh = M.make_module("G-E")
    with pytest.raises(RuntimeError, match="never loaded"):
        dec(w=fresh)
    # every accepted form of weights passes everything up to the placement check
    forms = (net, net.decoder, sd, bare, {"decoder." + k: v for k, v in bare.items()}, {"generator.decoder." + k: v for k, v in bare.items()},
             {"module." + k: v for k, v in bare.items()}, {"module." + k: v for k, v in sd.items()}, {"generator": sd, "kp_detector": {}})
    for w in forms:
        with pytest.raises(RuntimeError, match="CUDA"):                                       # a CPU tensor: the last refusal
            dec(w=w)
        with pytest.raises(RuntimeError, match="CUDA"):                                       # ... and in front of the empty batch's early return too
            dec(f=f[:0], w=w)


def test_kernel_wrappers_refuse_before_any_launch():
    from e4s2024_amd import ops
    x, stats, gb = torch.zeros(2, 5, 3, 5), (torch.zeros(10), torch.ones(10)), torch.zeros(2, 10, 6, 10)
    with pytest.raises(ValueError, match="up is 3"):
        ops.spade_norm(x, stats, gb, up=3)
    with pytest.raises(ValueError, match="gamma \\| beta"):
        ops.spade_norm(x, stats, gb, up=1)                                                    # gb is the x2 size
    with pytest.raises(ValueError, match="gamma \\| beta"):
        ops.spade_norm(x, stats, gb, gb[:, :, :3], up=2)
    with pytest.raises(ValueError, match="mean"):
        ops.spade_norm(x, (torch.zeros(9), torch.ones(10)), gb, up=2)
    with pytest.raises(ValueError, match="float32"):
        ops.spade_norm(x.double(), stats, gb, up=2)
    with pytest.raises(ValueError, match="out_s without"):
        ops.spade_norm(x, stats, gb, up=2, out_s=torch.zeros(2, 5, 6, 10))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.spade_norm(x, stats, gb, gb, up=2)
    w, b = torch.zeros(3, 5, 3, 3), torch.zeros(3)
    with pytest.raises(ValueError, match=r"\(3, 5, 3, 3\)"):
        ops.image_head(x, torch.zeros(3, 4, 3, 3), b)
    with pytest.raises(ValueError, match=r"\(3, 5, 3, 3\)"):
        ops.image_head(x, torch.zeros(4, 5, 3, 3), torch.zeros(4))
    with pytest.raises(ValueError, match="float32"):
        ops.image_head(x, w.double(), b)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.image_head(x, w, b)


def test_frame_entry_points_refuse_before_any_launch():
    from e4s2024_amd import ops, pipeline
    c = M.case("G-E")
    net = _net()
    x = T(c["source"])
    kd, ks = M.kp_dicts("G-E")
    f3 = T(c["out64"]["feature_3d"].astype(np.float32))
    front_only = {k: v for k, v in c["sd"].items() if not k.startswith("decoder.")}
    native = ops.NativeSPADEGenerator(net)
    calls = {"generator_frames": lambda w: ops.generator_frames(f3, kd, ks, w), "generator_forward": lambda w: ops.generator_forward(x, kd, ks, w),
             "reenact_frames": lambda w: pipeline.reenact_frames(w, f3, kd, ks),
             "make_animation": lambda w: ops.make_animation(x, x.repeat(2, 1, 1, 1), w, None, None)}
    for nm, call in calls.items():
        with pytest.raises(KeyError, match="fc.weight"):                                      # the front's keys alone do not make a frame
            call(front_only)
        with pytest.raises(RuntimeError, match="CUDA"):
            call(net)
        with pytest.raises(RuntimeError, match="CUDA"):
            call({"generator": c["sd"]})
    net.train()
    try:
        for call in list(calls.values()) + [lambda w: native(x, kd, ks)]:
            with pytest.raises(NotImplementedError, match="training mode"):
                call(net)
    finally:
        net.eval()
    with pytest.raises(RuntimeError, match="CUDA"):
        native(x, kp_source=ks, kp_driving=kd)                                                # by keyword, as the reference's make_animation calls it
    assert native.feature_builds == 0
    with pytest.raises(ValueError, match="expected that batch, or 1"):
        ops.generator_forward(x.repeat(3, 1, 1, 1), kd, ks, net)
    with pytest.raises(ValueError, match="batch is 0"):
        ops.make_animation(x, x, net, None, None, batch=0)
    with pytest.raises(ValueError, match="of one size"):
        ops.make_animation(x.repeat(2, 1, 1, 1), x, net, None, None)
    with pytest.raises(TypeError, match="module"):
        ops.NativeSPADEGenerator(c["sd"])

