"""Row f9 (Blender recolouring, stage 2) without a GPU: the float64 restatement ``resunet_model`` against the reference's own ``ResUNet``
(``g21_resunet.npz``), the bar of the GPU tests pinned from the other side by single-change mutants, the mirror module, the package's names and the argument
errors that must raise before any launch.

The bound of a case is ``max(8 e32, 2e-7)``, ``e32`` the model in float32 against itself in float64 (the reference's arithmetic class, 4e-7 .. 7e-6 over
the cases, computed here).  Every mutant of the model moves the float64 output by at least ten bounds (measured: 900 bounds for the nearest one, conv1.bias
left out of the bn2 fold at 256 x 256), so a kernel inside the bound has none of these mistakes."""
import argparse

import numpy as np
import pytest
import torch

import resunet_model as RM
from conftest import load_golden

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ENTRY_POINTS = {"e4s_resunet_preact", "e4s_resunet_up_cat_preact", "e4s_resunet_head"}


def _stored(tag, full):
    return full.reshape(-1)[RM.sample_positions(tag)] if tag in RM.SAMPLED else full


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_model_against_the_reference(tag):
    g = load_golden("g21_resunet")
    assert RM.crc(RM.case_inputs(tag)) == int(g[f"{tag}.crc"]), "the seeded inputs are not the ones the fixture was made from"
    out = RM.reference_output(tag)
    H, W, bs, _ = RM.CASES[tag]
    assert out.shape == (bs, 3, H, W) and g[f"{tag}.out"].dtype == np.float32
    err, e32 = RM.max_err(_stored(tag, out), g[f"{tag}.out"]), RM.e32(tag)
    print(f"{tag}: model against the reference {err:.3e} (when the fixture was made {float(g[f'{tag}.ref_err']):.3e}), e32 {e32:.3e}, bound {RM.bound(e32):.3e}")
    assert err <= RM.bound(e32)


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_output_is_spread_over_the_unit_interval(tag):
    out = RM.reference_output(tag)
    inside = float(((out > 0.02) & (out < 0.98)).mean())
    print(f"{tag}: std {out.std():.3f}, {100 * inside:.1f} % in (0.02, 0.98)")
    assert out.std() >= 0.15 and inside >= 0.90


@pytest.mark.parametrize("tag", list(RM.CASES))
def test_every_mutant_is_ten_bounds_away(tag):
    want, bound = RM.reference_output(tag), RM.bound(RM.e32(tag))
    for mutant in RM.MUTANTS:
        moved = RM.max_err(RM.forward(RM.state_dict(RM.CASES[tag][3]), RM.case_inputs(tag), mutant=mutant), want)
        print(f"{tag}: {mutant} moves the output by {moved:.3e} = {moved / bound:.0f} bounds")
        assert moved >= RM.MUTANT_MARGIN * bound, mutant


@pytest.mark.parametrize("width", [64, 16])
def test_seeded_batchnorm_has_a_zero_and_negative_scales(width):
    sd = RM.state_dict(width)
    gammas = [v for k, v in sd.items() if ".bn" in k and k.endswith(".weight")]
    assert len(gammas) == 13
    for g in gammas:
        assert int((g == 0).sum()) == 1 and int((g < 0).sum()) >= 3 and float(g.abs().max()) <= 1.5
    assert all(0.5 <= float(v.min()) and float(v.max()) <= 2.0 for k, v in sd.items() if k.endswith("running_var"))
    assert all(float(v.abs().max()) <= 0.5 for k, v in sd.items() if k.endswith("running_mean") or (".bn" in k and k.endswith(".bias")))


@pytest.mark.parametrize("width", [64, 16])
def test_mirror_has_the_reference_keys_and_shapes(width):
    from e4s2024_amd import ops
    g = load_golden("g21_resunet")
    want = [(line.split("|")[0], tuple(int(d) for d in line.split("|")[1].split("x") if d)) for line in str(g[f"keys.w{width}"]).split("\n")]
    net = ops.ResUNet(width)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    assert list(ops.resunet_state_dict_shapes(width).items()) == want
    net.load_state_dict(RM.state_dict(width), strict=True)
    prefixed = {"unet." + k: v for k, v in RM.state_dict(width).items()}                     # latest_netG.pth's entries: the prefix taken off
    ops.ResUNet(width).load_state_dict({k[len("unet."):]: v for k, v in prefixed.items()}, strict=True)
    with pytest.raises(ValueError, match="width 32"):
        ops.ResUNet(32)


@pytest.mark.parametrize("tag", ["8x8.w64", "32x32.b2.w16", "48x64.w64"])
def test_mirror_in_float64_equals_the_model(tag):
    from e4s2024_amd import ops
    net = ops.ResUNet(RM.CASES[tag][3]).eval()
    net.load_state_dict(RM.state_dict(RM.CASES[tag][3]))
    with torch.no_grad():
        got = net.double()(T(RM.case_inputs(tag)).double()).numpy()
    assert RM.max_err(got, RM.reference_output(tag)) <= 1e-12                               # two float64 evaluations: BatchNorm is factored differently


def test_names_and_overrides():
    import e4s2024_amd
    from e4s2024_amd import ops, ops_recolor, seeded
    for name in ("ResUNet", "blender_unet", "blender_recolor", "resunet_state_dict_shapes", "PreparedResUNet", "RESUNET_WIDTHS"):
        assert name in ops_recolor.__all__ and getattr(ops, name) is getattr(ops_recolor, name)
    assert "seeded_resunet_state_dict" in seeded.__all__
    assert e4s2024_amd.RECOLOR_NET_OVERRIDES == {"swap_face_fine.Blender.model_center.res_u_net": "swap_face_fine/Blender/model_center/res_u_net.py"}
    assert set(e4s2024_amd.RECOLOR_NET_OVERRIDES) <= set(e4s2024_amd._redirected())
    assert e4s2024_amd.RECOLOR_OVERRIDES == {"swap_face_fine.Blender.model_center.semantic_tools": "swap_face_fine/Blender/model_center/semantic_tools.py"}


def test_entry_points_are_declared_once_and_bound():
    from e4s2024_amd import _lib
    assert ENTRY_POINTS <= set(_lib.declared_symbols()) and ENTRY_POINTS <= set(_lib._PROTOS)
    src = open(_lib.HEADER).read()
    assert all(src.count(name + "(") == 1 for name in ENTRY_POINTS)


def _dropin():
    from conftest import install_dropin
    install_dropin()
    import e4s2024_amd
    from swap_face_fine.Blender.model_center import res_u_net
    assert res_u_net.__file__.startswith(e4s2024_amd.DROPIN_DIR)
    return res_u_net


def test_dropin_exports_the_reference_names_and_keys():
    m = _dropin()
    g = load_golden("g21_resunet")
    assert all(hasattr(m, n) for n in ("ResUNet", "ResBlock", "InputEncodeLayer"))
    for small, width in ((False, 64), (True, 16)):
        net = m.ResUNet(argparse.Namespace(small_FPN=small))
        assert [f"{k}|{'x'.join(str(d) for d in v.shape)}" for k, v in net.state_dict().items()] == str(g[f"keys.w{width}"]).split("\n")
        net.load_state_dict(RM.state_dict(width), strict=True)
        with pytest.raises(NotImplementedError, match="eval"):
            net.train()(T(RM.case_inputs("8x8.w64")))
    assert list(m.ResBlock(8, 16, 2).state_dict()) == [k[len("res_en_layer2."):] for k in net.state_dict() if k.startswith("res_en_layer2.")]
    assert list(m.InputEncodeLayer(12, 16).state_dict()) == [k[len("input_encoder_layer."):] for k in net.state_dict() if k.startswith("input_encoder_layer.")]


def test_argument_errors_before_any_launch():
    from e4s2024_amd import ops
    net = ops.ResUNet(16).eval()
    net.load_state_dict(RM.state_dict(16))
    good = T(RM.case_inputs("8x8.w16"))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):                           # CPU tensors are refused once everything else is in order
        ops.blender_unet(good, net)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_unet(good, RM.state_dict(16))                                             # a mapping serves as weights too
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_unet(good.expand(2, -1, -1, -1).transpose(2, 3), net)                     # non-contiguous input is accepted as far as the checks go
    with pytest.raises(TypeError):
        ops.blender_unet(good.numpy(), net)
    with pytest.raises(TypeError):
        ops.blender_unet(good, None)
    with pytest.raises(ValueError, match="float32"):
        ops.blender_unet(good.double(), net)
    with pytest.raises(ValueError, match="float32"):
        ops.blender_unet(good[0], net)                                                        # rank
    with pytest.raises(ValueError, match="12"):
        ops.blender_unet(good[:, :11], net)
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.blender_unet(torch.zeros(1, 12, 8, 12), net)
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.blender_unet(torch.zeros(1, 12, 4, 8), net)
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.blender_unet(torch.zeros(1, 12, 0, 8), net)
    with pytest.raises(RuntimeError, match="training mode"):
        ops.blender_unet(good, ops.ResUNet(16))
    with pytest.raises(RuntimeError, match="device mismatch"):
        ops.blender_unet(good, ops.ResUNet(16).eval().to("meta"))
    with pytest.raises(RuntimeError, match="training mode"):
        ops.blender_recolor(None, None, None, None, None, None, 7.0, ops.ResUNet(16))
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.blender_recolor(torch.zeros(1, 3, 12, 12), torch.zeros(1, 3, 12, 12), None, None, None, None, 7.0, net)
    lab = torch.zeros(1, 16, 16, dtype=torch.uint8)
    img, feats = torch.zeros(1, 3, 16, 16), torch.zeros(1, 256, 4, 4)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ops.blender_recolor(img, img, lab, lab, feats, feats, 7.0, net)
    with pytest.raises(TypeError):
        ops.blender_recolor(img, img, lab, lab, feats, None, 7.0, net)


def test_inner_weights_are_refused_by_name_before_any_launch():
    """Every key, shape and dtype of a Res-U-Net is checked on the host, not the first convolution's alone; CPU tensors are refused after that."""
    from e4s2024_amd import ops
    good, sd, key = T(RM.case_inputs("8x8.w16")), RM.state_dict(16), "res_en_layer3.conv2.weight"
    assert tuple(sd[key].shape) == (64, 64, 3, 3)
    for call in (lambda w: ops.blender_unet(good, w), lambda w: ops.resunet_weight_tensors(w),
                 lambda w: ops.blender_recolor(None, None, None, None, None, None, 7.0, w)):
        with pytest.raises(KeyError, match=key):
            call({k: v for k, v in sd.items() if k != key})
        with pytest.raises(ValueError, match=key):
            call({**sd, key: torch.zeros(64, 32, 3, 3)})                                      # the wrong cin
        with pytest.raises(ValueError, match=f"{key}.*float64"):
            call({**sd, key: sd[key].double()})
        with pytest.raises(KeyError, match=key):
            call({"unet." + k: v for k, v in sd.items() if k != key})
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):                           # num_batches_tracked is no float weight: not asked for
        ops.blender_unet(good, {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
