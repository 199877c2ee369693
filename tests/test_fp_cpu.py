"""Face-parsing feature loss without a GPU: the float64 restatement (tests/fp_model.py) against the fixture g16 made from the reference's own
criteria/face_parsing/face_parsing_loss.py, the host-built pooling operator, the network's state_dict layout, the seeded weights and the drop-in's
loading and refusals."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp_model as M
from conftest import install_dropin, load_golden
from e4s2024_amd import lossnet, ops_fp, seeded


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_face_parsing")


@pytest.fixture(scope="module")
def sd(g16):
    return seeded.seeded_unet_state_dict(int(g16["seed"]))


@pytest.mark.parametrize("side", [512, 1024, 256])
def test_restatement_matches_fixture(g16, sd, side):
    x, y = M.images(int(g16["seed"]), side, 2)
    loss, sim, per, g = M.loss_and_grad(x, y, sd)
    want = float(g16[f"loss{side}"])
    assert abs(loss.item() - want) <= 1e-10 * abs(want), (loss.item(), want)
    assert abs(sim - float(g16[f"sim{side}"])) <= 1e-10 * abs(want)
    np.testing.assert_allclose(per.numpy(), g16[f"per{side}"], rtol=1e-10)
    samp = g.reshape(-1).numpy()[g16[f"grad{side}_idx"]]
    norm = float(g16[f"grad{side}_norm"])
    np.testing.assert_allclose(samp, g16[f"grad{side}_samples"], rtol=1e-10, atol=1e-10 * norm)
    assert abs(g.norm().item() - norm) <= 1e-10 * norm


@pytest.mark.parametrize("side", [256, 1024, 600])
def test_pooling_operator(side):
    """AdaptiveAvgPool2d((512, 512)) as the banded matrices the GPU resampler reads."""
    x = torch.from_numpy(np.random.RandomState(side).standard_normal((1, 3, side, side)))
    A = torch.from_numpy(lossnet.pool_matrix(side, ops_fp.SIDE))
    got = torch.einsum("iy,bcyx,jx->bcij", A, x, A)
    assert (got - M.preprocess(x)).abs().max().item() <= 1e-12
    rows, cols = lossnet.bands(A.numpy())
    assert 1 <= (rows[:, 1] - rows[:, 0]).min() and (rows[:, 1] - rows[:, 0]).max() <= -(-side // 512) + 1
    assert ((cols[:, 1] - cols[:, 0]) >= 1).all()


def test_state_dict_layout(g16, sd):
    keys = [str(k) for k in g16["keys"]]
    assert len(keys) == 136 and keys == ["G." + k for k in ops_fp.state_dict_keys()]
    shapes = ops_fp.state_dict_shapes()
    for k, shp in zip(keys, g16["shapes"]):
        s = list(shapes[k[len("G."):]])
        assert s + [1] * (4 - len(s)) == list(shp), k
    assert list(sd.keys()) == ops_fp.state_dict_keys()
    enc = ops_fp.encoder_keys()
    assert len(enc) == 70 and sum(sd[k].numel() for k in enc) == 1182746
    assert sum(v.numel() for v in sd.values()) == 1947317


def test_seeded_weights_keep_activations_o1(g16, sd):
    x, _ = M.images(int(g16["seed"]), 256, 1)
    rms, pos = M.tap_rms(x, sd)
    assert all(0.05 <= r <= 20 for r in rms), rms
    assert all(0.2 <= p <= 0.9 for p in pos), pos


def test_dropin_loads_checkpoint_and_refuses_wrong_keys(g16, sd, tmp_path):
    install_dropin()
    from criteria.face_parsing.face_parsing_loss import FaceParsingLoss
    path = os.path.join(tmp_path, "face_parsing.pth")
    torch.save(sd, path)
    m = FaceParsingLoss(types.SimpleNamespace(face_parsing_model_path=path))
    assert list(m.state_dict().keys()) == [str(k) for k in g16["keys"]]
    assert all(torch.equal(m.G.state_dict()[k], v) for k, v in sd.items())
    assert not m.G.training and not any(p.requires_grad for p in m.parameters())
    assert ops_fp.check_loaded(m) is m
    with pytest.raises(NotImplementedError, match="decoder"):
        m.inference(torch.zeros(1, 3, 512, 512))
    bad = dict(sd)
    bad["conv1.conv1.0.weightx"] = bad.pop("conv1.conv1.0.weight")
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match="conv1.conv1.0.weight"):
        FaceParsingLoss(types.SimpleNamespace(face_parsing_model_path=path))
    torch.save({k: v for k, v in sd.items() if not k.startswith("final.")}, path)       # the reference loads strictly: the decoder keys are required
    with pytest.raises(RuntimeError, match="final"):
        FaceParsingLoss(types.SimpleNamespace(face_parsing_model_path=path))


def test_refuses_unloaded_and_training_mode(sd):
    with pytest.raises(RuntimeError, match="never loaded"):
        ops_fp.check_loaded(ops_fp.FaceParsingNet().eval())
    net = ops_fp.FaceParsingNet()
    net.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="training mode"):
        ops_fp.check_loaded(net.train())
    with pytest.raises(KeyError, match=r"fp_loss: the weights lack 'center\.conv2\.1\.running_var'"):
        ops_fp.weight_tensors({k: v for k, v in sd.items() if k != "center.conv2.1.running_var"})
    from e4s2024_amd import pti
    with pytest.raises(RuntimeError, match="never loaded"):
        pti.style_vector_step(None, None, None, None, None, face_parsing=ops_fp.FaceParsingNet().eval())


def test_flat_image_restatement_routes_to_first_maximum(sd):
    """On a flat image every 2 x 2 window of the interior ties; PyTorch's max pool sends the gradient to the first element (row-major).  The GPU
    test compares against this gradient, so pin here that the restatement has those ties and that rule."""
    x = torch.full((1, 3, 64, 64), 0.3, dtype=torch.float64)
    outs = M.block_outputs(x, M.double_sd(sd))
    a = outs[0][0, :, 8:56, 8:56].reshape(16, 24, 2, 24, 2)
    assert (a == a[:, :, :1, :, :1]).all()
    t = outs[0].detach().clone().requires_grad_(True)
    F.max_pool2d(t, 2).sum().backward()
    gw = t.grad[0, :, 8:56, 8:56].reshape(16, 24, 2, 24, 2)
    assert (gw[:, :, 0, :, 0] == 1).all() and gw.sum().item() == 16 * 24 * 24
