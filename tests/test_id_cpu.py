"""ArcFace identity loss without a GPU: the float64 restatement (tests/id_model.py) against the fixture g15 made from the reference's own
criteria/id_loss.py, the host-built pre-processing operator, the drop-in's state_dict layout and its refusals."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import id_model as M
from conftest import install_dropin, load_golden
from e4s2024_amd import lossnet, ops_id, seeded


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_id")


@pytest.fixture(scope="module")
def sd(g15):
    return seeded.seeded_irse50_state_dict(int(g15["seed"]))


@pytest.mark.parametrize("side", [112, 256])
def test_restatement_matches_fixture(g15, sd, side):
    x, y = M.images(int(g15["seed"]), side, 2)
    for ms, tag in ((True, "ms"), (False, "ss")):
        loss, sim, per, g = M.loss_and_grad(x, y, sd, ms)
        want = float(g15[f"loss{side}_{tag}"])
        assert abs(loss.item() - want) <= 1e-9 * abs(want), (tag, loss.item(), want)
        assert abs(sim - float(g15[f"sim{side}_{tag}"])) <= 1e-9 * abs(want)
        if ms:
            np.testing.assert_allclose(per.numpy(), g15[f"per{side}"], rtol=1e-9)
        samp = g.reshape(-1).numpy()[g15[f"grad{side}_{tag}_idx"]]
        np.testing.assert_allclose(samp, g15[f"grad{side}_{tag}_samples"], rtol=1e-9, atol=1e-9 * float(g15[f"grad{side}_{tag}_norm"]))
    if side == 112:
        _, _, _, g = M.loss_and_grad(x, y, sd, True)
        assert np.abs(g.numpy() - g15["grad112_ms"]).max() <= 1e-6 * np.abs(g15["grad112_ms"]).max()


@pytest.mark.parametrize("side", [256, 300, 512, 1024])
def test_preprocessing_operator(side):
    x = torch.from_numpy(np.random.RandomState(side).standard_normal((2, 3, side, side)))
    ay, ax = ops_id.axis_matrix(side, side != 256, ops_id.CROP[0]), ops_id.axis_matrix(side, side != 256, ops_id.CROP[1])
    got = torch.einsum("iy,bcyx,jx->bcij", torch.from_numpy(ay), x, torch.from_numpy(ax))
    want = M.preprocess(x)
    assert (got - want).abs().max().item() <= 1e-12
    (ry, cy), (rx, cx) = lossnet.bands(ay), lossnet.bands(ax)
    for A, rows, cols in ((ay, ry, cy), (ax, rx, cx)):
        for i in range(A.shape[0]):
            assert np.count_nonzero(A[i]) == rows[i, 1] - rows[i, 0] and A[i, rows[i, 0]:rows[i, 1]].all()
        for j in range(A.shape[1]):
            assert np.count_nonzero(A[:, j]) == cols[j, 1] - cols[j, 0]


def test_state_dict_layout(g15, sd):
    keys = [str(k) for k in g15["keys"]]
    assert len(keys) == 397 and keys == ["facenet." + k for k in ops_id.state_dict_keys()]
    shapes = ops_id.state_dict_shapes()
    for k, shp in zip(keys, g15["shapes"]):
        s = list(shapes[k[len("facenet."):]])
        assert s + [1] * (4 - len(s)) == list(shp), k
    assert list(sd.keys()) == ops_id.state_dict_keys()


def test_dropin_layout_and_refusals(g15, sd, tmp_path):
    install_dropin()
    from criteria.id_loss import IDLoss
    path = os.path.join(tmp_path, "ir_se50.pth")
    torch.save(sd, path)
    m = IDLoss(types.SimpleNamespace(ir_se50_path=path, id_loss_multiscale=True))
    assert list(m.state_dict().keys()) == [str(k) for k in g15["keys"]]
    assert not m.facenet.training and not any(p.requires_grad for p in m.parameters())
    assert ops_id.check_loaded(m) is m
    with pytest.raises(RuntimeError, match="never loaded"):
        ops_id.check_loaded(ops_id.IdNet().eval())
    with pytest.raises(RuntimeError, match="training mode"):
        ops_id.check_loaded(m.facenet.train())
    with pytest.raises(RuntimeError, match="training mode"):
        ops_id.check_loaded(m)
    m.facenet.eval()
    from e4s2024_amd import pti
    with pytest.raises(RuntimeError, match="never loaded"):
        pti.style_vector_step(None, None, None, None, None, id_loss=ops_id.IdNet().eval())


def test_seeded_weights_keep_activations_o1(g15, sd):
    x, _ = M.images(int(g15["seed"]), 256, 1)
    assert all(0.05 <= r <= 20 for r in M.tap_rms(x, sd))
