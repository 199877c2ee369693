"""A float64 restatement of the ArcFace identity loss (criteria/id_loss.py on models/encoders/model_irse.py::Backbone(112, 50, 'ir_se'),
helpers.py::bottleneck_IR_SE) in plain torch: the yardstick of tests/test_id_cpu.py (against the fixture g15, made from the reference's own
classes) and of tests/test_gpu_id.py."""
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import ops_id, seeded

TAP_UNITS = (2, 6, 20, 23)


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def _unit(x, sd, i, cin, depth, stride):
    p = f"body.{i}."
    if cin == depth:
        short = F.max_pool2d(x, 1, stride)
    else:
        short = _bn(F.conv2d(x, sd[p + "shortcut_layer.0.weight"], stride=stride), sd, p + "shortcut_layer.1")
    r = _bn(x, sd, p + "res_layer.0")
    r = F.conv2d(r, sd[p + "res_layer.1.weight"], padding=1)
    r = F.prelu(r, sd[p + "res_layer.2.weight"])
    r = _bn(F.conv2d(r, sd[p + "res_layer.3.weight"], stride=stride, padding=1), sd, p + "res_layer.4")
    g = F.adaptive_avg_pool2d(r, 1)
    g = torch.sigmoid(F.conv2d(F.relu(F.conv2d(g, sd[p + "res_layer.5.fc1.weight"])), sd[p + "res_layer.5.fc2.weight"]))
    return r * g + short


def backbone(x, sd, multi_scale=True):
    """Backbone.forward(x, multi_scale): the l2-normalised features."""
    x = F.prelu(_bn(F.conv2d(x, sd["input_layer.0.weight"], padding=1), sd, "input_layer.1"), sd["input_layer.2.weight"])
    taps = []
    for i, u in enumerate(ops_id.units()):
        x = _unit(x, sd, i, *u)
        if multi_scale and i in TAP_UNITS:
            taps.append(x.reshape(x.shape[0], -1))
    x = _bn(x, sd, "output_layer.0").reshape(x.shape[0], -1)
    x = F.linear(x, sd["output_layer.3.weight"], sd["output_layer.3.bias"])
    x = F.batch_norm(x, sd["output_layer.4.running_mean"], sd["output_layer.4.running_var"], sd["output_layer.4.weight"], sd["output_layer.4.bias"],
                     False, 0.0, 1e-5)
    taps.append(x)
    return [t / t.norm(2, 1, True) for t in taps]


def preprocess(x):
    """IDLoss.extract_feats before the network: pool to 256 unless H is 256, crop, pool to 112."""
    if x.shape[2] != 256:
        x = F.adaptive_avg_pool2d(x, (256, 256))
    return F.adaptive_avg_pool2d(x[:, :, 35:223, 32:220], (112, 112))


def id_loss(y_hat, y, sd, multi_scale=True):
    """(loss, sim_improvement, per-scale losses) of IDLoss.forward."""
    fh = backbone(preprocess(y_hat), sd, multi_scale)
    fy = [f.detach() for f in backbone(preprocess(y), sd, multi_scale)]
    per, sim = [], 0.0
    for a, b in zip(fh, fy):
        st = (a * b).sum(1)
        per.append((1 - st).mean())
        sim = sim + (st.detach() - (b * b).sum(1)).mean().item()
    return sum(per), sim, torch.stack(per)


def double_sd(sd):
    return {k: (v.detach().to(torch.float64) if v.is_floating_point() else v) for k, v in sd.items()}


def loss_and_grad(y_hat, y, sd, multi_scale=True):
    """(loss, sim_improvement, per-scale losses, d loss / d y_hat) in float64."""
    sd = double_sd(sd)
    x = y_hat.detach().to(torch.float64).requires_grad_(True)
    loss, sim, per = id_loss(x, y.detach().to(torch.float64), sd, multi_scale)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), sim, per.detach(), g


def images(seed: int, side: int, bs: int):
    """The seeded (y_hat, y) pair of a fixture case, float32 in (-1, 1)."""
    x = np.tanh(seeded.seeded_array(seed, f"id_x{side}", (bs, 3, side, side), dist="normal")).astype(np.float32)
    y = np.tanh(seeded.seeded_array(seed, f"id_y{side}", (bs, 3, side, side), dist="normal")).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y)


def tap_rms(x, sd):
    """RMS of the un-normalised activations at the five taps (the seeded weights must keep them O(1))."""
    sd = double_sd(sd)
    x = preprocess(x.to(torch.float64))
    x = F.prelu(_bn(F.conv2d(x, sd["input_layer.0.weight"], padding=1), sd, "input_layer.1"), sd["input_layer.2.weight"])
    out = []
    for i, u in enumerate(ops_id.units()):
        x = _unit(x, sd, i, *u)
        if i in TAP_UNITS:
            out.append(x.pow(2).mean().sqrt().item())
    return out
