"""A float64 restatement of the face-parsing feature loss (criteria/face_parsing/face_parsing_loss.py on criteria/face_parsing/unet.py::unet
(feature_scale=4).extract_feats, model_utils.py::unetConv2) in plain torch: the yardstick of tests/test_fp_cpu.py (against the fixture g16, made
from the reference's own classes) and of tests/test_gpu_fp.py."""
import numpy as np
import torch
import torch.nn.functional as F

from e4s2024_amd import ops_fp, seeded


def _conv_bn_relu(x, sd, p):
    x = F.conv2d(x, sd[p + ".0.weight"], sd[p + ".0.bias"], padding=1)
    x = F.batch_norm(x, sd[p + ".1.running_mean"], sd[p + ".1.running_var"], sd[p + ".1.weight"], sd[p + ".1.bias"], False, 0.0, 1e-5)
    return F.relu(x)


def block_outputs(x, sd):
    """The five encoder block outputs (not normalised) of unet.extract_feats."""
    out = []
    for i, name in enumerate(ops_fp.BLOCKS):
        if i:
            x = F.max_pool2d(x, 2)
        x = _conv_bn_relu(_conv_bn_relu(x, sd, name + ".conv1"), sd, name + ".conv2")
        out.append(x)
    return out


def unet_feats(x, sd):
    """unet.extract_feats: the l2-normalised, flattened block outputs."""
    return [t.reshape(t.shape[0], -1) / t.reshape(t.shape[0], -1).norm(2, 1, True) for t in block_outputs(x, sd)]


def preprocess(x):
    """FaceParsingLoss.extract_feats before the network: AdaptiveAvgPool2d((512, 512)) unless H is 512."""
    return x if x.shape[2] == 512 else F.adaptive_avg_pool2d(x, (512, 512))


def fp_loss(y_hat, y, sd):
    """(loss, sim_improvement, per-tap losses) of FaceParsingLoss.forward."""
    fh = unet_feats(preprocess(y_hat), sd)
    fy = [f.detach() for f in unet_feats(preprocess(y), sd)]
    per, sim = [], 0.0
    for a, b in zip(fh, fy):
        st = (a * b).sum(1)
        per.append((1 - st).mean())
        sim = sim + (st.detach() - (b * b).sum(1)).mean().item()
    return sum(per), sim, torch.stack(per)


def double_sd(sd):
    return {k: (v.detach().to(torch.float64) if v.is_floating_point() else v) for k, v in sd.items()}


def loss_and_grad(y_hat, y, sd):
    """(loss, sim_improvement, per-tap losses, d loss / d y_hat) in float64."""
    sd = double_sd(sd)
    x = y_hat.detach().to(torch.float64).requires_grad_(True)
    loss, sim, per = fp_loss(x, y.detach().to(torch.float64), sd)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), sim, per.detach(), g


def images(seed: int, side: int, bs: int):
    """The seeded (y_hat, y) pair of a fixture case, float32 in (-1, 1)."""
    x = np.tanh(seeded.seeded_array(seed, f"fp_x{side}", (bs, 3, side, side), dist="normal")).astype(np.float32)
    y = np.tanh(seeded.seeded_array(seed, f"fp_y{side}", (bs, 3, side, side), dist="normal")).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y)


def tap_rms(x, sd):
    """RMS of the un-normalised block outputs and their share of positive values (the seeded weights must keep them O(1))."""
    with torch.no_grad():
        outs = block_outputs(preprocess(x.to(torch.float64)), double_sd(sd))
    return [t.pow(2).mean().sqrt().item() for t in outs], [(t > 0).double().mean().item() for t in outs]
