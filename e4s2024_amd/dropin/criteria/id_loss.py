"""Drop-in for the reference's ``criteria/id_loss.py``: ``IDLoss(opts)`` with the reference's constructor (``torch.load(opts.ir_se50_path)`` from a
local file; nothing is downloaded), its ``facenet.*`` state_dict and its ``forward(y_hat, y) -> (loss, sim_improvement, None)``; the ArcFace
network runs on the HIP kernels of ``e4s2024_amd.ops_id`` (forward, and the gradient with respect to ``y_hat``)."""
import torch
from torch import nn

from e4s2024_amd import ops_id


class IDLoss(nn.Module):
    """Identity loss of ``y_hat`` against ``y``: per feature scale (five with ``opts.id_loss_multiscale``, else the 512-d embedding) the mean over
    the batch of 1 - cos of the l2-normalised features, summed over scales; ``y``'s features are detached."""

    def __init__(self, opts):
        super(IDLoss, self).__init__()
        self.opts = opts
        self.face_pool_1 = torch.nn.AdaptiveAvgPool2d((256, 256))
        self.facenet = ops_id.IdNet()
        self.facenet.load_state_dict(torch.load(opts.ir_se50_path, map_location="cpu"))
        self.face_pool_2 = torch.nn.AdaptiveAvgPool2d((112, 112))
        self.facenet.eval()
        self.set_requires_grad(False)

    def set_requires_grad(self, flag=True):
        for p in self.parameters():
            p.requires_grad = flag

    def extract_feats(self, x):
        return ops_id.id_features(x, self.facenet, multiscale=self.opts.id_loss_multiscale)

    def forward(self, y_hat, y):
        loss, sim, _ = ops_id.id_loss_terms(y_hat, y, self.facenet, multiscale=self.opts.id_loss_multiscale)
        return loss, float(sim), None
