"""Drop-in for the reference's ``criteria/face_parsing/face_parsing_loss.py``: ``FaceParsingLoss(opts)`` with the reference's constructor
(``torch.load(opts.face_parsing_model_path)`` from a local file; nothing is downloaded), its ``G.*`` state_dict and its
``forward(y_hat, y) -> (loss, sim_improvement)``; the unet encoder runs on the HIP kernels of ``e4s2024_amd.ops_fp`` (forward, and the gradient
with respect to ``y_hat``).  No cv2, torchvision or PIL import."""
import torch
from torch import nn

from e4s2024_amd import ops_fp


class FaceParsingLoss(nn.Module):
    """Face-parsing feature loss of ``y_hat`` against ``y``: per unet encoder block the mean over the batch of 1 - cos of the l2-normalised block
    outputs, summed over the five blocks; ``y``'s features are detached.  Images are pooled to 512 x 512 unless their height is 512."""

    def __init__(self, opts):
        super(FaceParsingLoss, self).__init__()
        self.opts = opts
        self.face_pool = torch.nn.AdaptiveAvgPool2d((512, 512))
        self.G = ops_fp.FaceParsingNet()
        self.G.load_state_dict(torch.load(opts.face_parsing_model_path, map_location="cpu"))
        self.G.eval()
        self.set_requires_grad(False)

    def set_requires_grad(self, flag=True):
        for p in self.parameters():
            p.requires_grad = flag

    def inference(self, x):
        raise NotImplementedError("FaceParsingLoss.inference needs the unet decoder and the label colour maps, which this engine does not provide; "
                                  "only the loss (forward / extract_feats) runs here")

    def extract_feats(self, x):
        return ops_fp.fp_features(x, self.G)

    def forward(self, y_hat, y):
        loss, sim, _ = ops_fp.fp_loss_terms(y_hat, y, self.G)
        return loss, float(sim)
