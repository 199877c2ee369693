"""Drop-in for the reference's ``swap_face_fine/gpen/sr_model/real_esrnet.py``: ``RealESRNet`` with the reference's constructor, the same checkpoint file
(``<base_dir>/weights/realesrnet_x2.pth`` without ``model``, ``<base_dir>/weights/<model>_x<scale>.pth`` with one) and ``process(img)``, numpy BGR uint8 in
and out, the whole of it on the device (``ops.gpen_sr_image``).  Neither cv2 nor basicsr is imported.

An image with no more rows or columns than the reflect pad adds raises ``ValueError`` (the reference's ``F.pad`` raises ``RuntimeError`` there, in front of its
``try``).  The reference's ``sr failed`` branch, which swallows every error of the network and returns None, has no counterpart: an error here is raised."""
import os

import numpy as np
import torch

from e4s2024_amd import ops
from swap_face_fine.gpen.sr_model.rrdbnet_arch import RRDBNet


def checkpoint_path(base_dir, model, scale):
    """Where the reference looks for its checkpoint (real_esrnet.py:17-20)."""
    return os.path.join(base_dir, "weights", "realesrnet_x2.pth" if model is None else model + "_x%d.pth" % scale)


class RealESRNet(object):
    def __init__(self, base_dir="./", model=None, scale=2, device="cuda"):
        self.base_dir = base_dir
        self.scale = scale
        self.device = device
        self.load_srmodel(base_dir, model)

    def load_srmodel(self, base_dir, model):
        self.srmodel = RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=32, num_block=23, num_grow_ch=32, scale=self.scale)
        loadnet = torch.load(checkpoint_path(self.base_dir, model, self.scale), map_location="cpu")
        self.srmodel.load_state_dict(loadnet["params_ema"], strict=True)
        self.srmodel.eval()
        self.srmodel = self.srmodel.to(self.device)

    def process(self, img):
        """``img``: a uint8 BGR image ``[H, W, 3]`` (numpy, or a tensor on any device).  Returns the super-resolved uint8 BGR numpy image."""
        frame = torch.as_tensor(np.ascontiguousarray(img) if isinstance(img, np.ndarray) else img)
        if frame.dtype != torch.uint8:
            raise TypeError(f"RealESRNet.process: img is {frame.dtype}: the native pass takes the uint8 image (the reference divides whatever it gets by 255)")
        return ops.gpen_sr_image(frame.to(self.device)[None].contiguous(), self.srmodel, bgr=True)[0].cpu().numpy()
