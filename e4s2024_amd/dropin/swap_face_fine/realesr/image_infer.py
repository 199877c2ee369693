"""Drop-in for the reference's ``swap_face_fine/realesr/image_infer.py``: ``RealESRBatchInfer`` with the reference's argument-less constructor, the same
checkpoint file and the same two methods, the network on the HIP kernels of ``e4s2024_amd.ops_recolor`` (``csrc/conv.hip``, ``csrc/rrdb.hip``).  It needs
neither basicsr nor cv2: the architecture is ``ops.RRDBNet``, which has basicsr's ``state_dict`` keys, so ``RealESRGAN_x4plus.pth`` loads with
``strict=True`` as before.

The reference finds its checkpoint relative to its own file, three directories up from ``swap_face_fine/realesr/``: a ``ReliableSwap`` directory beside
the reference tree.  This file lives elsewhere, so ``checkpoint_path`` starts from the ``swap_face_fine`` package that is first on ``sys.path`` — the
reference's, when the engine is used inside it (``e4s2024_amd.install`` puts the drop-in packages last) — and from this file's own package otherwise."""
import importlib.util
import os
import types

import numpy as np
import torch
from PIL import Image

from e4s2024_amd import ops, pipeline

CHECKPOINT = os.path.join("ReliableSwap", "pretrained", "third_party", "RealESRGAN", "RealESRGAN_x4plus.pth")


def checkpoint_path() -> str:
    """Where the reference looks for ``RealESRGAN_x4plus.pth``: ``<swap_face_fine>/realesr/../../../ReliableSwap/pretrained/third_party/RealESRGAN/``."""
    spec = importlib.util.find_spec("swap_face_fine")
    roots = list(spec.submodule_search_locations or []) if spec is not None else []
    package = roots[0] if roots else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.normpath(os.path.join(package, "realesr", "..", "..", "..", CHECKPOINT))


class RealESRBatchInfer:
    def __init__(self):
        self.device = "cuda:0"
        self.args = types.SimpleNamespace(model_name="RealESRGAN_x4plus", model_path=checkpoint_path())
        checkpoint = torch.load(self.args.model_path, map_location="cpu")
        key = next((k for k in ("params_ema", "params") if k in checkpoint), None)                # the smoothed weights where the file has them
        if key is None:
            raise KeyError(f"RealESRBatchInfer: {self.args.model_path} has neither 'params_ema' nor 'params'")
        self.model = ops.RRDBNet(num_block=23).eval()
        self.model.load_state_dict(checkpoint[key], strict=True)
        self.model.to(self.device)

    @torch.no_grad()
    def infer_batch(self, source_tensor: torch.Tensor, out_hw: tuple = None):
        """Float ``[B, 3, H, W]`` in [-1, 1] to ``[B, 3, *out_hw]`` in [-1, 1] (``pipeline.realesr_infer_batch``)."""
        return pipeline.realesr_infer_batch(self.model, source_tensor, out_hw)

    def infer_image(self, img: Image):
        """A PIL RGB image of any size to the enhanced 1024 x 1024 PIL image (``pipeline.realesr_infer_image``)."""
        frame = torch.from_numpy(np.array(img)).to(self.device)[None]
        return Image.fromarray(pipeline.realesr_infer_image(self.model, frame)[0].cpu().numpy())
