"""Drop-in for the reference's ``swap_face_fine/face_inpainting.py``: ``inpainting(face_img, mask)`` with the reference's signature (a PIL RGB face and a numpy
mask in, the inpainted 256 x 256 PIL image out), the whole of it on the HIP kernels of ``e4s2024_amd.ops_inpaint`` (``pipeline.inpaint_faces``: Pillow's BICUBIC
resize, the support of ``cv2.resize`` on the mask, the network, the composite).  It needs neither cv2 nor basicsr, and it runs on a current numpy (the
reference's ``mask.astype(np.float)`` does not).  ``gcfsr_arch.py`` has no drop-in: the architecture is ``ops.FaceInpainting``, which has the reference's
``state_dict`` keys, so ``net_g_50000.pth``'s ``params_ema`` loads with ``strict=True`` as before.

The reference loads its checkpoint when the module is imported; here that happens on the first call (``model()``), from the same relative ``model_path``, so
that importing the module needs neither the file nor a device.  Every call draws fresh noise, as the reference's does."""
import numpy as np
import torch
from PIL import Image

from e4s2024_amd import ops, pipeline

model_path = './pretrained/inpainting/net_g_50000.pth'
device = "cuda:0"
_model = None


def model():
    """The network with the checkpoint's smoothed weights, loaded on first use."""
    global _model
    if _model is None:
        net = ops.FaceInpainting(out_size=256).eval()
        net.load_state_dict(torch.load(model_path, map_location="cpu")['params_ema'], strict=True)
        _model = net.to(device)
    return _model


def inpainting(face_img, mask):
    faces = torch.from_numpy(np.ascontiguousarray(np.array(face_img.convert("RGB")))).to(device)[None]
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError(f"inpainting: mask is a 2-D array, got shape {m.shape}")
    hole = torch.from_numpy(np.ascontiguousarray(m if m.dtype == np.uint8 else m.astype(np.float32))).to(device)[None]
    return Image.fromarray(pipeline.inpaint_faces(model(), faces, hole)[0].cpu().numpy())
