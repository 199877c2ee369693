"""Drop-in for the reference's ``swap_face_fine/gpen/face_detect/retinaface_detection.py``: ``RetinaFaceDetection`` with the reference's constructor and
``detect`` signature, the whole of ``detect`` — network, priors, decode, threshold, NMS — on the device (``ops.retinaface_detect``), returning numpy arrays as
the reference does.  Neither ``cv2`` nor ``torchvision`` is imported, nor the sibling ``data``, ``layers`` and ``utils`` packages.

Out of scope, each refused by name: ``detect_tensor`` (``NotImplementedError``), an image above 1500 on its longer side (the reference's ``cv2.resize``
branch; ``ValueError``), ``resize != 1`` (``ValueError``), an image that is not uint8 (``TypeError``: the reference takes a float frame as it is, and
quantising it here would change the detections without notice)."""
import os

import numpy as np
import torch

from e4s2024_amd import ops
from swap_face_fine.gpen.face_detect.facemodels.retinaface import RetinaFace

cfg_re50 = dict(ops.RETINAFACE_CFG_RE50)


class RetinaFaceDetection(object):
    def __init__(self, base_dir, device="cuda", network="RetinaFace-R50"):
        self.pretrained_path = os.path.join(base_dir, "weights", network + ".pth")
        self.device = device
        self.cfg = cfg_re50
        self.net = RetinaFace(cfg=self.cfg, phase="test")
        self.load_model()
        self.net = self.net.to(device)

    def remove_prefix(self, state_dict, prefix):
        """The mapping with a leading ``prefix`` (``module.`` of a DataParallel checkpoint) taken off the names that carry it."""
        n = len(prefix)
        return {(name[n:] if name[:n] == prefix else name): tensor for name, tensor in state_dict.items()}

    def load_model(self, load_to_cpu=False):
        pretrained = torch.load(self.pretrained_path, map_location=torch.device("cpu"))
        pretrained = self.remove_prefix(pretrained["state_dict"] if "state_dict" in pretrained else pretrained, "module.")
        if not set(pretrained) & set(self.net.state_dict()):
            raise AssertionError("load NONE from pretrained checkpoint")
        self.net.load_state_dict(pretrained, strict=False)
        self.net.eval()

    def detect(self, img_raw, resize=1, confidence_threshold=0.9, nms_threshold=0.4, top_k=5000, keep_top_k=750, save_image=False):
        """``img_raw``: a uint8 BGR image ``[H, W, 3]`` (numpy, or a tensor on any device).  Returns numpy ``(dets [n, 5], landms [n, 10])``."""
        if resize != 1:
            raise ValueError(f"RetinaFaceDetection.detect: resize {resize!r} is not implemented: the native detector is resize=1")
        img = torch.as_tensor(np.ascontiguousarray(img_raw) if isinstance(img_raw, np.ndarray) else img_raw)
        if img.dtype != torch.uint8:
            raise TypeError(f"RetinaFaceDetection.detect: img_raw is {img.dtype}: the native detector takes the uint8 frame (the reference subtracts the mean "
                            "from np.float32(img_raw) as it is, so a quantised float frame would give other detections)")
        dets, landms = ops.retinaface_detect(img.to(self.device)[None].contiguous(), self.net, True, confidence_threshold, nms_threshold, top_k, keep_top_k)[0]
        return dets.cpu().numpy(), landms.cpu().numpy()

    def detect_tensor(self, img, resize=1, confidence_threshold=0.9, nms_threshold=0.4, top_k=5000, keep_top_k=750, save_image=False):
        raise NotImplementedError("RetinaFaceDetection.detect_tensor is not implemented: it rescales the frame to 1000 on its longer side with F.interpolate; "
                                  "use detect (ops.retinaface_detect)")
