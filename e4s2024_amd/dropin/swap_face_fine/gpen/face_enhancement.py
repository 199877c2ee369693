"""Drop-in for the reference's ``swap_face_fine/gpen/face_enhancement.py``: ``FaceEnhancement`` with the reference's constructor and ``process(img, aligned)``,
numpy BGR uint8 in, numpy results out, the whole of ``process`` on the device (``pipeline.gpen_face_enhancement``): the RealESRNet pass, the resize of the frame
to its size, the detector, the 5-point crops, the generator, the ParseNet mask, its feathering and the paste.  cv2, skimage and basicsr are not imported, nor the
reference's ``face_gan.py`` and ``face_parsing.py`` (both import cv2): the generator and the ParseNet are built and loaded here as those two files do it, from
``<base_dir>/weights/<model>.pth`` and ``<base_dir>/weights/ParseNet-latest.pth``.

Out of scope, each refused by name: ``in_size != out_size`` (``FullGenerator_SR`` and the ``cv2.resize`` of the enhanced face), an aligned face that is not
``in_size`` square (the reference resizes it with cv2).  The reference's ``img_sr is None`` branch (its RealESRNet swallowed an error of the network) has no
counterpart: an error is raised."""
import os

import numpy as np
import torch

from e4s2024_amd import ops, pipeline
from swap_face_fine.gpen.align_faces import get_reference_facial_points
from swap_face_fine.gpen.face_detect.retinaface_detection import RetinaFaceDetection
from swap_face_fine.gpen.face_model.gpen_model import FullGenerator
from swap_face_fine.gpen.face_parse.parse_model import ParseNet
from swap_face_fine.gpen.sr_model.real_esrnet import RealESRNet


def _load_generator(base_dir, in_size, model, channel_multiplier, narrow, key, device):
    """``FaceGAN.load_model`` (face_model/face_gan.py:27-36)."""
    net = FullGenerator(in_size, 512, 8, channel_multiplier, narrow=narrow, device=device)
    pretrained = torch.load(os.path.join(base_dir, "weights", model + ".pth"), map_location=torch.device("cpu"))
    net.load_state_dict(pretrained if key is None else pretrained[key])
    return net.to(device).eval()


def _load_parsenet(base_dir, device, model="ParseNet-latest"):
    """``FaceParse.load_model`` (face_parse/face_parsing.py:33-37)."""
    net = ParseNet(512, 512, 32, 64, 19, norm_type="bn", relu_type="LeakyReLU", ch_range=[32, 256])
    net.load_state_dict(torch.load(os.path.join(base_dir, "weights", model + ".pth"), map_location=torch.device("cpu")))
    return net.to(device).eval()


class FaceEnhancement(object):
    def __init__(self, base_dir="./", in_size=512, out_size=None, model=None, use_sr=True, sr_model=None, sr_scale=2, channel_multiplier=2, narrow=1, key=None,
                 device="cuda"):
        if out_size is not None and out_size != in_size:
            raise NotImplementedError(f"FaceEnhancement: out_size {out_size!r} != in_size {in_size!r} (FullGenerator_SR) is not implemented")
        self.facedetector = RetinaFaceDetection(base_dir, device)
        self.facegan = _load_generator(base_dir, in_size, model, channel_multiplier, narrow, key, device)
        self.srmodel = RealESRNet(base_dir, sr_model, sr_scale, device=device)
        self.faceparser = _load_parsenet(base_dir, device)
        self._configure(in_size, use_sr, device)

    @classmethod
    def from_networks(cls, detector, gpen, parsenet, sr, use_sr=True, device="cuda"):
        """A ``FaceEnhancement`` around networks that are already loaded (as ``pipeline.gpen_face_enhancement`` takes them); ``sr`` may be None without
        ``use_sr``."""
        self = object.__new__(cls)
        self.facedetector, self.facegan, self.faceparser, self.srmodel = detector, gpen, parsenet, sr
        self._configure(int(gpen.size), use_sr, device)
        return self

    def _configure(self, in_size, use_sr, device):
        self.device = device
        self.use_sr = use_sr
        self.in_size = self.out_size = in_size
        self.threshold = ops.GPEN_PASTE_DEFAULTS["threshold"]
        self.reference_5pts = get_reference_facial_points((in_size, in_size), 0.25, (0, 0), True)

    def _networks(self):
        sr = getattr(self.srmodel, "srmodel", self.srmodel) if self.use_sr else None
        return getattr(self.facedetector, "net", self.facedetector), self.facegan, self.faceparser, sr

    def process(self, img, aligned=False):
        """``img``: a uint8 BGR image ``[H, W, 3]``.  Returns ``(img, orig_faces, enhanced_faces)`` as the reference does: BGR uint8 numpy arrays."""
        frame = torch.as_tensor(np.ascontiguousarray(img))
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3:
            raise TypeError(f"FaceEnhancement.process: img is {frame.dtype} {tuple(frame.shape)}: expected a uint8 [H, W, 3] BGR image")
        detector, gpen, parsenet, sr = self._networks()
        rgb = frame.to(self.device).flip(2)[None].contiguous()
        out, orig, enhanced = pipeline.gpen_face_enhancement(detector, gpen, parsenet, sr, rgb, aligned=aligned, return_faces=True)
        to_bgr = lambda t: t.flip(-1).cpu().numpy()                           # noqa: E731
        if aligned:
            return to_bgr(out[0]), [img], [to_bgr(enhanced[0][0])]
        return to_bgr(out[0]), [to_bgr(f) for f in orig[0]], [to_bgr(f) for f in enhanced[0]]
