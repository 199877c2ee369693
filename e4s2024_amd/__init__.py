"""e4s2024_amd — MI355X-native engine for the E4S regional-GAN-inversion hot path.

Layout
    csrc/        hand-written HIP kernels for gfx950 + the C ABI (include/e4s_hip.h) -> lib/libe4s_hip.so
    _lib.py      ctypes binding (fails loudly if the .so is missing: there is no CPU fallback)
    ops.py       tensor-level wrappers (torch = device memory + stream plumbing only)
    dropin/      files with the reference's module paths (``models/networks.py``, ``models/stylegan2/model.py``,
                 ``models/stylegan2/op/``, ``models/encoders/psp_encoders.py``, ``swap_face_fine/face_parsing/*.py``, ``criteria/lpips/*.py``,
                 ``criteria/id_loss.py``, ``criteria/face_parsing/face_parsing_loss.py``,
                 ``swap_face_fine/Blender/model_center/semantic_tools.py``, ``swap_face_fine/Blender/model_center/res_u_net.py``,
                 ``swap_face_fine/Blender/model_center/backbone.py``, ``swap_face_fine/realesr/image_infer.py``,
                 ``swap_face_fine/gpen/face_model/gpen_model.py``, ``swap_face_fine/gpen/face_parse/parse_model.py``,
                 ``swap_face_fine/gpen/face_detect/facemodels/retinaface.py``, ``swap_face_fine/gpen/face_detect/retinaface_detection.py``,
                 ``swap_face_fine/gpen/align_faces.py``, ``swap_face_fine/gpen/sr_model/rrdbnet_arch.py``,
                 ``swap_face_fine/gpen/sr_model/real_esrnet.py``, ``swap_face_fine/gpen/face_enhancement.py``,
                 ``swap_face_fine/face_vid2vid/modules/keypoint_detector.py``, ``swap_face_fine/face_inpainting.py``)
                 whose forward passes call the kernels
    runner.py    one-process-per-GPU frame sharding over torch.distributed (RCCL)
    seeded.py    seed-only weights/inputs used by tests, fixtures and the bench

``install()`` redirects exactly those module names to the drop-in files, leaving every other module of the reference
tree (``utils.*``, ``models.encoders.model_irse``, the rest of ``swap_face_fine.gpen`` …) to resolve as before::

    import e4s2024_amd; e4s2024_amd.install()
    from models.networks import Net3                      # the MI355X implementation
"""
from __future__ import annotations

import importlib.abc
import importlib.util
import os
import sys

__version__ = "0.1.0"

DROPIN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")

# module name -> path under dropin/ (packages end with /__init__.py)
OVERRIDES = {
    "models.networks": "models/networks.py",
    "models.stylegan2.model": "models/stylegan2/model.py",
    "models.stylegan2.op": "models/stylegan2/op/__init__.py",
    "models.stylegan2.op.fused_act": "models/stylegan2/op/fused_act.py",
    "models.stylegan2.op.upfirdn2d": "models/stylegan2/op/upfirdn2d.py",
    "models.stylegan2.op.conv2d_gradfix": "models/stylegan2/op/conv2d_gradfix.py",
    "models.encoders.psp_encoders": "models/encoders/psp_encoders.py",
    "swap_face_fine.face_parsing.model": "swap_face_fine/face_parsing/model.py",
    "swap_face_fine.face_parsing.resnet": "swap_face_fine/face_parsing/resnet.py",
    "swap_face_fine.face_parsing.face_parsing_demo": "swap_face_fine/face_parsing/face_parsing_demo.py",
}

# the training-loss networks the tuning loops take from the reference (``criteria.*``), redirected the same way
LOSS_OVERRIDES = {
    "criteria.lpips": "criteria/lpips/__init__.py",
    "criteria.lpips.lpips": "criteria/lpips/lpips.py",
    "criteria.lpips.networks": "criteria/lpips/networks.py",
    "criteria.lpips.utils": "criteria/lpips/utils.py",
    "criteria.id_loss": "criteria/id_loss.py",
    "criteria.face_parsing.face_parsing_loss": "criteria/face_parsing/face_parsing_loss.py",
}

# Blender recolouring, stage 1 (row f8): the helpers of the reference's Referencer.forward, with the semantic colour reference on the device.  The rest of
# swap_face_fine.Blender (referencer.py, blener.py, inference.py) stays the reference's own and runs on the three drop-ins
RECOLOR_OVERRIDES = {
    "swap_face_fine.Blender.model_center.semantic_tools": "swap_face_fine/Blender/model_center/semantic_tools.py",
}

# stage 2 (row f9): the Res-U-Net that turns the packages into the recoloured image, eval-mode forward on the device
RECOLOR_NET_OVERRIDES = {
    "swap_face_fine.Blender.model_center.res_u_net": "swap_face_fine/Blender/model_center/res_u_net.py",
}

# stage 3 (row f10): the feature networks (AdaptiveFeatureGenerator at the reference's default arguments, SmallFPN), eval-mode forward on the device
RECOLOR_FPN_OVERRIDES = {
    "swap_face_fine.Blender.model_center.backbone": "swap_face_fine/Blender/model_center/backbone.py",
}

# row f11: the Real-ESRGAN step behind the recolouring network (RealESRBatchInfer), without basicsr and cv2
ENHANCE_OVERRIDES = {
    "swap_face_fine.realesr.image_infer": "swap_face_fine/realesr/image_infer.py",
}

# row f12: GPEN face enhancement, stage 1: the generator behind FaceGAN (face_gan.py:14 imports FullGenerator and FullGenerator_SR from it).  The sibling ``op``
# package is not redirected: the drop-in does not import it
GPEN_OVERRIDES = {
    "swap_face_fine.gpen.face_model.gpen_model": "swap_face_fine/gpen/face_model/gpen_model.py",
}

# row f13: GPEN face enhancement, stage 2: the network behind FaceParse (face_parsing.py:11 imports ParseNet from it).  The sibling ``blocks`` module is not
# redirected: the drop-in does not import it
GPEN_PARSE_OVERRIDES = {
    "swap_face_fine.gpen.face_parse.parse_model": "swap_face_fine/gpen/face_parse/parse_model.py",
}


# row f14: GPEN face enhancement, stage 3: the detector behind FaceEnhancement (face_enhancement.py imports RetinaFaceDetection, which imports RetinaFace).  The
# siblings (``facemodels.net``, ``data``, ``layers``, ``utils``) are not redirected: the drop-ins do not import them
GPEN_DETECT_OVERRIDES = {
    "swap_face_fine.gpen.face_detect.facemodels.retinaface": "swap_face_fine/gpen/face_detect/facemodels/retinaface.py",
    "swap_face_fine.gpen.face_detect.retinaface_detection": "swap_face_fine/gpen/face_detect/retinaface_detection.py",
}

# row f15: GPEN face enhancement, stage 4: the 5-point alignment (face_enhancement.py imports warp_and_crop_face and get_reference_facial_points from it),
# without cv2 and skimage
GPEN_ALIGN_OVERRIDES = {
    "swap_face_fine.gpen.align_faces": "swap_face_fine/gpen/align_faces.py",
}

# row f16: GPEN face enhancement, stage 5: the RealESRNet pass (real_esrnet.py imports RRDBNet from rrdbnet_arch.py) and FaceEnhancement itself, without cv2,
# skimage and basicsr.  ``sr_model.arch_util`` is not redirected: the drop-ins do not import it
GPEN_SR_OVERRIDES = {
    "swap_face_fine.gpen.sr_model.rrdbnet_arch": "swap_face_fine/gpen/sr_model/rrdbnet_arch.py",
    "swap_face_fine.gpen.sr_model.real_esrnet": "swap_face_fine/gpen/sr_model/real_esrnet.py",
    "swap_face_fine.gpen.face_enhancement": "swap_face_fine/gpen/face_enhancement.py",
}

# row f17: face-vid2vid reenactment, stage 1: KPDetector and HEEstimator (drive_demo.py imports them from it).  ``sync_batchnorm`` and ``modules.util`` are not
# redirected: the drop-in imports neither
REENACT_KP_OVERRIDES = {
    "swap_face_fine.face_vid2vid.modules.keypoint_detector": "swap_face_fine/face_vid2vid/modules/keypoint_detector.py",
}

# row f18: face-vid2vid reenactment, stage 2: DenseMotionNetwork (the reference's own modules/generator.py imports it from there and constructs it unchanged).
# ``modules.util`` is still the reference's: the generator's other blocks come from it
REENACT_MOTION_OVERRIDES = {
    "swap_face_fine.face_vid2vid.modules.dense_motion": "swap_face_fine/face_vid2vid/modules/dense_motion.py",
}

# row f25: face inpainting, stage 1: ``inpainting(face_img, mask)`` (Face_swap_with_two_imgs.py imports it from there).  ``swap_face_fine.gcfsr_arch`` is not
# redirected: the drop-in does not import it (``ops.FaceInpainting`` has its keys), and it needs basicsr and the JIT ops
INPAINT_OVERRIDES = {
    "swap_face_fine.face_inpainting": "swap_face_fine/face_inpainting.py",
}


def _redirected():
    return {**OVERRIDES, **LOSS_OVERRIDES, **RECOLOR_OVERRIDES, **RECOLOR_NET_OVERRIDES, **RECOLOR_FPN_OVERRIDES, **ENHANCE_OVERRIDES, **GPEN_OVERRIDES,
            **GPEN_PARSE_OVERRIDES, **GPEN_DETECT_OVERRIDES, **GPEN_ALIGN_OVERRIDES, **GPEN_SR_OVERRIDES, **REENACT_KP_OVERRIDES, **REENACT_MOTION_OVERRIDES}


def _all_redirected():
    """Every module name ``install`` redirects: ``_redirected()``, the network modules of rows up to f18 (row f21's test pins that table's size: its stage added
    no drop-in), and the tables of later rows, which redirect a caller-level entry (``INPAINT_OVERRIDES``)."""
    return {**_redirected(), **INPAINT_OVERRIDES}


class _DropinFinder(importlib.abc.MetaPathFinder):
    def find_spec(self, fullname, path=None, target=None):
        rel = _all_redirected().get(fullname)
        if rel is None:
            return None
        file = os.path.join(DROPIN_DIR, rel)
        is_pkg = rel.endswith("__init__.py")
        return importlib.util.spec_from_file_location(fullname, file, submodule_search_locations=[os.path.dirname(file)] if is_pkg else None)


_finder = None


def install(force: bool = False) -> str:
    """Redirect the hot-path module names (``OVERRIDES``), the loss networks' (``LOSS_OVERRIDES``) and the recolouring modules' (``RECOLOR_OVERRIDES``,
    ``RECOLOR_NET_OVERRIDES``, ``RECOLOR_FPN_OVERRIDES``), the Real-ESRGAN wrapper's (``ENHANCE_OVERRIDES``), GPEN's generator (``GPEN_OVERRIDES``), GPEN's
    face-mask network (``GPEN_PARSE_OVERRIDES``), GPEN's face detector (``GPEN_DETECT_OVERRIDES``), GPEN's 5-point alignment (``GPEN_ALIGN_OVERRIDES``) and
    GPEN's RealESRNet pass with ``FaceEnhancement`` itself (``GPEN_SR_OVERRIDES``) and face-vid2vid's keypoint detector and head-pose estimator
    (``REENACT_KP_OVERRIDES``) and dense-motion network (``REENACT_MOTION_OVERRIDES``) and the face-inpainting entry ``inpainting(face_img, mask)``
    (``INPAINT_OVERRIDES``) to the drop-in files.

    Parent packages (``models``, ``models.encoders``, ``swap_face_fine`` …) resolve to whatever is first on ``sys.path`` —
    the reference tree when the engine is used inside it, otherwise the empty packages under ``dropin/`` (appended at the
    END of ``sys.path``).  If an overridden module was already imported from elsewhere, raise unless ``force`` (then it is
    purged so the next import takes the drop-in)."""
    global _finder
    stale = [m for m in _all_redirected() if m in sys.modules
             and not (getattr(sys.modules[m], "__file__", None) or "").startswith(DROPIN_DIR)]
    if stale:
        if not force:
            raise RuntimeError(f"{stale} already imported from elsewhere; call e4s2024_amd.install() first, or install(force=True)")
        for m in list(sys.modules):
            if any(m == s or m.startswith(s + ".") for s in stale):
                del sys.modules[m]
    if _finder is None:
        _finder = _DropinFinder()
        sys.meta_path.insert(0, _finder)
    if DROPIN_DIR not in sys.path:
        sys.path.append(DROPIN_DIR)
    return DROPIN_DIR


def invalidate_weight_caches(module) -> int:
    """See ``ops.invalidate_weight_caches``: forget the prepared weight copies under ``module`` after raw ``p.data`` writes."""
    from . import ops
    return ops.invalidate_weight_caches(module)


def uninstall() -> None:
    global _finder
    if _finder is not None and _finder in sys.meta_path:
        sys.meta_path.remove(_finder)
    _finder = None
    if DROPIN_DIR in sys.path:
        sys.path.remove(DROPIN_DIR)
    for m in list(sys.modules):
        if any(m == s or m.startswith(s + ".") for s in _all_redirected()):
            del sys.modules[m]
