"""Drop-in for the reference's ``swap_face_fine/gpen/face_detect/facemodels/retinaface.py``: ``RetinaFace(cfg, phase)`` with the reference's constructor
signature and ``state_dict`` keys, its eval-mode forward on the HIP kernels of ``e4s2024_amd.ops_retinaface`` (``csrc/retinaface.hip`` around the library's
convolutions).  ``torchvision`` is not imported: the ResNet-50 body is written out.  The sibling ``net`` module is not imported.

Forward only, ``cfg['name'] == 'Resnet50'`` and ``phase='test'``: anything else raises ``ValueError`` naming it, training mode raises ``NotImplementedError``."""
from e4s2024_amd import ops


class RetinaFace(ops.RetinaFace):
    """``RetinaFace(cfg=None, phase='train')``; ``forward(x)`` is ``ops.retinaface_forward(x, self)``: ``(loc, softmax conf, landms)``."""

    def __init__(self, cfg=None, phase="train"):
        super().__init__(cfg, phase)

    def forward(self, inputs):
        if self.training:
            raise NotImplementedError("RetinaFace: the native network is forward only, in eval mode: call .eval()")
        return ops.retinaface_forward(inputs, self)
