"""Drop-in for the reference's ``swap_face_fine/face_vid2vid/modules/keypoint_detector.py``: ``KPDetector`` and ``HEEstimator`` with the reference's constructor
signatures and ``state_dict`` keys, their eval-mode forwards on the HIP kernels of ``e4s2024_amd.ops_reenact`` (``csrc/conv3d.hip``, ``csrc/vid2vid.hip`` and
the library's 2-D convolutions).  ``drive_demo.load_checkpoints`` picks them up through its import, so ``checkpoint['kp_detector']`` and
``checkpoint['he_estimator']`` load as before.  Neither ``sync_batchnorm`` nor ``modules.util`` is imported: in eval mode a synchronised BatchNorm is a plain
running-statistics one, folded into the convolutions here.

Forward only: training mode raises ``NotImplementedError``; ``single_jacobian_map=True``, a ``scale_factor`` whose inverse is no integer and a
``reshape_channel`` that does not fit ``reshape_depth`` raise ``ValueError`` naming the argument."""
from e4s2024_amd import ops


class KPDetector(ops.KPDetector):
    """``KPDetector(block_expansion, feature_channel, num_kp, image_channel, max_features, reshape_channel, reshape_depth, num_blocks, temperature,
    estimate_jacobian=False, scale_factor=1, single_jacobian_map=False)``; ``forward(x)`` is ``ops.kp_detector_forward(x, self)``: ``{'value'[, 'jacobian']}``."""

    def __init__(self, block_expansion, feature_channel, num_kp, image_channel, max_features, reshape_channel, reshape_depth, num_blocks, temperature,
                 estimate_jacobian=False, scale_factor=1, single_jacobian_map=False):
        super().__init__(block_expansion, feature_channel, num_kp, image_channel, max_features, reshape_channel, reshape_depth, num_blocks, temperature,
                         estimate_jacobian, scale_factor, single_jacobian_map)

    def forward(self, x):
        if self.training:
            raise NotImplementedError("KPDetector: the native network is forward only, in eval mode: call .eval()")
        return ops.kp_detector_forward(x, self)


class HEEstimator(ops.HEEstimator):
    """``HEEstimator(block_expansion, feature_channel, num_kp, image_channel, max_features, num_bins=66, estimate_jacobian=True)``; ``forward(x)`` is
    ``ops.he_estimator_forward(x, self)``: the five-key dict, head names crossed as the reference crosses them."""

    def __init__(self, block_expansion, feature_channel, num_kp, image_channel, max_features, num_bins=66, estimate_jacobian=True):
        super().__init__(block_expansion, feature_channel, num_kp, image_channel, max_features, num_bins, estimate_jacobian)

    def forward(self, x):
        if self.training:
            raise NotImplementedError("HEEstimator: the native network is forward only, in eval mode: call .eval()")
        return ops.he_estimator_forward(x, self)
