"""Drop-in for the reference's ``swap_face_fine/face_vid2vid/modules/dense_motion.py``: ``DenseMotionNetwork`` with the reference's constructor signature and
``state_dict`` keys, its eval-mode forward on the HIP kernels of ``e4s2024_amd.ops_reenact`` (``csrc/conv3d.hip``, ``csrc/conv3d_k7.hip``,
``csrc/vid2vid.hip``).  The reference's own ``modules/generator.py`` imports the class from here and constructs it unchanged, so the generator checkpoint's
``dense_motion_network.`` keys load as before.  Neither ``sync_batchnorm`` nor ``modules.util`` is imported: in eval mode a synchronised BatchNorm is a plain
running-statistics one, folded into the convolutions here.

Forward only: training mode raises ``NotImplementedError``; ``num_kp + 1 > 32`` raises ``ValueError`` naming the argument."""
from e4s2024_amd import ops


class DenseMotionNetwork(ops.DenseMotionNetwork):
    """``DenseMotionNetwork(block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress, estimate_occlusion_map=False)``;
    ``forward(feature, kp_driving, kp_source)`` is ``ops.dense_motion_forward(feature, kp_driving, kp_source, self)``: ``{'mask', 'deformation'[,
    'occlusion_map']}``."""

    def __init__(self, block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress, estimate_occlusion_map=False):
        super().__init__(block_expansion, num_blocks, max_features, num_kp, feature_channel, reshape_depth, compress, estimate_occlusion_map)

    def forward(self, feature, kp_driving, kp_source):
        if self.training:
            raise NotImplementedError("DenseMotionNetwork: the native network is forward only, in eval mode: call .eval()")
        return ops.dense_motion_forward(feature, kp_driving, kp_source, self)
