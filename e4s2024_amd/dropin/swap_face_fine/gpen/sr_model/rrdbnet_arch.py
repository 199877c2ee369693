"""Drop-in for the reference's ``swap_face_fine/gpen/sr_model/rrdbnet_arch.py``: ``RRDBNet`` with the reference's constructor signature and ``state_dict``
keys, its eval-mode forward on the HIP kernels of ``e4s2024_amd.ops_gpen_sr`` (the library's three-way split-bf16 convolutions, ``csrc/rrdb.hip``,
``csrc/gpen_sr.hip``).  The sibling ``arch_util`` module is not imported; basicsr is not needed.

Forward only: training mode raises ``NotImplementedError``.  Three colour channels in and out, ``num_grow_ch=32``, ``num_feat`` 32 or 64, ``scale`` 1, 2 or 4:
anything else raises ``ValueError`` naming it."""
from e4s2024_amd import ops


class RRDBNet(ops.GpenSRNet):
    """``RRDBNet(num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32)``; ``forward(x)`` is ``ops.gpen_sr_forward(x, self)``."""

    def __init__(self, num_in_ch, num_out_ch, scale=4, num_feat=64, num_block=23, num_grow_ch=32):
        if num_in_ch != 3 or num_out_ch != 3 or num_grow_ch != 32:
            raise ValueError(f"RRDBNet: num_in_ch {num_in_ch!r}, num_out_ch {num_out_ch!r}, num_grow_ch {num_grow_ch!r}: the native network is 3, 3, 32")
        super().__init__(num_block, num_feat, scale)

    def forward(self, x):
        if self.training:
            raise NotImplementedError("RRDBNet: the native network is forward only, in eval mode: call .eval()")
        return ops.gpen_sr_forward(x, self)
