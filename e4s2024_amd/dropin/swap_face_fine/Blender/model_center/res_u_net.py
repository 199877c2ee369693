"""Drop-in for the reference's ``swap_face_fine/Blender/model_center/res_u_net.py``: the Res-U-Net of the recolouring network with the reference's class
names, constructor arguments and ``state_dict`` keys, its eval-mode forward on the HIP kernels of ``e4s2024_amd.ops_recolor`` (``csrc/conv.hip``,
``csrc/resunet.hip``).  The reference's ``blener.py`` picks it up through its relative import, so ``latest_netG.pth`` loads as before.

Forward only: in training mode (BatchNorm on batch statistics, gradients) ``ResUNet.forward`` raises ``NotImplementedError``.  ``ResBlock`` and
``InputEncodeLayer`` on their own are plain PyTorch modules."""
from e4s2024_amd import ops
from e4s2024_amd.ops_recolor import _Block


class InputEncodeLayer(_Block):
    def __init__(self, ch_in, ch_out):
        super().__init__(ch_in, ch_out, first=True)


class ResBlock(_Block):
    def __init__(self, ch_in, ch_out, stride=1):
        super().__init__(ch_in, ch_out, stride)


class ResUNet(ops.ResUNet):
    """``ResUNet(args)``: width 16 with ``args.small_FPN``, else 64.  ``forward(pkgs)`` is ``ops.blender_unet(pkgs, self)``."""

    def __init__(self, args):
        super().__init__(16 if args.small_FPN else 64)

    def forward(self, pkgs):
        if self.training:
            raise NotImplementedError("ResUNet: the native Res-U-Net is forward only, in eval mode (BatchNorm on running statistics): call .eval()")
        return ops.blender_unet(pkgs, self)
