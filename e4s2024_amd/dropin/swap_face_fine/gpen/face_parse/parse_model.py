"""Drop-in for the reference's ``swap_face_fine/gpen/face_parse/parse_model.py``: ``ParseNet`` with the reference's constructor signature and ``state_dict``
keys, its eval-mode forward on the HIP kernels of ``e4s2024_amd.ops_parsenet`` (``csrc/parsenet.hip`` around the library's three-way split-bf16 convolutions),
and ``define_P``.  The reference's ``face_parsing.py`` picks it up through its import, so ``ParseNet-latest.pth`` loads as before and ``FaceParse.process`` /
``process_tensor`` run on the native network unchanged.  The sibling ``blocks`` module is not imported.

Forward only, ``norm_type='bn'`` and ``relu_type='LeakyReLU'`` (what ``FaceParse`` and ``define_P`` build): another type raises ``ValueError`` naming it, training
mode raises ``NotImplementedError``."""
import torch

from e4s2024_amd import ops


class ParseNet(ops.ParseNet):
    """``ParseNet(in_size=128, out_size=128, min_feat_size=32, base_ch=64, parsing_ch=19, res_depth=10, relu_type='prelu', norm_type='bn',
    ch_range=[32, 512])``; ``forward(x)`` is ``ops.parsenet_forward(x, self, with_image=True)``: ``(out_mask, out_img)``."""

    def __init__(self, in_size=128, out_size=128, min_feat_size=32, base_ch=64, parsing_ch=19, res_depth=10, relu_type="prelu", norm_type="bn",
                 ch_range=[32, 512]):
        super().__init__(in_size, out_size, min_feat_size, base_ch, parsing_ch, res_depth, relu_type, norm_type, tuple(ch_range))

    def forward(self, x):
        if self.training:
            raise NotImplementedError("ParseNet: the native network is forward only, in eval mode: call .eval()")
        return ops.parsenet_forward(x, self, with_image=True)


def define_P(in_size=512, out_size=512, min_feat_size=32, relu_type="LeakyReLU", isTrain=False, weight_path=None):
    net = ParseNet(in_size, out_size, min_feat_size, 64, 19, norm_type="bn", relu_type=relu_type, ch_range=[32, 256])
    if not isTrain:
        net.eval()
    if weight_path is not None:
        net.load_state_dict(torch.load(weight_path))
    return net
