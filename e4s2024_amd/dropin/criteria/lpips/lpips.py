"""Drop-in for the reference's ``criteria/lpips/lpips.py``: ``LPIPS(net_type='alex', version='0.1')`` with the reference's state_dict,
whose ``forward`` runs the HIP kernels of ``e4s2024_amd.ops_lpips`` (forward and gradient with respect to both images).

Nothing is downloaded: the module starts without weights and refuses to run — here, and when handed to ``ops_lpips`` or the ``pti`` entry
points — until ``load_state_dict`` has filled it (``criteria.lpips.utils.convert_upstream_state_dict`` builds the state_dict from the
published files)."""
import torch
import torch.nn as nn

from criteria.lpips.networks import get_network, LinLayers
from e4s2024_amd import ops_lpips


class LPIPS(nn.Module):
    """Perceptual distance of two image batches in [-1, 1]: per tap of the feature network, the channel-normalised activations of the two
    images are compared, weighted per channel by ``lin`` and averaged over pixels; the five taps are summed and divided by the batch size.
    Only ``net_type='alex'`` and ``version='0.1'`` exist here."""

    def __init__(self, net_type: str = 'alex', version: str = '0.1'):
        if version != '0.1':
            raise ValueError(f"LPIPS version {version!r}: only '0.1' is provided")
        super().__init__()
        self.net = get_network(net_type)
        self.lin = LinLayers(self.net.n_channels_list)
        self._loaded = False

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        if set(ops_lpips.state_dict_keys()) <= set(state_dict.keys()):
            self._loaded = self.net._loaded = True
        return out

    def forward(self, x: torch.Tensor, y: torch.Tensor):
        return ops_lpips.lpips(x, y, self)
