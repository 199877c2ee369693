"""Drop-in for the reference's ``swap_face_fine/gpen/face_model/gpen_model.py``: ``FullGenerator`` with the reference's constructor signature and
``state_dict`` keys, its eval-mode forward on the HIP kernels of ``e4s2024_amd.ops_gpen`` (``csrc/gpen.hip`` and the library's modulated convolutions).  The
reference's ``face_gan.py`` picks it up through its import, so ``GPEN-BFR-512.pth`` loads as before.  The sibling ``op`` package is not imported.

Forward only, one style per sample, concatenated noise: training mode, ``truncation < 1``, ``inject_index``, ``input_is_latent=True`` and ``isconcat=False``
raise ``NotImplementedError``.  ``FullGenerator_SR``, ``Generator`` and ``Discriminator`` exist as names (``face_gan.py`` imports the first); constructing one
raises ``NotImplementedError``."""
from e4s2024_amd import ops


class FullGenerator(ops.GPEN):
    """``FullGenerator(size, style_dim, n_mlp, channel_multiplier=2, blur_kernel=[1, 3, 3, 1], lr_mlp=0.01, isconcat=True, narrow=1, device='cpu')``;
    ``forward(inputs)`` is ``ops.gpen_forward(inputs, self)``: ``(image, None)``, or ``(image, latent)`` with ``return_latents``."""

    def __init__(self, size, style_dim, n_mlp, channel_multiplier=2, blur_kernel=[1, 3, 3, 1], lr_mlp=0.01, isconcat=True, narrow=1, device="cpu"):
        if not isconcat:
            raise NotImplementedError("FullGenerator: isconcat=False (additive noise) is not implemented; GPEN's checkpoints concatenate")
        if list(blur_kernel) != [1, 3, 3, 1] or lr_mlp != 0.01:
            raise NotImplementedError(f"FullGenerator: blur_kernel {blur_kernel!r} / lr_mlp {lr_mlp!r}: only [1, 3, 3, 1] and 0.01 are implemented")
        super().__init__(size, style_dim, n_mlp, channel_multiplier, narrow)
        self.device = device

    def forward(self, inputs, return_latents=False, inject_index=None, truncation=1, truncation_latent=None, input_is_latent=False):
        if self.training:
            raise NotImplementedError("FullGenerator: the native generator is forward only, in eval mode: call .eval()")
        if truncation < 1:
            raise NotImplementedError("FullGenerator: truncation < 1 is not implemented")
        if inject_index is not None:
            raise NotImplementedError("FullGenerator: inject_index (style mixing) is not implemented: the encoder gives one style per sample")
        if input_is_latent:
            raise NotImplementedError("FullGenerator: input_is_latent=True is not implemented")
        return ops.gpen_forward(inputs, self, return_latents=return_latents)


def _not_implemented(name, why):
    class _Stub:
        def __init__(self, *args, **kwargs):
            raise NotImplementedError(f"{name}: {why}")
    _Stub.__name__ = _Stub.__qualname__ = name
    return _Stub


FullGenerator_SR = _not_implemented("FullGenerator_SR", "the super-resolution variant of GPEN's generator is not implemented (FaceGAN's default, is SR off, uses FullGenerator)")
Generator = _not_implemented("Generator", "the bare synthesis network is not implemented on its own; FullGenerator holds it as .generator")
Discriminator = _not_implemented("Discriminator", "training is not implemented")
