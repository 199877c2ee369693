"""Drop-in for the reference's ``criteria/lpips`` package (LPIPS-AlexNet on the HIP kernels of ``e4s2024_amd.ops_lpips``)."""
