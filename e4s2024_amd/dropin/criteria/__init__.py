"""Drop-in ``criteria`` package: only ``criteria.lpips`` is provided (the perceptual term of the PTI / W-optimisation losses)."""
