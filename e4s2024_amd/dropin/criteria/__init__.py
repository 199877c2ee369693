"""Drop-in ``criteria`` package: ``criteria.lpips`` and ``criteria.id_loss`` are provided (the perceptual and identity terms of the PTI /
W-optimisation losses)."""
