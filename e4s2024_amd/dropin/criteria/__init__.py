"""Drop-in ``criteria`` package: ``criteria.lpips``, ``criteria.id_loss`` and ``criteria.face_parsing.face_parsing_loss`` are provided (the perceptual,
identity and face-parsing terms of the PTI / W-optimisation losses)."""
