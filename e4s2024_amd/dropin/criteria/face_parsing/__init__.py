"""Drop-in ``criteria.face_parsing`` package: ``face_parsing_loss.FaceParsingLoss`` is provided."""
