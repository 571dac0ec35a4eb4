"""Losses of the reference that run on the GPU here: ``supcontrast.SupConLoss`` (stage-1 prompt learning)."""
