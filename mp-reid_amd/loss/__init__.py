"""Losses of the reference that run on the GPU here: ``supcontrast.SupConLoss`` (stage-1 prompt learning), and the stage-2 head's
``softmax_loss.CrossEntropyLabelSmooth``, ``triplet_loss.TripletLoss`` and ``make_loss.make_loss``."""
