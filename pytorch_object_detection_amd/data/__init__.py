"""Training-side input pipeline on the device: augment.collate_train_raw."""
from .augment import AugmentParams, collate_train_raw, sample_params  # noqa: F401
