"""Input pipeline on the device: augment.collate_train_raw, jpeg.JpegDecoder."""
from .augment import AugmentParams, collate_train_raw, sample_params  # noqa: F401
from .jpeg import JpegDecoder, decode_jpeg_batch  # noqa: F401
