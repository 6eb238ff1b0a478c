"""Input pipeline on the device: augment.collate_train_raw, augment.collate_train_mosaic,
jpeg.JpegDecoder."""
from .augment import AugmentParams, MosaicParams, collate_train_mosaic, collate_train_raw, sample_mosaic, sample_params  # noqa: F401
from .jpeg import JpegDecoder, decode_jpeg_batch  # noqa: F401
