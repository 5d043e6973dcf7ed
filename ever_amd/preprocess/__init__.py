"""Input preparation and augmentation on tensors (the reference's `ever.preprocess`): `function`, `thcomm`, `thsegm`.

Not covered: the reference's `albu`, `segm` and `comm` modules, which need albumentations or work on numpy / PIL images
(DESIGN §7)."""
from . import function, thcomm, thsegm  # noqa: F401
