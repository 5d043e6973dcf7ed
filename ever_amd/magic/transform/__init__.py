from . import segm, tta  # noqa: F401
