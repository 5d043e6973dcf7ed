from . import bigimage, transform  # noqa: F401
