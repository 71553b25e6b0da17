from .image import ImageClassifier  # noqa: F401
