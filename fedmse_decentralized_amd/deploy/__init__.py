from .detector import Detector, score_rows_numpy  # noqa: F401
