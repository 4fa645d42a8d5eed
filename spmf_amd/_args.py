"""The two argument checks that the analysis calls and their helper modules share; each raises ValueError with the
call's ``name`` in front."""
import numpy as np


def integer(name, what, value, lo=None, hi=None):
    """``value`` as an int: an integer, not a bool, with ``lo`` <= value <= ``hi`` where they are given."""
    ok = not isinstance(value, bool) and isinstance(value, (int, np.integer))
    if not ok or (lo is not None and int(value) < lo) or (hi is not None and int(value) > hi):
        bounds = "" if lo is None else f" >= {lo}" if hi is None else f" in {lo}..{hi}"
        raise ValueError(f"{name}: {what} must be an integer{bounds}, got {value!r}")
    return int(value)


def number(name, what, value, positive=False, hi=None):
    """``value`` as a float: a finite number, not a bool, >= 0 (> 0 with ``positive``) and at most ``hi``."""
    ok = isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool)
    if not ok or not np.isfinite(value) or value < 0 or (hi is not None and value > hi) or (positive and value <= 0):
        raise ValueError(f"{name}: {what} must be a finite number {'> 0' if positive else '>= 0'}, got {value!r}")
    return float(value)
