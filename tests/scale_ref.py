"""The rule that puts a read on the model's pA scale (csrc/pg_fit.h, include/pgmove.h: pg_fit_calibrate), restated in Python floats, which
are IEEE doubles: every line is one rounded operation. Nothing here calls the product.

    g      = range / digitisation
    center = (a + offset) * g
    spread = (b * 1000.0) * g               (levels are in 1e-3 pA)
    use    = status == ok  and  center is finite  and  spread is finite and > 0

The collector then stores (pA - center) / spread per sample, a sample outside [pa_min, pa_max] zeroed first."""
import math

import numpy as np

OK = 0


def div(x, y):
    """x / y as IEEE does it: a zero divisor gives an infinity or a NaN, no exception."""
    return float(np.float64(x) / np.float64(y)) if y == 0 else x / y


def scale(status, a, b, digitisation, offset, rng):
    """(center, spread, use); (0.0, 0.0, 0) for a read that is not used."""
    if status != OK:
        return 0.0, 0.0, 0
    with np.errstate(all="ignore"):
        g = div(float(rng), float(digitisation))
        center = float(np.float64(a + offset) * np.float64(g))
        spread = float(np.float64(b * 1000.0) * np.float64(g))
    if not math.isfinite(center) or not math.isfinite(spread) or not spread > 0.0:
        return 0.0, 0.0, 0
    return center, spread, 1


def scaled(pa, center, spread, pa_min, pa_max):
    """What the collector stores for samples `pa` (float64 array, in pA) of one read."""
    x = np.where((pa < pa_min) | (pa > pa_max), 0.0, pa)
    return (x - center) / spread
