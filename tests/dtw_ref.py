"""Float64 restatement of the reference's DTW (test infrastructure): utils/dtw.py::dtw with the cost np.abs(x - y), accelerated_dtw with
the cityblock cost, _traceback, and the moments scripts/pitch_dtw.py prints — vectorised along anti-diagonals (cell (i, j) needs
(i-1, j-1), (i, j-1), (i-1, j), all on earlier diagonals), so that a 2000 x 1000 pair takes well under a second.

The recurrence is D[i][j] = c(i, j) + min(D[i-1][j-1], s D[i][j-1], s D[i-1][j]): one rounding (the add) of an exact minimum of values that
are themselves fixed by earlier cells (s D is one rounding of a fixed value), so ANY evaluation order gives the same bits, and
tests/test_dtw_cpu.py holds this restatement to the reference's own output bit for bit.
"""
import math

import numpy as np


def cost_abs(x, y):
    """F = 1: |x_i - y_j| in the inputs' own precision (a float32 subtract for float32 tracks), widened to float64"""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    return np.abs(x[:, None] - y[None, :]).astype(np.float64)


def cost_cityblock(x, y):
    """scipy's cdist(x, y, 'cityblock'): the inputs widened to float64, the terms added with k ascending"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c = np.zeros((x.shape[0], y.shape[0]))
    for k in range(x.shape[1]):
        c += np.abs(x[:, k, None] - y[None, :, k])
    return c


def accumulate(C, w=None, s=1.0):
    """cost [N, M] -> D0 [(N + 1), (M + 1)] of utils/dtw.py (D0[1:, 1:] is the accumulated cost D1); w None = no band"""
    N, M = C.shape
    D0 = np.full((N + 1, M + 1), np.inf)
    D0[0, 0] = 0.0
    for d in range(N + M - 1):
        i = np.arange(max(0, d - M + 1), min(N - 1, d) + 1)
        j = d - i
        if w is not None:
            live = (j >= np.maximum(0, i - w)) & (j <= np.minimum(M, i + w))
            i, j = i[live], j[live]
        left, up = D0[i + 1, j], D0[i, j + 1]
        if s != 1.0:
            left, up = left * s, up * s
        D0[i + 1, j + 1] = C[i, j] + np.minimum(D0[i, j], np.minimum(left, up))
    return D0


def traceback(D0):
    """_traceback: from (N - 1, M - 1), the first minimum of the unscaled (diagonal, i - 1, j - 1); forward order"""
    i, j = D0.shape[0] - 2, D0.shape[1] - 2
    p, q = [i], [j]
    while i > 0 or j > 0:
        tb = int(np.argmin((D0[i, j], D0[i, j + 1], D0[i + 1, j])))
        if tb == 0:
            i, j = i - 1, j - 1
        elif tb == 1:
            i -= 1
        else:
            j -= 1
        p.append(i)
        q.append(j)
    return np.array(p[::-1], np.int32), np.array(q[::-1], np.int32)


def dtw(x, y, w=None, s=1.0):
    """-> distance, D1 [N, M], (p, q).  x, y 1-D: dtw(x, y, lambda a, b: np.abs(a - b), w=w, s=s); 2-D [T, F]: accelerated_dtw(x, y,
    'cityblock') (the reference gives that form neither a band nor a slope; here both apply to either).  For N = 1 or M = 1 the reference
    returns the one possible path without a traceback; the traceback gives the same."""
    x, y = np.asarray(x), np.asarray(y)
    C = cost_abs(x, y) if x.ndim == 1 else cost_cityblock(x, y)
    D0 = accumulate(C, w, s)
    return float(D0[-1, -1]), D0[1:, 1:], traceback(D0)


def valid_pair(N, M, N_ld, M_ld, w):
    return 1 <= N <= N_ld and 1 <= M <= M_ld and (w is None or w >= abs(N - M))


def moments(v):
    """mean, np.std, scipy.stats.skew(bias=True), scipy.stats.kurtosis(bias=True) of a 1-D track, by math.fsum (correctly rounded sums)"""
    v = [float(a) for a in np.asarray(v, np.float64).reshape(-1)]
    n = len(v)
    mean = math.fsum(v) / n
    d = [a - mean for a in v]
    m2, m3, m4 = (math.fsum(a ** k for a in d) / n for k in (2, 3, 4))
    if m2 == 0.0:
        return np.array([mean, 0.0, np.nan, np.nan])
    return np.array([mean, math.sqrt(m2), m3 / m2 ** 1.5, m4 / m2 ** 2 - 3.0])
