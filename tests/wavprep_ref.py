"""Float64 restatements of the two waveform-conditioning units, in the arithmetic include/dicttts_hip.h specifies
(DTTS_OUT_RESAMPLE: resampy 0.4.2's resample_f; DTTS_OUT_LOUDNESS: pyloudnorm 0.1.1's meter and normalisation with the reference's peak
rule).  Neither library is on the build machine: these restatements ARE the definition the device is held to, and tests/test_wavprep_cpu.py
anchors them physically (sines against the analytic sine, the 997 Hz conformance tone, the BS.1770 coefficient table).

Every output sample / filter state is computed by a sequential loop with one accumulator, in the specified order.  The resampler's loop runs
over the taps and is vectorised ACROSS outputs (each output still sees its own taps one after the other); ``resample_scalar`` is the same
thing as two plain nested loops, for the test that they agree bit for bit.

The reference-rounding variants model what the libraries themselves round: resampy adds every tap into a float32 y[t]
(``per_tap_f32=True``); pyloudnorm stores each filter stage back into the float32 input array and squares and sums that
(``f32_storage=True``).
"""
import math

import numpy as np

from dict_tts_amd import wavprep as W


# ---------------------------------------------------------------- resampler
def resample_geometry(L, sr_in, sr_out, n_win, num_table):
    ratio = float(sr_out) / float(sr_in)
    lr = float(L) * ratio
    scale = min(1.0, ratio)
    return dict(ratio=ratio, n_out=int(lr), out_len=int(math.ceil(lr)), scale=scale, inc=1.0 / ratio, index_step=int(scale * num_table),
                tscale=ratio if ratio < 1.0 else 1.0)


def delta_table(win):
    d = np.zeros_like(win)
    d[:-1] = win[1:] - win[:-1]
    return d


def resample(x, sr_in, sr_out, win, num_table, per_tap_f32=False):
    """x float32 [L] -> dict: y64 f64 [n_out] (the accumulators; with per_tap_f32 the float32 running values widened), out f32 [out_len]
    (rounded once, fix_length's zero appended), absum f64 [n_out] = sum |w x| over the taps, taps i64 [n_out], n_out, out_len"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 1
    L, n_win = len(x), len(win)
    g = resample_geometry(L, sr_in, sr_out, n_win, num_table)
    n_out, step, scale = g["n_out"], g["index_step"], g["scale"]
    ws, ds = win * g["tscale"], delta_table(win) * g["tscale"]
    xd = x.astype(np.float64)
    t = np.arange(n_out, dtype=np.float64)
    tr = t * g["inc"]
    n = tr.astype(np.int64)
    frac = scale * (tr - n)
    acc = np.zeros(n_out, np.float32 if per_tap_f32 else np.float64)
    absum = np.zeros(n_out)
    taps = np.zeros(n_out, np.int64)
    for wing in (0, 1):
        f = (frac if wing == 0 else scale - frac) * float(num_table)
        off = f.astype(np.int64)
        eta = f - off
        cnt = np.minimum(n + 1 if wing == 0 else L - n - 1, (n_win - off) // step)
        taps += np.maximum(cnt, 0)
        for i in range(int(cnt.max()) if n_out else 0):
            m = np.nonzero(cnt > i)[0]
            idx = off[m] + i * step
            w = ws[idx] + eta[m] * ds[idx]
            p = w * xd[n[m] - i if wing == 0 else n[m] + i + 1]
            acc[m] = (acc[m].astype(np.float64) + p).astype(acc.dtype)
            absum[m] += np.abs(p)
    out = np.zeros(g["out_len"], np.float32)
    out[:n_out] = acc.astype(np.float32)
    return dict(y64=acc.astype(np.float64), out=out, absum=absum, taps=taps, n_out=n_out, out_len=g["out_len"], index_step=step)


def resample_scalar(x, sr_in, sr_out, win, num_table):
    """the specification as two nested loops over plain Python floats -> y64 [n_out]"""
    L, n_win = len(x), len(win)
    g = resample_geometry(L, sr_in, sr_out, n_win, num_table)
    step, scale, inc, ts = g["index_step"], g["scale"], g["inc"], g["tscale"]
    delta = delta_table(win)
    ws, ds = [float(v) * ts for v in win], [float(v) * ts for v in delta]
    xs = [float(v) for v in x]
    y = np.zeros(g["n_out"])
    for t in range(g["n_out"]):
        tr = t * inc
        n = int(tr)
        frac = scale * (tr - n)
        f = frac * num_table
        off = int(f)
        eta = f - off
        acc = 0.0
        for i in range(min(n + 1, (n_win - off) // step)):
            acc += (ws[off + i * step] + eta * ds[off + i * step]) * xs[n - i]
        f = (scale - frac) * num_table
        off = int(f)
        eta = f - off
        for k in range(min(L - n - 1, (n_win - off) // step)):
            acc += (ws[off + k * step] + eta * ds[off + k * step]) * xs[n + k + 1]
        y[t] = acc
    return y


# ---------------------------------------------------------------- loudness
def biquad(b, a, x, f32_out=False):
    """scipy.signal.lfilter's transposed direct form II from a zero state: y = z1 + b0 x; z1 = (z2 + b1 x) - a1 y; z2 = b2 x - a2 y"""
    b0, b1, b2 = (float(v) for v in b)
    a1, a2 = float(a[1]), float(a[2])
    z1 = z2 = 0.0
    y = np.empty(len(x), np.float64)
    for i, v in enumerate(x.tolist()):
        o = z1 + b0 * v
        z1 = (z2 + b1 * v) - a1 * o
        z2 = b2 * v - a2 * o
        y[i] = o
    return y.astype(np.float32) if f32_out else y


def k_filter(x, rate, f32_storage=False):
    (bs, as_), (bh, ah) = W.k_weighting(rate)
    y = biquad(bs, as_, np.asarray(x, np.float32).astype(np.float64), f32_storage)
    return biquad(bh, ah, y.astype(np.float64), f32_storage)


def block_powers(y, rate):
    """z_j of the filtered signal y, sample-ordered sums: f64 [n_blocks]"""
    L = len(y)
    nb = W.n_blocks_of(L, rate)
    z = np.zeros(nb)
    if y.dtype == np.float32:                            # pyloudnorm on a float32 array: float32 squares, numpy's float32 sum
        for j, (lo, hi) in enumerate(W.block_bounds(rate, nb)):
            z[j] = float(np.sum(np.square(y[lo:hi]))) / (0.4 * float(rate))
        return z
    y2 = y * y
    for j, (lo, hi) in enumerate(W.block_bounds(rate, nb)):
        s = np.cumsum(y2[lo:min(hi, L)])                 # (sequential: one accumulator in sample order)
        z[j] = (float(s[-1]) if len(s) else 0.0) / (0.4 * float(rate))
    return z


def gate(z, target=-22.0):
    """z f64 [n_blocks] -> dict(lufs, gain, status bits 0 / 1, gamma, levels l_j, margin): the gating, one accumulator per mean"""
    if len(z) == 0:
        return dict(lufs=float("nan"), gain=1.0, status=1, gamma=float("nan"), levels=np.zeros(0), margin=float("inf"))
    with np.errstate(divide="ignore"):
        lv = -0.691 + 10.0 * np.log10(z)
    s, c = 0.0, 0
    for j in range(len(z)):
        if lv[j] >= -70.0:
            s += float(z[j])
            c += 1
    if c == 0:
        return dict(lufs=float("-inf"), gain=1.0, status=2, gamma=float("nan"), levels=lv, margin=float(np.min(np.abs(lv[np.isfinite(lv)] + 70.0), initial=np.inf)))
    gamma = -0.691 + 10.0 * math.log10(s / c) - 10.0
    s2, c2 = 0.0, 0
    for j in range(len(z)):
        if lv[j] > gamma and lv[j] > -70.0:
            s2 += float(z[j])
            c2 += 1
    fin = np.isfinite(lv)
    margin = float(min(np.min(np.abs(lv[fin] + 70.0), initial=np.inf), np.min(np.abs(lv[fin] - gamma), initial=np.inf)))
    lufs = -0.691 + 10.0 * math.log10(s2 / c2)
    return dict(lufs=lufs, gain=float(np.power(10.0, (target - lufs) / 20.0)), status=0, gamma=gamma, levels=lv, margin=margin)


def apply_gain(x, gain, status):
    """-> (y float32 like x, status with bit 2): numpy float32 arithmetic, (float)gain x and the peak rule; refused kinds are copied"""
    x = np.asarray(x, np.float32)
    if status & 3:
        return x.copy(), status
    y = np.float32(gain) * x
    p = np.float32(np.abs(y).max()) if len(y) else np.float32(0)
    if p > 1:
        return y / p, status | 4
    return y, status


def loudness(x, rate, target=-22.0, f32_storage=False):
    """the whole unit for one utterance x float32 [L] -> dict(y = the filtered signal, z, n_blocks, lufs, gain, status, out, margin, levels)"""
    x = np.asarray(x, np.float32)
    nb = W.n_blocks_of(len(x), rate)
    if nb == 0:
        g = gate(np.zeros(0), target)
        out, st = apply_gain(x, 1.0, 1)
        return dict(y=np.zeros(0), z=np.zeros(0), n_blocks=0, out=out, peak=0.0, **{**g, "status": st})
    (bs, as_), (bh, ah) = W.k_weighting(rate)
    ya = biquad(bs, as_, x.astype(np.float64), f32_storage)
    y = biquad(bh, ah, ya.astype(np.float64), f32_storage)
    z = block_powers(y, rate)
    g = gate(z, target)
    out, st = apply_gain(x, g["gain"], g["status"])
    peak = float(max(np.abs(x).max(), np.abs(ya).max(), np.abs(y).max()))   # the largest value the recurrence handles, up to its coefficients
    return dict(y=y, z=z, n_blocks=nb, out=out, peak=peak, **{**g, "status": st})


def state_matrix(rate):
    """M of s' = M s + g x for the cascade, s = (z1, z2 of the shelf, z1, z2 of the high pass): the images of the unit states at x = 0"""
    (bs, as_), (bh, ah) = W.k_weighting(rate)
    M = np.zeros((4, 4))
    for j in range(4):
        s = [0.0] * 4
        s[j] = 1.0
        ya = s[0]
        s[0], s[1] = s[1] - as_[1] * ya, -as_[2] * ya
        yb = s[2] + bh[0] * ya
        s[2], s[3] = (s[3] + bh[1] * ya) - ah[1] * yb, bh[2] * ya - ah[2] * yb
        M[:, j] = s
    return M


def rounding_gain(rate):
    """R = sum over m >= 0 of ||M^m||_inf: how far the rounding errors of single steps, each carried on by the recurrence, can add up in a
    state (the series converges: the cascade is stable); and |c| = the row of the output, y = s[2] + b0h (s[0] + b0s x)"""
    M = state_matrix(rate)
    P, R = np.eye(4), 0.0
    for _ in range(200000):
        nrm = float(np.abs(P).sum(axis=1).max())
        R += nrm
        if nrm < 1e-18 * R:
            break
        P = P @ M
    return R
