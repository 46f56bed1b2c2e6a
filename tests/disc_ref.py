"""Float64 restatement of HifiGAN's discriminators, written from their definitions (modules/hifigan/hifigan.py:154-338): the yardstick of
tests/test_disc_gpu.py, itself held against the reference's own float64 run in tests/test_disc_cpu.py (fixture g16_disc.npz).  numpy only.

MultiPeriodDiscriminator, period p: the waveform is reflect padded on the right to a multiple of p and folded to [rows][p]; every column
goes through Conv(1 -> 32 -> 128 -> 512 -> 1024; k = 5, stride 3, pad 2), Conv(1024 -> 1024; k = 5, pad 2), leaky_relu(0.1) after each, and
conv_post (1024 -> 1; k = 3, pad 1).  MultiScaleDiscriminator, scale i: the waveform pooled i times by AvgPool1d(4, 2, padding = 1) (zero
padding counted) goes through the seven Conv1d of DISC_MSD_CONVS with leaky_relu(0.1), then conv_post.  The feature maps are the activated
outputs, conv_post's raw output last; D is that output flattened (rows major, the period's columns minor).
"""
import numpy as np

PERIODS = (2, 3, 5, 7, 11)
SLOPE = 0.1
# (C_out, C_in, k, stride, groups)
MPD_CONVS = ((32, 1, 5, 3, 1), (128, 32, 5, 3, 1), (512, 128, 5, 3, 1), (1024, 512, 5, 3, 1), (1024, 1024, 5, 1, 1))
MSD_CONVS = ((128, 1, 15, 1, 1), (128, 128, 41, 2, 4), (256, 128, 41, 2, 16), (512, 256, 41, 4, 16), (1024, 512, 41, 4, 16),
             (1024, 1024, 41, 1, 16), (1024, 1024, 5, 1, 1))
POST = (1, 1024, 3, 1, 1)
MIN_LEN = 6


def lrelu(x):
    return np.where(x > 0, x, x * SLOPE)


def conv1d(x, w, b, stride, groups):
    """x [C_in, T], w [C_out, C_in / groups, k] (trailing singleton dimensions dropped), padding k // 2 -> [C_out, T_out], float64"""
    w = np.asarray(w, np.float64)
    w = w.reshape(w.shape[0], w.shape[1], w.shape[2])
    co, cig, k = w.shape
    pad = k // 2
    T = x.shape[1]
    xp = np.zeros((x.shape[0], T + 2 * pad))
    xp[:, pad:pad + T] = x
    T_out = (T + 2 * pad - k) // stride + 1
    win = np.lib.stride_tricks.sliding_window_view(xp, k, axis=1)[:, ::stride][:, :T_out]   # [C_in, T_out, k]
    cog = co // groups
    out = np.empty((co, T_out))
    for g in range(groups):
        cols = win[g * cig:(g + 1) * cig].transpose(1, 0, 2).reshape(T_out, cig * k)
        out[g * cog:(g + 1) * cog] = (cols @ w[g * cog:(g + 1) * cog].reshape(cog, cig * k).T).T
    return out + np.asarray(b, np.float64)[:, None]


def avg_pool(x):
    """AvgPool1d(4, 2, padding = 1), count_include_pad: the edges divide by 4 too"""
    n = (len(x) + 2 - 4) // 2 + 1
    xp = np.concatenate([[0.0], x, [0.0, 0.0]])
    return np.array([xp[2 * i:2 * i + 4].sum() / 4.0 for i in range(n)])


def mpd_forward(W, i, x):
    """discriminator i of the MultiPeriodDiscriminator on one waveform -> (D [n], fmaps: arrays [C, rows, p])"""
    p = PERIODS[i]
    x = np.asarray(x, np.float64)
    L = len(x)
    if L % p:
        n_pad = p - L % p
        if n_pad > L - 1:
            raise ValueError(f"reflect padding of {n_pad} samples needs more than {L} samples")
        x = np.concatenate([x, x[L - 2::-1][:n_pad]])
    cols = x.reshape(-1, p)                                   # [rows, p]
    h = [cols[:, j][None, :] for j in range(p)]               # per column [1, rows]
    fmaps = []
    for j, (co, ci, k, s, g) in enumerate(MPD_CONVS):
        pre = f"mpd.{i}.convs.{j}"
        h = [lrelu(conv1d(c, W[pre + ".weight"], W[pre + ".bias"], s, g)) for c in h]
        fmaps.append(np.stack(h, axis=2))
    pre = f"mpd.{i}.conv_post"
    h = [conv1d(c, W[pre + ".weight"], W[pre + ".bias"], 1, 1) for c in h]
    post = np.stack(h, axis=2)                                # [1, rows, p]
    fmaps.append(post)
    return post.reshape(-1), fmaps


def msd_forward(W, i, x):
    """discriminator i of the MultiScaleDiscriminator on one waveform (pooled i times here) -> (D [n], fmaps: arrays [C, T])"""
    x = np.asarray(x, np.float64)
    for _ in range(i):
        x = avg_pool(x)
    h = x[None, :]
    fmaps = []
    for j, (co, ci, k, s, g) in enumerate(MSD_CONVS):
        pre = f"msd.{i}.convs.{j}"
        h = lrelu(conv1d(h, W[pre + ".weight"], W[pre + ".bias"], s, g))
        fmaps.append(h)
    pre = f"msd.{i}.conv_post"
    h = conv1d(h, W[pre + ".weight"], W[pre + ".bias"], 1, 1)
    fmaps.append(h)
    return h.reshape(-1), fmaps


def forward(W, d, x):
    return mpd_forward(W, d, x) if d < 5 else msd_forward(W, d - 5, x)


def score_pair(W, y, y_hat, discs=range(8)):
    """one utterance pair, alone at its own length -> dict: d_real / d_gen (lists of D per discriminator, None where not run), sums [8, 4]
    (sum (1 - D(y))^2, sum D(y)^2, sum (1 - D(y_hat))^2, sum D(y_hat)^2), counts [8], fm / fm_counts [8, 8] (sum |fmap(y) - fmap(y_hat)|
    and its element count per layer), fmax [8, 8] (the larger of max |fmap(y)|, max |fmap(y_hat)|)"""
    if len(y) != len(y_hat) or len(y) < MIN_LEN:
        raise ValueError(f"a pair of {len(y)} / {len(y_hat)} samples (equal lengths >= {MIN_LEN})")
    out = {"d_real": [None] * 8, "d_gen": [None] * 8, "sums": np.full((8, 4), np.nan), "counts": np.zeros(8, np.int64),
           "fm": np.full((8, 8), np.nan), "fm_counts": np.zeros((8, 8), np.int64), "fmax": np.zeros((8, 8))}
    for d in discs:
        dr, fr = forward(W, d, y)
        dg, fg = forward(W, d, y_hat)
        out["d_real"][d], out["d_gen"][d] = dr, dg
        out["sums"][d] = [((1 - dr) ** 2).sum(), (dr ** 2).sum(), ((1 - dg) ** 2).sum(), (dg ** 2).sum()]
        out["counts"][d] = dr.size
        for l, (a, b) in enumerate(zip(fr, fg)):
            out["fm"][d, l] = np.abs(a - b).sum()
            out["fm_counts"][d, l] = a.size
            out["fmax"][d, l] = max(np.abs(a).max(), np.abs(b).max())
    return out


def figures(sums, counts, fm=None, fm_counts=None):
    """sums [B, 8, 4], counts [B, 8] (fm, fm_counts [B, 8, 8]) -> the reference's figures per utterance and pooled over the batch"""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.float64)
    out = {}
    for tag, sl in (("p", slice(0, 5)), ("s", slice(5, 8))):
        for name, q in (("a", 2), ("r", 0), ("f", 3)):
            out[f"{name}_{tag}"] = (sums[:, sl, q] / counts[:, sl]).mean(1)
            out[f"{name}_{tag}_batch"] = (sums[:, sl, q].sum(0) / counts[:, sl].sum(0)).mean()
    if fm is not None:
        fm, fmc = np.asarray(fm, np.float64), np.asarray(fm_counts, np.float64)
        for tag, sl, nl in (("f", slice(0, 5), 6), ("s", slice(5, 8), 8)):
            out[f"fm_{tag}"] = 2.0 * (fm[:, sl, :nl] / fmc[:, sl, :nl]).sum((1, 2))
            out[f"fm_{tag}_batch"] = 2.0 * (fm[:, sl, :nl].sum(0) / fmc[:, sl, :nl].sum(0)).sum()
    return out
