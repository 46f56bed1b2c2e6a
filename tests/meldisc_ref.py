"""A float64 numpy restatement of modules/fastspeech/multi_window_disc.py::Discriminator in eval mode (no cond_disc): the yardstick of
tests/test_meldisc_gpu.py, itself held against the reference's float64 by tests/test_meldisc_cpu.py.  It takes the plain weights of
``mel_discriminator.fold_state_dict(state, np.float64)``.
"""
import numpy as np

WINS = (32, 64, 128)
SLOPE = 0.2
IN_EPS = 1e-5


def conv3x3_s2(x, w, b):
    """Conv2d(3 x 3, stride 2, pad 1): x [C_in, T, F], w [C_out, C_in, 3, 3], b [C_out] -> [C_out, T / 2, F / 2]"""
    _, T, F = x.shape
    To, Fo = (T - 1) // 2 + 1, (F - 1) // 2 + 1
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    cols = np.concatenate([xp[:, dt:dt + 2 * To:2, df:df + 2 * Fo:2].reshape(x.shape[0], -1) for dt in range(3) for df in range(3)])
    out = w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1) @ cols      # one contraction over (tap, channel)
    return out.reshape(w.shape[0], To, Fo) + b[:, None, None]


def describe(weights):
    n = 0
    while f"{n}.conv.0.weight" in weights:
        n += 1
    H = weights["0.conv.0.weight"].shape[0]
    return n, H, weights["0.adv.weight"].size == H * 10


def window_forward(weights, w, clip):
    """Discriminator2DFactory.forward of window w on one clip [win, 80] -> (D [1] or [win / 8], [h0, h1, h2] each [H, t, f])"""
    x = np.asarray(clip, np.float64)[None]
    h = []
    for l in range(3):
        x = conv3x3_s2(x, weights[f"{w}.conv.{l}.weight"], weights[f"{w}.conv.{l}.bias"])
        x = np.where(x > 0, x, x * SLOPE)
        if f"{w}.norm.{l}.weight" in weights:       # InstanceNorm2d(affine=True): biased variance over the map, eps 1e-5
            m = x.mean(axis=(1, 2), keepdims=True)
            v = ((x - m) ** 2).mean(axis=(1, 2), keepdims=True)
            x = (x - m) / np.sqrt(v + IN_EPS) * weights[f"{w}.norm.{l}.weight"][:, None, None] + weights[f"{w}.norm.{l}.bias"][:, None, None]
        elif f"{w}.affine.{l}.scale" in weights:    # BatchNorm2d in eval mode, folded
            x = x * weights[f"{w}.affine.{l}.scale"][:, None, None] + weights[f"{w}.affine.{l}.shift"][:, None, None]
        h.append(x)
    aw, ab = weights[f"{w}.adv.weight"].reshape(-1), weights[f"{w}.adv.bias"].reshape(-1)
    H, T3, F3 = x.shape
    if aw.size == H * F3:                           # reduction none: per time row over (c, f)
        d = x.transpose(1, 0, 2).reshape(T3, -1) @ aw + ab[0]
    else:
        d = np.array([x.reshape(-1) @ aw + ab[0]])
    return d, h


def clip_of(mel, length, start, win):
    """`win` frames from `start`; frames at or behind `length` are zeros"""
    out = np.zeros((win, mel.shape[1]))
    n = max(0, min(length, start + win) - start)
    out[:n] = mel[start:start + n]
    return out


def score_utterance(weights, mel_g, mel_p, starts):
    """one utterance alone at its own length.  starts[w]: the clip starts of window w (all within the length).  -> d_g, d_p: per window
    [n_clips, n_out]; sums [2, 3, 2] (signal, window, (sum (1 - D)^2, sum D^2)), counts [2, 3]"""
    n_win, _, per_row = describe(weights)
    L = mel_g.shape[0]
    res = {"d_g": [], "d_p": [], "sums": np.zeros((2, 3, 2)), "counts": np.zeros((2, 3), np.int64)}
    for w in range(n_win):
        for si, (key, mel) in enumerate((("d_g", mel_g), ("d_p", mel_p))):
            ds = [window_forward(weights, w, clip_of(mel, L, s, WINS[w]))[0] for s in starts[w]]
            d = np.stack(ds) if ds else np.zeros((0, WINS[w] // 8 if per_row else 1))
            res[key].append(d)
            res["sums"][si, w] = [((1 - d) ** 2).sum(), (d ** 2).sum()]
            res["counts"][si, w] = d.size
    return res


def x_len_of(x):
    """Discriminator.forward's x_len: the number of frames whose bins do not sum to 0"""
    return (np.asarray(x).sum(-1) != 0).sum(-1)


def forward(weights, reduction, x, starts):
    """Discriminator.forward(x [B, T, 80], start_frames_wins=[[s] * B per window]) -> (y or None, h): y [B, 1, n_win] (stack), [B, 1] (sum)
    or [B, sum win / 8] (none); h: the maps of every window that ran, [B, H, t, f]"""
    n_win = describe(weights)[0]
    x = np.asarray(x, np.float64)
    B, T = x.shape[:2]
    xl = int(x_len_of(x).max())
    ys, hs = [], []
    for w in range(n_win):
        if xl < WINS[w]:
            continue
        out = [window_forward(weights, w, clip_of(x[b], T, starts[w], WINS[w])) for b in range(B)]
        ys.append(np.stack([o[0] for o in out]))
        hs += [np.stack([o[1][l] for o in out]) for l in range(3)]
    if len(ys) != n_win:
        return None, hs
    if reduction == "sum":
        return sum(ys), hs
    if reduction == "stack":
        return np.stack(ys, -1), hs
    return np.concatenate(ys, -1), hs


def figures(sums, counts, n_win):
    """sums [2B, 3, 2], counts [2B, 3] (recordings, then predictions) -> r, f, a [B, n_win], <name>_win [n_win], <name>_batch"""
    sums, counts = np.asarray(sums, np.float64)[:, :n_win], np.asarray(counts, np.float64)[:, :n_win]
    B = sums.shape[0] // 2
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, sl, q in (("r", slice(0, B), 0), ("f", slice(B, 2 * B), 1), ("a", slice(B, 2 * B), 0)):
            out[name] = sums[sl, :, q] / counts[sl]
            pooled = sums[sl, :, q].sum(0) / counts[sl].sum(0)
            out[name + "_win"] = pooled
            out[name + "_batch"] = np.nanmean(pooled) if np.any(~np.isnan(pooled)) else np.nan
    return out
