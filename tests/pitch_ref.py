"""Float64 restatement of the F0 extraction specified in include/dicttts_hip.h (DTTS_OUT_PITCH): Boersma's autocorrelation method as Praat's
Sound_to_Pitch_any (ac, Hanning window) and Pitch_pathFinder run it.  Plain numpy; every sum is a math.fsum of float64 products.  Each stage
can be run on its own input, so that a test can feed it the device's previous stage.

The maximiser of the depth-70 interpolant is converged to 1e-12 in lag: a golden-section search over [l - 1, l + 1] to 1e-7, then the zero of
the ANALYTIC derivative bracketed around it (function values alone define a flat maximum only to about 1e-6: sqrt(2 eps / curvature)).
``maximise_signchange`` restates the method the device uses instead (the sign change of the analytic derivative), so that the two can be
compared here.
"""
import math

import numpy as np

NCAND = 15
PRAAT = dict(voicing_threshold=0.6, silence_threshold=0.03, octave_cost=0.01, octave_jump_cost=0.35, voiced_unvoiced_cost=0.14)


def params(sr=22050, hop=256, floor=80.0, ceiling=750.0, **kw):
    p = dict(PRAAT, sr=int(sr), hop=int(hop), floor=float(floor), ceiling=float(ceiling))
    p.update(kw)
    return p


def geometry(sr, floor):
    q = (3.0 * float(sr)) / float(floor)
    nsw0 = int(math.floor(q))
    half = nsw0 // 2 - 1
    nsw = 2 * half
    nper = int(math.floor(float(sr) / float(floor)))
    return dict(nsw=nsw, half=half, nper=nper, halfper=nper // 2 + 1, maxlag=min(nsw // 3 + 2, nsw), brent=nsw // 2, n_lag=nsw // 2 + 1,
                first=int(math.ceil(q)))


def n_frames(L, g, hop):
    return (L - g["first"]) // hop + 1 if L >= g["first"] else 0


_TABLES = {}


def tables(nsw):
    """the window w [nsw] and its autocorrelation normalised by lag 0, wr [nsw / 2 + 1]"""
    if nsw not in _TABLES:
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(nsw, dtype=np.float64) + 1.0) / (nsw + 1))
        w0 = math.fsum(w * w)
        wr = np.array([math.fsum(w[:nsw - l] * w[l:]) / w0 for l in range(nsw // 2 + 1)])
        _TABLES[nsw] = (w, wr)
    return _TABLES[nsw]


def frames(x, p):
    """x: the utterance's samples -> dict: nF, acf [nF, n_lag], intensity [nF], left [nF], gpeak"""
    x = np.asarray(x, np.float64)
    L = len(x)
    g = geometry(p["sr"], p["floor"])
    hop, nsw, half = p["hop"], g["nsw"], g["half"]
    nF = n_frames(L, g, hop)
    out = dict(nF=nF, acf=np.zeros((nF, g["n_lag"])), intensity=np.zeros(nF), left=np.zeros(nF, np.int64), gpeak=0.0)
    if nF == 0:
        return out
    w, wr = tables(nsw)
    gmean = math.fsum(x) / L
    gpeak = float(np.abs(x - gmean).max())
    out["gpeak"] = gpeak
    for k in range(nF):
        left = (L - nF * hop + hop - 1 + 2 * k * hop) // 2
        right = left + 1
        out["left"][k] = left
        lo, hi = max(0, right - g["nper"]), min(L - 1, left + g["nper"])
        mean = math.fsum(x[lo:hi + 1]) / (hi - lo + 1)
        s0 = right - half
        assert s0 >= 0 and s0 + nsw <= L
        gq = x[s0:s0 + nsw] - mean
        peak = float(np.abs(gq[max(0, half - g["halfper"]):min(nsw, half + g["halfper"])]).max())
        out["intensity"][k] = 0.0 if peak == 0.0 else (1.0 if peak > gpeak else peak / gpeak)
        f = gq * w
        ac0 = math.fsum(f * f)
        r = out["acf"][k]
        r[0] = 1.0
        if peak == 0.0 or not ac0 > 0.0:
            continue
        for l in range(1, g["n_lag"]):
            r[l] = math.fsum(f[:nsw - l] * f[l:]) / (ac0 * wr[l])
    return out


def _terms(r, brent, x, D):
    """the index, phase and taper width of every term of sincD(x), left terms first"""
    ml = int(math.floor(x))
    mr = ml + 1
    D = min(D, ml + brent + 1, brent - ml)
    il = np.arange(ml, mr - D - 1, -1)
    ir = np.arange(mr, ml + D + 1)
    return ml, mr, D, il, ir


def sinc(r, x, D):
    """Praat's NUM_interpolate_sinc of depth D at the lag x on r[0 .. brent] taken symmetrically"""
    brent = len(r) - 1
    if x == math.floor(x):
        return float(r[abs(int(x))])
    ml, mr, D, il, ir = _terms(r, brent, x, D)
    pl = np.pi * (x - il)
    pr = np.pi * (ir - x)
    tl = r[np.abs(il)] * np.sin(pl) / pl * (0.5 + 0.5 * np.cos(pl / (x - (mr - D) + 1)))
    tr = r[np.abs(ir)] * np.sin(pr) / pr * (0.5 + 0.5 * np.cos(pr / ((ml + D) - x + 1)))
    return math.fsum(np.concatenate([tl, tr]))


def dsinc(r, x, D):
    """d sincD / dx at a non-integer x (the term set is fixed between two integers)"""
    brent = len(r) - 1
    ml, mr, D, il, ir = _terms(r, brent, x, D)
    out = []
    for idx, ph, W, sg in ((il, np.pi * (x - il), x - (mr - D) + 1, 1.0), (ir, np.pi * (ir - x), (ml + D) - x + 1, -1.0)):
        S = np.sin(ph) / ph
        dS = sg * np.pi * (np.cos(ph) * ph - np.sin(ph)) / (ph * ph)
        th = ph / W
        H = 0.5 + 0.5 * np.cos(th)
        dH = -0.5 * np.sin(th) * sg * (np.pi * W - ph) / (W * W)
        out.append(r[np.abs(idx)] * (dS * H + S * dH))
    return math.fsum(np.concatenate(out))


def vertex(r, l):
    return l + 0.5 * (r[l + 1] - r[l - 1]) / (2.0 * r[l] - r[l - 1] - r[l + 1])


_GOLD = (math.sqrt(5.0) - 1.0) / 2.0


def maximise(r, l, D=70):
    """the maximiser of sincD on [l - 1, l + 1], converged to 1e-12 in lag -> (x, polished)"""
    a, b = l - 1.0, l + 1.0
    c, d = b - _GOLD * (b - a), a + _GOLD * (b - a)
    fc, fd = sinc(r, c, D), sinc(r, d, D)
    while b - a > 1e-7:
        if fc >= fd:
            b, d, fd = d, c, fc
            c = b - _GOLD * (b - a)
            fc = sinc(r, c, D)
        else:
            a, c, fc = c, d, fd
            d = a + _GOLD * (b - a)
            fd = sinc(r, d, D)
    x = 0.5 * (a + b)
    cell = math.floor(x)
    lo, hi = max(x - 1e-4, cell + 1e-9, l - 1.0 + 1e-9), min(x + 1e-4, cell + 1.0 - 1e-9, l + 1.0 - 1e-9)
    flo, fhi = dsinc(r, lo, D), dsinc(r, hi, D)
    if not (flo > 0.0 > fhi):
        return x, False                      # the maximum sits on a cell edge or on the bracket's: the search's own answer stands
    for _ in range(100):                     # Illinois regula falsi on the derivative
        if hi - lo <= 1e-13:
            break
        xm = hi - fhi * (hi - lo) / (fhi - flo)
        if not lo < xm < hi:
            xm = 0.5 * (lo + hi)
        fm = dsinc(r, xm, D)
        if fm == 0.0:
            lo = hi = xm
            break
        if fm > 0.0:
            lo, flo = xm, fm
            fhi *= 0.5
        else:
            hi, fhi = xm, fm
            flo *= 0.5
    return 0.5 * (lo + hi), True


def maximise_signchange(r, l, D=70):
    """the device's method: the place where d sincD / dx changes sign from + to - (a zero inside a cell, or a kink on an integer lag, where
    the term set changes), bracketed around the parabolic vertex inside [l - 1, l + 1] and closed in on by the Illinois regula falsi"""
    eps = 2.0 ** -30

    def d(x):
        return dsinc(r, x + 2.0 ** -40 if x == math.floor(x) else x, D)

    xv = vertex(r, l)
    a, b = max(xv - 0.5, l - 1.0 + eps), min(xv + 0.5, l + 1.0 - eps)
    fa, fb = d(a), d(b)
    if not fa > 0.0:
        a = l - 1.0 + eps
        fa = d(a)
        if not fa > 0.0:
            return a
    if not fb < 0.0:
        b = l + 1.0 - eps
        fb = d(b)
        if not fb < 0.0:
            return b
    for _ in range(80):
        if b - a <= 1e-12:
            break
        xm = b - fb * (b - a) / (fb - fa)
        if not a < xm < b:
            xm = 0.5 * (a + b)
        fm = d(xm)
        if fm > 0.0:
            a, fa = xm, fm
            fb *= 0.5
        elif fm < 0.0:
            b, fb = xm, fm
            fa *= 0.5
        else:
            return xm
    return 0.5 * (a + b)


def candidates(r, p, maximiser=maximise):
    """one frame's r[0 .. brent] -> dict: cand [15, 2] (frequency, strength), n, lag [15] (the integer lag of each slot), x [15] (the
    refined lag), maxima (how many maxima the frame had)"""
    g = geometry(p["sr"], p["floor"])
    sr, oc, floor = float(p["sr"]), p["octave_cost"], p["floor"]
    slots = [(0.0, 0.0, 0)]
    maxima = 0
    for l in range(2, min(g["maxlag"], g["brent"])):
        if r[l] > 0.5 * p["voicing_threshold"] and r[l] > r[l - 1] and r[l] >= r[l + 1]:
            maxima += 1
            x0 = vertex(r, l)
            s0 = sinc(r, x0, 30)
            if s0 > 1.0:
                s0 = 1.0 / s0
            f = sr / x0
            if len(slots) < NCAND:
                slots.append((f, s0, l))
                continue
            figs = [s - oc * math.log2(floor / fq) for fq, s, _ in slots[1:]]
            iw = 1 + int(np.argmin(figs))                     # the first of the smallest
            if s0 - oc * math.log2(floor / f) > figs[iw - 1]:
                slots[iw] = (f, s0, l)
    cand, lag, xs = np.zeros((NCAND, 2)), np.zeros(NCAND, np.int64), np.zeros(NCAND)
    for i, (f, s, l) in enumerate(slots):
        if i:
            x = maximiser(r, l)
            x = x[0] if isinstance(x, tuple) else x
            s = sinc(r, x, 70)
            if s > 1.0:
                s = 1.0 / s
            f = sr / x
            xs[i] = x
        cand[i] = (f, s)
        lag[i] = l
    return dict(cand=cand, n=len(slots), lag=lag, x=xs, maxima=maxima)


def path(cand, n_cand, intensity, p):
    """cand [nF, 15, 2], n_cand [nF], intensity [nF] -> dict: selected [nF], f0 [nF], margin (the smallest gap between the best and the
    second-best value at the decisions on the chosen path: its backpointers and the final argmax; inf when there was never a choice)"""
    nF = len(n_cand)
    ceiling = min(p["ceiling"], 0.5 * p["sr"])
    vt, st, oc = p["voicing_threshold"], p["silence_threshold"], p["octave_cost"]
    corr = 0.01 / (p["hop"] / float(p["sr"]))
    OJ, VU = p["octave_jump_cost"] * corr, p["voiced_unvoiced_cost"] * corr
    voiced = lambda f: 0.0 < f < ceiling
    delta = np.full((nF, NCAND), -np.inf)
    psi = np.zeros((nF, NCAND), np.int64)
    gaps = np.full((nF, NCAND), np.inf)
    for k in range(nF):
        for c2 in range(int(n_cand[k])):
            f2, s2 = cand[k, c2]
            local = s2 - oc * math.log2(ceiling / f2) if voiced(f2) else vt + max(0.0, 2.0 - intensity[k] * (1.0 + vt) / st)
            if k == 0:
                delta[k, c2] = local
                continue
            vals = []
            for c1 in range(int(n_cand[k - 1])):
                f1 = cand[k - 1, c1, 0]
                v1, v2 = voiced(f1), voiced(f2)
                cost = VU if v1 != v2 else (OJ * abs(math.log2(f1 / f2)) if v1 else 0.0)
                vals.append(delta[k - 1, c1] - cost)
            best = int(np.argmax(vals))                        # the first maximum
            delta[k, c2] = vals[best] + local
            psi[k, c2] = best
            if len(vals) > 1:
                srt = sorted(vals)
                gaps[k, c2] = srt[-1] - srt[-2]
    sel = np.zeros(nF, np.int64)
    margin = np.inf
    if nF:
        last = delta[nF - 1, :int(n_cand[nF - 1])]
        c = int(np.argmax(last))
        if len(last) > 1:
            srt = sorted(last)
            margin = srt[-1] - srt[-2]
        for k in range(nF - 1, -1, -1):
            sel[k] = c
            if k > 0:
                margin = min(margin, gaps[k, c])
                c = int(psi[k, c])
    f0 = np.array([cand[k, sel[k], 0] if voiced(cand[k, sel[k], 0]) else 0.0 for k in range(nF)])
    return dict(selected=sel, f0=f0, margin=float(margin))


def pitch(x, p, maximiser=maximise):
    """the whole chain on one utterance -> dict of every stage"""
    fr = frames(x, p)
    nF = fr["nF"]
    cand, n_cand, lag, xs, maxima = np.zeros((nF, NCAND, 2)), np.zeros(nF, np.int64), np.zeros((nF, NCAND), np.int64), np.zeros((nF, NCAND)), np.zeros(nF, np.int64)
    for k in range(nF):
        c = candidates(fr["acf"][k], p, maximiser)
        cand[k], n_cand[k], lag[k], xs[k], maxima[k] = c["cand"], c["n"], c["lag"], c["x"], c["maxima"]
    out = path(cand, n_cand, fr["intensity"], p)
    out.update(nF=nF, acf=fr["acf"], intensity=fr["intensity"], left=fr["left"], gpeak=fr["gpeak"], cand=cand, n_cand=n_cand, lag=lag, x=xs, maxima=maxima)
    return out
