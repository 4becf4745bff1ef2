"""The recursion of include/qn_terms.h restated in numpy.longdouble, with the dense B it stands for and the margin of
every decision it takes - the reference of the quasi-Newton ring's tests (test_qn_ring_host.py, test_qn_ring.py,
test_qn_ring_shim.py).  Written from the formulas in the header's comment; it shares no code with the library."""
import numpy as np

LD = np.longdouble
SR1, BFGS, DAMPED = 0, 1, 2
U = 2.0 ** -52


def _dot(a, b):
    return (a * b).sum(dtype=LD)


def _rel_gap(a, b):
    """relative distance of two compared quantities"""
    m = max(abs(a), abs(b))
    return float(abs(a - b) / m) if m > 0 else 0.0


def _sign_margin(a, b):
    """how far the sum a . b is from zero, relative to the size of its terms"""
    m = np.abs(a * b).sum(dtype=LD)
    return float(abs(_dot(a, b)) / m) if m > 0 else 0.0


def qn_ref(kind, S, Y, memory):
    """S, Y: n x npairs (oldest first).  Returns a dict: scale, V (n x rank, longdouble), coef, rank, damped, skipped
    (lists over the used pairs), B (dense, longdouble) and margins - (name, pair, margin) of every comparison that
    decides the discrete outcome, margin = relative distance from its threshold (exact ties: 0)."""
    S = np.asarray(S, dtype=LD)
    Y = np.asarray(Y, dtype=LD)
    n, npairs = S.shape
    L = min(npairs, memory)
    S, Y = S[:, npairs - L:], Y[:, npairs - L:]
    scale = LD(1)
    margins = []
    if L:
        s, y = S[:, -1], Y[:, -1]
        ys = _dot(y, s)
        if kind == SR1:
            margins.append(("scale_ys_sign", L - 1, _sign_margin(y, s)))
            scale = _dot(y, y) / ys if ys > 0 else LD(1e-4)
        elif ys != 0:
            scale = max(_dot(s, s) / ys, LD(1e-6))
            if kind == DAMPED:
                scale = min(scale, LD(1))
    cols, coef, damped, skipped = [], [], [False] * L, [False] * L

    def apply(v):
        out = scale * v
        for c, f in zip(cols, coef):
            out = out + f * _dot(c, v) * c
        return out

    for j in range(L):
        s, y = S[:, j], Y[:, j]
        Bs = apply(s)
        if kind == SR1:
            a = y - Bs
            a_s = _dot(a, s)
            thr = LD(1e-8) * np.sqrt(_dot(s, s)) * np.sqrt(_dot(a, a))
            if a_s == 0 or abs(a_s) < thr:
                skipped[j] = True
                if a_s != 0:
                    margins.append(("sr1_skip", j, _rel_gap(abs(a_s), thr)))
                continue
            margins.append(("sr1_keep", j, _rel_gap(abs(a_s), thr)))
            cols.append(a)
            coef.append(1 / a_s)
            continue
        sBs = _dot(s, Bs)
        yts = _dot(y, s)
        margins.append(("sBs_sign", j, _sign_margin(s, Bs)))
        if not sBs > 0:
            skipped[j] = True
            continue
        yt = y
        if kind == DAMPED:
            margins.append(("damp", j, _rel_gap(yts, LD(0.2) * sBs)))
            if yts < LD(0.2) * sBs:
                theta = LD(0.8) * sBs / (sBs - yts)
                yt = theta * y + (1 - theta) * Bs
                yts = _dot(yt, s)
                damped[j] = True
        if not damped[j]:
            margins.append(("yts_sign", j, _sign_margin(y, s)))
        if not yts > 0:
            skipped[j] = True
            continue
        cols += [Bs, yt]
        coef += [-1 / sBs, 1 / yts]
    V = np.stack(cols, axis=1) if cols else np.zeros((n, 0), dtype=LD)
    coef = np.array(coef, dtype=LD)
    return {"scale": scale, "V": V, "coef": coef, "rank": len(cols), "damped": damped, "skipped": skipped,
            "B": dense_B(scale, V, coef), "margins": margins}


def dense_B(scale, V, coef):
    """scale I + V diag(coef) V' in longdouble"""
    V = np.asarray(V, dtype=LD)
    n = V.shape[0]
    return LD(scale) * np.eye(n, dtype=LD) + (V * np.asarray(coef, dtype=LD)) @ V.T


def rel_err(B, Bref):
    """entrywise error relative to max |Bref|"""
    return float(np.abs(np.asarray(B, dtype=LD) - Bref).max() / np.abs(Bref).max())


def random_pairs(n, L, kind, correlated, seed):
    """Steps S (independent, or 0.99-correlated neighbours, lengths over three decades) and Y = H S with H definite
    (BFGS), indefinite (SR1) or indefinite with half of the spectrum negative (damped BFGS: independent steps get damped pairs)."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, L))
    if correlated:
        for j in range(1, L):
            S[:, j] = 0.99 * S[:, j - 1] / np.linalg.norm(S[:, j - 1]) * np.linalg.norm(S[:, j]) + np.sqrt(1 - 0.99 ** 2) * S[:, j]
    S *= 10.0 ** rng.uniform(-1.5, 1.5, L)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = 10.0 ** rng.uniform(-1, 1, n)
    if kind == SR1:
        ev *= rng.choice([-1.0, 1.0], n)
    elif kind == DAMPED:
        ev[: n // 2] *= -1.0
    H = (Q * ev) @ Q.T
    H = (H + H.T) / 2
    return np.asfortranarray(S), np.asfortranarray(H @ S)
