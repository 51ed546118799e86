"""Float64 numpy Viterbi of the jump-GPLVM HMM (TEST INFRASTRUCTURE ONLY).

The model is the one decode_latent_viterbi maximises:

    log p(x, y) = log pi0[x_0] + sum_{t>=1} (logA[d_{t-1}, d_t] + logK[d_t][l_{t-1}, l_t]) + sum_t u[t, l_t]

with u = likelihood_scale * ll, logK[0] = logK0 (any (L, L) log kernel, -inf allowed),
logK[1] = -log L, and pi0 a uniform state "at t = -1" pushed through one transition with
a sum (oracle/brute.py's p0).  Every arg-max takes the first index (np.argmax), in
(d, i) order.
"""
import numpy as np


def banded_logK(tr):
    """(L, L) log continuous kernel [i_prev, j_next] of a BandedTransition at its float32
    device values: log g[|i-j|] + log invz[i] within the band, -inf beyond it."""
    L, band = int(tr.L), int(tr.band)
    g = np.asarray(tr.g, np.float32).astype(np.float64)
    invz = np.asarray(tr.invz, np.float32).astype(np.float64)
    i = np.arange(L)
    dist = np.abs(i[:, None] - i[None, :])
    with np.errstate(divide='ignore'):
        lg = np.log(g)
        out = np.where(dist <= band, lg[np.minimum(dist, band)] + np.log(invz)[:, None], -np.inf)
    return out


def device_logA(tr):
    """(2, 2) log dynamics matrix at its float32 device values (log 0 = -inf)."""
    A = np.asarray(tr.A, np.float64).astype(np.float32).astype(np.float64)
    with np.errstate(divide='ignore'):
        return np.log(A)


def log_pi0(logK0, logA):
    """(2, L) log prior of x_0: sum_x 1/(2L) * A[d, d'] * K[d'][i, j]."""
    L = logK0.shape[0]
    A = np.exp(logA)
    K0 = np.exp(logK0)
    pi0 = np.stack([(A[0, 0] + A[1, 0]) / (2 * L) * K0.sum(0), np.full(L, (A[0, 1] + A[1, 1]) / (2 * L))])
    with np.errstate(divide='ignore'):
        return np.log(pi0)


def viterbi(u, logK0, logA, log_pi0):
    """u (T, L) float64.  Returns (path (T, 2) int32 of (d, l), score)."""
    u = np.asarray(u, np.float64)
    T, L = u.shape
    logL = np.log(L)
    delta = log_pi0 + u[0][None, :]                    # (2, L)
    ptr = np.zeros((T, 2, L), np.int64)                # previous state d * L + i
    for t in range(1, T):
        a = delta[:, None, :] + logA[:, :, None]       # [d, d', i]
        ad = a.argmax(0)                               # (d', i)
        am = a.max(0)
        c0 = am[0][:, None] + logK0                    # [i, j]
        i0 = c0.argmax(0)
        v0 = c0[i0, np.arange(L)]
        i1 = int(am[1].argmax())
        v1 = am[1][i1] - logL
        ptr[t, 0] = ad[0][i0] * L + i0
        ptr[t, 1] = ad[1][i1] * L + i1
        delta = np.stack([v0, np.full(L, v1)]) + u[t][None, :]
    x = int(delta.reshape(-1).argmax())
    score = float(delta.reshape(-1)[x])
    path = np.zeros((T, 2), np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = (x // L, x % L)
        if t:
            x = int(ptr[t, x // L, x % L])
    return path, score


def path_score(path, u, logK0, logA, log_pi0):
    """(score, M): log p(path, y) in float64 and the largest absolute per-step increment,
    the latter with u taken relative to its row maximum (the scale the device works at)."""
    u = np.asarray(u, np.float64)
    path = np.asarray(path)
    T, L = u.shape
    d, l = path[:, 0].astype(np.int64), path[:, 1].astype(np.int64)
    tr = np.empty(T)
    tr[0] = log_pi0[d[0], l[0]]
    k0 = logK0[l[:-1], l[1:]]
    tr[1:] = logA[d[:-1], d[1:]] + np.where(d[1:] == 0, k0, -np.log(L))
    ut = u[np.arange(T), l]
    inc = tr + ut
    rel = tr + (ut - u.max(axis=1))
    return float(inc.sum()), float(np.max(np.abs(rel)))
