"""Float64 reference of the posterior path sampler (pmg_segment_sample /
sample_latent_segments; TEST INFRASTRUCTURE ONLY) and the step-by-step check of sampled paths.

Forward filtering, backward sampling over the flat state index x = d L + l.  With the
filter posteriors alpha (T, 2, L) of one chain [a, b):
  t = b - 1:  w[x] = alpha[t, d, l]
  t < b - 1, (d+, l+) the state at t + 1:
    d+ = 0:   w[x] = alpha[t, d, l] A[d, 0] K0[l, l+]     (K0[l, l+] = g[|l - l+|] invz[l] within
                                                           the band, 0 beyond it)
    d+ = 1:   w[x] = alpha[t, d, l] A[d, 1]               (the jump kernel 1 / L cancels)
and the draw is the smallest x with cdf[x] > u total, cdf the inclusive prefix sum of w.
The random numbers come in from outside (u (R, T), column = row of the compact layout), so
the device paths are a deterministic function of (alpha, transition, u) and check_paths can
judge every step on its own, conditional on the path's own state at t + 1 ("teacher
forced"): a flip at one step cannot hide, or cause, a violation at another.

The cases, the ragged batch (tests/segments_ref.LENS, 120 rows) and the uniforms are shared by
tests/test_sample_host.py, which checks that they make the GPU test mean something, and
tests/test_gpu_sample.py, which runs them.
"""
import functools

import numpy as np

from tests import scan_ref as S
from tests import segments_ref as R

LENS = R.LENS
N_SAMPLES = 256
# (L, band): every J, both VEC paths (L % 4), both band extremes; full lanes; tiny lines
RAGGED_CASES = ((61, 3), (127, 7), (250, 15), (500, 30), (1000, 30))
FULL_CASES = ((64, 5), (1024, 32))
TINY_CASES = ((1, 0), (2, 1), (3, 2), (8, 7), (33, 32))
CASES = RAGGED_CASES + FULL_CASES + TINY_CASES

# Rounding allowance of check_paths, relative to the step's total.  A device prefix goes
# through at most 15 in-lane adds (J = 16 values summed in latent order), 6 adds of the
# Hillis-Steele scan over the 64 lanes (depth <= 7 allowed for), one add of the d = 0 total,
# three multiplies per weight (alpha A g invz), the sum of the two row totals and the product
# u total: 27 roundings, fewer than 32, of non-negative terms, each <= 2^-24 of the total.  The
# count is doubled for slack: eps = 2 x 32 x 2^-24.
ROUNDINGS = 32
EPS = 2 * ROUNDINGS * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def uniforms(n_samples=N_SAMPLES, n_rows=int(sum(LENS)), seed=7):
    u = np.random.default_rng(seed).random((n_samples, n_rows), np.float32)
    u.setflags(write=False)
    return u


def weights(alpha_t, K0, A, d_next, l_next):
    """(2 L,) float64 weights of one step in x order.  alpha_t (2, L); K0 (L, L) [l, l+] the
    continuous kernel; A (2, 2) [d, d+]; d_next < 0 (or None): the chain's last row."""
    a = np.asarray(alpha_t, np.float64)
    if d_next is None or d_next < 0:
        return a.reshape(-1).copy()
    if d_next == 0:
        return (a * A[:, 0][:, None] * K0[:, l_next][None, :]).reshape(-1)
    return (a * A[:, 1][:, None]).reshape(-1)


def _batch_weights(alpha_t, K0T, A, dn, ln):
    """weights() for R next states at once: dn, ln (R,) -> (R, 2 L)."""
    a = np.asarray(alpha_t, np.float64)
    cont = (A[:, 0][None, :, None] * K0T[ln][:, None, :])          # (R, 2, L): A[d, 0] K0[l, l+_r]
    jump = np.broadcast_to(A[:, 1][None, :, None], cont.shape)
    f = np.where((dn == 0)[:, None, None], cont, jump)
    return (a[None] * f).reshape(len(dn), -1)


def _kernels(tr, K0, A):
    K0 = S.dense_K(tr)[0] if K0 is None else np.asarray(K0, np.float64)
    A = S.device_A(tr) if A is None else np.asarray(A, np.float64)
    return np.ascontiguousarray(K0.T), A


def _draw(w, u_t):
    """Smallest x with cdf[x] > u total per row of w (R, X); the last x with w > 0 where the
    target is not below the total.  Returns (x, cdf)."""
    cdf = np.cumsum(w, axis=1)
    target = u_t * cdf[:, -1]
    above = cdf > target[:, None]
    x = above.argmax(1)
    none = ~above.any(1)
    if none.any():
        x[none] = w.shape[1] - 1 - (w[none, ::-1] > 0).argmax(1)
    return x, cdf


def ffbs(alpha, tr, off, u, K0=None, A=None):
    """The float64 reference sampler: (path_d, path_l) (R, T) int32, -1 in rows that no
    segment owns.  alpha (T, 2, L) filter posteriors, tr a BandedTransition (its float32 device
    values are used), off (S + 1,) row offsets, u (R, T) uniforms.  K0 (L, L) [l, l+] / A
    (2, 2): another kernel or dynamics matrix in place of the transition's (wrong samplers)."""
    K0T, A = _kernels(tr, K0, A)
    alpha = np.asarray(alpha, np.float64)
    u = np.asarray(u, np.float64)
    n, L = u.shape[0], alpha.shape[2]
    pd = np.full(u.shape, -1, np.int32)
    pl = np.full(u.shape, -1, np.int32)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        for t in range(b - 1, a - 1, -1):
            if t == b - 1:
                w = np.broadcast_to(alpha[t].reshape(1, -1), (n, 2 * L))
            else:
                w = _batch_weights(alpha[t], K0T, A, pd[:, t + 1], pl[:, t + 1])
            x, _ = _draw(w, u[:, t])
            pd[:, t], pl[:, t] = x // L, x % L
    return pd, pl


def step_report(alpha, tr, off, u, path_d, path_l, eps=EPS):
    """Teacher-forced judgement of every (sample, row) of every segment: dict of boolean
    (R, T) arrays (False in rows that no segment owns)
      owned     the row belongs to a segment,
      positive  (a) the path's state has weight > 0 given the path's own state at t + 1,
      in_cell   (b) cdf[x - 1] - eps total <= u total < cdf[x] + eps total,
      near_edge u total lies within eps total of cdf[x - 1] or cdf[x] of the exact draw
                (the steps where rounding may move the draw),
    all in float64 on the transition's float32 device values."""
    K0T, A = _kernels(tr, None, None)
    alpha = np.asarray(alpha, np.float64)
    u = np.asarray(u, np.float64)
    pd, pl = np.asarray(path_d, np.int64), np.asarray(path_l, np.int64)
    n, L = u.shape[0], alpha.shape[2]
    rep = {k: np.zeros(u.shape, bool) for k in ('owned', 'positive', 'in_cell', 'near_edge')}
    rows = np.arange(n)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        for t in range(b - 1, a - 1, -1):
            rep['owned'][:, t] = True
            valid = (pd[:, t] >= 0) & (pd[:, t] < 2) & (pl[:, t] >= 0) & (pl[:, t] < L)
            if t == b - 1:
                w = np.broadcast_to(alpha[t].reshape(1, -1), (n, 2 * L))
            else:
                nv = (pd[:, t + 1] >= 0) & (pd[:, t + 1] < 2) & (pl[:, t + 1] >= 0) & (pl[:, t + 1] < L)
                valid &= nv           # no state to condition on: the step cannot be judged right
                w = _batch_weights(alpha[t], K0T, A, np.where(nv, pd[:, t + 1], 1), np.where(nv, pl[:, t + 1], 0))
            cdf = np.cumsum(w, axis=1)
            total = cdf[:, -1]
            target = u[:, t] * total
            x = np.where(valid, pd[:, t] * L + pl[:, t], 0)
            hi = cdf[rows, x]
            lo = np.where(x > 0, cdf[rows, np.maximum(x - 1, 0)], 0.0)
            rep['positive'][:, t] = valid & (w[rows, x] > 0)
            rep['in_cell'][:, t] = valid & (lo - eps * total <= target) & (target < hi + eps * total)
            above = cdf > target[:, None]
            x0 = np.where(above.any(1), above.argmax(1), 2 * L - 1)
            hi0 = cdf[rows, x0]
            lo0 = np.where(x0 > 0, cdf[rows, np.maximum(x0 - 1, 0)], 0.0)
            rep['near_edge'][:, t] = (target - lo0 < eps * total) | (hi0 - target <= eps * total)
    return rep


def check_paths(alpha, tr, off, u, path_d, path_l, eps=EPS):
    """Number of (sample, row) steps of the segments' rows that are not BOTH (a) a state of
    positive weight and (b) within eps total of the cell the uniform points at, each step
    conditional on the path's own state at t + 1.  Every step is judged; an index out of
    range (a -1 included) is a violation.  eps: see EPS."""
    rep = step_report(alpha, tr, off, u, path_d, path_l, eps)
    return int((rep['owned'] & ~(rep['positive'] & rep['in_cell'])).sum())


def z_scores(path_d, path_l, gamma):
    """The statistical bar: per row t, z of the frequency of d = 1 against the posterior
    gamma[t, 1].sum() and of the frequency of l = argmax_l P_t against P_t there (P_t =
    gamma[t].sum(0)), z = |f - p| / sqrt(max(p (1 - p), 1 / R) / R).  Returns (z_d, z_l) (T,)."""
    pd, pl = np.asarray(path_d), np.asarray(path_l)
    gamma = np.asarray(gamma, np.float64)
    n = pd.shape[0]
    P = gamma.sum(1)
    top = P.argmax(1)

    def z(f, p):
        return np.abs(f - p) / np.sqrt(np.maximum(p * (1 - p), 1.0 / n) / n)
    z_d = z((pd == 1).mean(0), gamma[:, 1].sum(1))
    z_l = z((pl == top[None, :]).mean(0), P[np.arange(len(top)), top])
    return z_d, z_l


@functools.lru_cache(maxsize=None)
def sample_reference(L, band, seed=0):
    """(data, transition, offsets, alpha32 (T, 2, L) float64 holding float32 values, gamma
    (T, 2, L), (path_d, path_l) of ffbs on alpha32 with uniforms()) of one case.  Shared:
    read only."""
    d, tr, off, (gamma, _, alpha, _) = R.segment_reference(L, band, LENS, seed)
    alpha32 = alpha.astype(np.float32).astype(np.float64)
    pd, pl = ffbs(alpha32, tr, off, uniforms())
    for v in (alpha32, pd, pl):
        v.setflags(write=False)
    return d, tr, off, alpha32, gamma, (pd, pl)
