"""Float64 reference of the shuffle log marginals (pmg_segment_shuffle_logz /
shuffle_test_segments; TEST INFRASTRUCTURE ONLY).

For a case (L, band) the log-likelihood ll (120, L) is that of tests/segments_ref._inputs (the
flat-band transition and the wide-step data of tests/scan_ref.py).  Shuffle r is applied in
float64 -- ll[perm[r]], then np.take_along_axis with (l + rot[r, t]) % L -- and every segment
of the ragged batch tests/segments_ref.LENS is filtered on its own by
scan_ref.forward_backward, whose logZ is the reference value.

The shuffle set is fixed: R = 8 rows from default_rng(11) over the 120 rows,
  rows 0-2  perm only (rot = 0): within-segment permutations,
  rows 3-4  rot only (perm = identity),
  rows 5-7  both,
with rot[r, t] = floor(v[r, t] L) for one uniform draw v, so the set is the same for every L.
tests/test_shuffle_segments_host.py checks that a scan which ignores perm, ignores rot, or clamps
l + rot where it should wrap moves these values by far more than the GPU bar;
tests/test_gpu_shuffle_segments.py runs them.
"""
import functools

import numpy as np

from tests import scan_ref as S
from tests import segments_ref as R

LENS = R.LENS
N_SHUFFLE = 8
PERM_ROWS = (0, 1, 2, 5, 6, 7)
ROT_ROWS = (3, 4, 5, 6, 7)
SEED = 11
MUTATIONS = ('ignore_perm', 'ignore_rot', 'clamp_rot')


@functools.lru_cache(maxsize=None)
def _draws():
    rng = np.random.default_rng(SEED)
    off = R.offsets(LENS)
    n = int(off[-1])
    perm = np.tile(np.arange(n, dtype=np.int32), (N_SHUFFLE, 1))
    for r in PERM_ROWS:
        for s in range(len(LENS)):
            a, b = int(off[s]), int(off[s + 1])
            perm[r, a:b] = a + rng.permutation(b - a)
    v = rng.random((N_SHUFFLE, n))
    for r in range(N_SHUFFLE):
        if r not in ROT_ROWS:
            v[r] = 0.0
    perm.setflags(write=False)
    v.setflags(write=False)
    return perm, v


def shuffles(L):
    """(perm, rot) (8, 120) int32 of the fixed set for a line of L latents.  Shared: read only."""
    perm, v = _draws()
    rot = np.floor(v * L).astype(np.int32)
    assert rot.min() >= 0 and rot.max() < L
    rot.setflags(write=False)
    return perm, rot


def shuffled_ll(ll, perm_r, rot_r, mutate=None):
    """One shuffle of the log-likelihood in float64: row t takes ll[perm_r[t]], latent l of it
    the source row's latent (l + rot_r[t]) % L.  mutate: one of MUTATIONS (a wrong scan)."""
    ll = np.asarray(ll, np.float64)
    T, L = ll.shape
    src = np.arange(T) if mutate == 'ignore_perm' else np.asarray(perm_r, np.int64)
    rt = np.zeros(T, np.int64) if mutate == 'ignore_rot' else np.asarray(rot_r, np.int64)
    col = np.arange(L)[None, :] + rt[:, None]
    col = np.minimum(col, L - 1) if mutate == 'clamp_rot' else col % L
    return np.take_along_axis(ll[src], col, axis=1)


def shuffle_logz(ll, K, A, off, perm, rot, likelihood_scale=1.0, mutate=None):
    """(R, S) float64: scan_ref.forward_backward's logZ of every segment of every shuffle."""
    out = np.empty((perm.shape[0], len(off) - 1))
    for r in range(perm.shape[0]):
        x = shuffled_ll(ll, perm[r], rot[r], mutate)
        for s in range(len(off) - 1):
            a, b = int(off[s]), int(off[s + 1])
            out[r, s] = S.forward_backward(x[a:b], K, A, likelihood_scale)[1]
    return out


@functools.lru_cache(maxsize=None)
def shuffle_reference(L, band, seed=0, likelihood_scale=1.0, pmj=S.P_DYN[0], pjm=S.P_DYN[1], mutate=None):
    """(data, transition, offsets, perm, rot, logz (8, S)) of one case on the fixed shuffle set.
    Shared: read only."""
    off = R.offsets(LENS)
    d, _, ll = R._inputs(L, band, int(off[-1]), seed)
    tr = S.flat_transition(L, band, pmj, pjm)
    perm, rot = shuffles(L)
    logz = shuffle_logz(ll, S.dense_K(tr), S.device_A(tr), off, perm, rot, likelihood_scale, mutate)
    logz.setflags(write=False)
    off.setflags(write=False)
    return d, tr, off, perm, rot, logz


def eligible(off, perm, rot):
    """Boolean (R, S) masks (perm_pairs, rot_pairs) of the pairs where a scan that ignores perm /
    mishandles rot must differ: perm -- a perm row, length >= 3, the segment's permutation
    neither the identity nor the reversal (a reversed chain's marginal is nearly the same);
    rot -- a rot row, length >= 2."""
    n_r, n_s = perm.shape[0], len(off) - 1
    ep = np.zeros((n_r, n_s), bool)
    er = np.zeros((n_r, n_s), bool)
    for s in range(n_s):
        a, b = int(off[s]), int(off[s + 1])
        ident = np.arange(a, b)
        for r in range(n_r):
            p = perm[r, a:b]
            ep[r, s] = (r in PERM_ROWS and b - a >= 3 and not np.array_equal(p, ident)
                        and not np.array_equal(p, ident[::-1]))
            er[r, s] = r in ROT_ROWS and b - a >= 2
    return ep, er
