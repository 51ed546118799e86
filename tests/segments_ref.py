"""Case tables and the per-segment float64 reference of the segment smoother
(pmg_segment_smoother / decode_latent_segments; TEST INFRASTRUCTURE ONLY).

The reference of a ragged batch is scan_ref.forward_backward on each segment's slice of the
log-likelihood, on the flat-band transition and the wide-step data of tests/scan_ref.py (a
lost outermost tap, or a filter that runs across a segment boundary, moves it by orders of
magnitude more than the parity bars: tests/test_segments_host.py checks both for every
case below).  The host test checks the inputs, the GPU tests run them.

LENS is the standard ragged batch (120 rows).  The segment kernels prefetch rows through
register rings 2, 4 or 8 deep (seg_pf_fwd / seg_pf_bwd in csrc/segments.hip), clamped to
the segment's own rows, so it holds
  a one-row segment (no backward step), first and last but one;
  lengths on both sides of every ring depth in use: 1 2 3, 3 4 5, 7 8 9;
  lengths beyond twice the deepest ring: 17, 33 (and 16 = exactly two rings);
  short segments after long ones (2, 1 after 33);
  a last segment that ends on the buffer's last row.
"""
import functools

import numpy as np

from oracle import gplvm_oracle as O
from tests import scan_ref as S

LENS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 2, 1, 12)
RING_DEPTHS = (2, 4, 8)
SEG_WP = S.VIT_WP                       # the segment kernels use the Viterbi band table
SEG_PAIRS = [(J, WP) for J in S.RAGGED_L for WP in SEG_WP]
TINY_L = (1, 2, 3, 8, 33)
N_NEURON = S.N_NEURON


def offsets(lens=LENS):
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(np.asarray(lens, np.int64), out=off[1:])
    return off


def seg_runs(J, WP):
    """The two runs of pair (J, WP), as scan_ref.scan_runs has them: a ragged line with a
    zero-padded band and a full-lane line at the widest band of the kernel set."""
    return dict(ragged=dict(L=S.RAGGED_L[J], band=WP - 2, seed=0),
                full=dict(L=64 * J, band=WP, seed=0))


def tiny_run(L):
    return dict(L=L, band=min(L - 1, S.MAX_BAND), seed=0)


ALL_RUNS = [r for J, WP in SEG_PAIRS for r in seg_runs(J, WP).values()] + [tiny_run(L) for L in TINY_L]


@functools.lru_cache(maxsize=None)
def _inputs(L, band, T, seed):
    d = S.wide_step_data(N_NEURON, L, T, band, seed)
    tr = S.flat_transition(L, band)
    ll = O.loglikelihood_poisson_all(d['y'], d['tuning'])
    ll.setflags(write=False)
    return d, tr, ll


def _per_segment(ll, K, A, off, likelihood_scale):
    T, L = ll.shape
    gamma, alpha = np.empty((T, 2, L)), np.empty((T, 2, L))
    logc, logz = np.empty(T), np.empty(len(off) - 1)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        gamma[a:b], logz[s], alpha[a:b], logc[a:b] = S.forward_backward(ll[a:b], K, A, likelihood_scale)
    return gamma, logz, alpha, logc


@functools.lru_cache(maxsize=None)
def segment_reference(L, band, lens=LENS, seed=0, likelihood_scale=1.0):
    """(data, transition, offsets, (gamma (T, 2, L), logz (S,), alpha (T, 2, L), logc (T,)))
    of one ragged batch: every segment smoothed on its own.  Shared: read only."""
    off = offsets(lens)
    d, tr, ll = _inputs(L, band, int(off[-1]), seed)
    ref = _per_segment(ll, S.dense_K(tr), S.device_A(tr), off, likelihood_scale)
    for v in ref:
        v.setflags(write=False)
    off.setflags(write=False)
    return d, tr, off, ref


def lost_tap_reference(L, band, lens=LENS, seed=0):
    """The per-segment reference of a scan that loses its outermost tap."""
    off = offsets(lens)
    _, tr, ll = _inputs(L, band, int(off[-1]), seed)
    return _per_segment(ll, S.dense_K(tr, drop_outer_tap=True), S.device_A(tr), off, 1.0)


def concatenated_reference(L, band, lens=LENS, seed=0):
    """The reference of ONE chain over all the rows (the filter run across the gaps)."""
    off = offsets(lens)
    _, tr, ll = _inputs(L, band, int(off[-1]), seed)
    return S.forward_backward(ll, S.dense_K(tr), S.device_A(tr))
