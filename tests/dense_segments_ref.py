"""Inputs and the per-segment float64 reference of the dense segment smoother
(pmg_dense_segment_smoother / decode_latent_segments(exact=True); TEST INFRASTRUCTURE ONLY).

The continuous kernel is a *shifted*, hence asymmetric, custom kernel: a scan that reads
it transposed moves every event, as does a chain that runs across the event boundaries
(tests/test_dense_segments_host.py checks both on exactly these inputs).  The reference of a
ragged batch is oracle.gplvm_oracle.decode_latent's smoother on each segment's rows alone
(oracle_segment).  Everything here is computed once and shared read only."""
import functools

import numpy as np

from oracle import gplvm_oracle as O
from tests import segments_ref as SR
from tests.synth import make

N_NEURON = 30
LENS = SR.LENS                    # 14 events, 120 rows
SHORT = (1, 2, 5)
FULL_L = (1, 2, 3, 33, 61, 80, 256, 257)     # JD = 1: ragged and full thread lines; first JD = 2 line
SHORT_L = (512, 513, 1025, 2049)             # the first lines of JD = 2, 4, 8 and 16
BITWISE_L = (61, 300)
offsets = SR.offsets


def custom_kernel(L, seed=5):
    """K[i, j] (previous latent i, next latent j) = exp(-|j - i - 1.5| / 3) + 0.02 U(0, 1)."""
    rng = np.random.default_rng(seed)
    i = np.arange(L)
    return np.exp(-np.abs(i[None, :] - i[:, None] - 1.5) / 3.0) + 0.02 * rng.random((L, L))


@functools.lru_cache(maxsize=None)
def inputs(L, lens=LENS):
    """(data of synth.make(30, L, Ttot), custom kernel (L, L), offsets (S + 1,))."""
    off = offsets(lens)
    d = make(N_NEURON, L, int(off[-1]))
    K = custom_kernel(L)
    for v in (d['y'], d['tuning'], K, off):
        v.setflags(write=False)
    return d, K, off


def _log_kernels(L, K, **kw):
    _, logK, _, logA = O.create_transition_prob_1d(L, custom_kernel=K, **kw)
    return logK, logA


def _pack(parts, off):
    """Per-segment results -> arrays over the compact rows (logz: one value per segment)."""
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != 'logz'}
    out['logz'] = np.array([p['logz'] for p in parts], np.float64)
    for v in out.values():
        v.setflags(write=False)
    return out


def oracle_segment(y, tuning, logK, logA, **kw):
    """One segment through the smoother oracle.decode_latent runs
    (smooth_all_step_combined_ma_chunk), without the pairwise joint that no test here reads
    (at L = 2049 accumulating it takes three quarters of the time): the same arithmetic,
    and test_dense_segments_host.py checks that the values equal decode_latent's bit for bit.
    The filter posteriors, which decode_latent does not return, come from the same call."""
    lpa, lz, lca, cs, _, _ = O.smooth_all_step_combined_ma_chunk(
        np.asarray(y, np.float64), np.asarray(tuning, np.float64), logK, logA, with_joint=False, **kw)
    return dict(gamma=np.exp(lpa), log_gamma=lpa, alpha=np.exp(lca), logc=cs, logz=float(lz))


@functools.lru_cache(maxsize=None)
def reference(L, lens=LENS, likelihood_scale=1.0):
    """{'gamma', 'log_gamma', 'alpha' (T, 2, L), 'logc' (T,), 'logz' (S,)}: every segment
    decoded on its own by the float64 oracle."""
    d, K, off = inputs(L, lens)
    logK, logA = _log_kernels(L, K)
    return _pack([oracle_segment(d['y'][int(a):int(b)], d['tuning'], logK, logA, likelihood_scale=likelihood_scale)
                  for a, b in zip(off[:-1], off[1:])], off)


def _smooth(y, tuning, logK, logA):
    lpa = O.smooth_all_step_combined_ma_chunk(np.asarray(y, np.float64), np.asarray(tuning, np.float64), logK, logA,
                                              with_joint=False)[0]
    return np.exp(lpa)


def transposed_posterior(L, lens=LENS):
    """The per-segment posteriors (T, 2, L) of a scan that reads the log kernel transposed."""
    d, K, off = inputs(L, lens)
    logK, logA = _log_kernels(L, K)
    logK = np.stack([logK[0].T, logK[1]])
    return np.concatenate([_smooth(d['y'][int(a):int(b)], d['tuning'], logK, logA)
                           for a, b in zip(off[:-1], off[1:])])


def concatenated_posterior(L, lens=LENS):
    """The posteriors (T, 2, L) of ONE chain over all the rows (the filter run across the gaps)."""
    d, K, off = inputs(L, lens)
    logK, logA = _log_kernels(L, K)
    return _smooth(d['y'], d['tuning'], logK, logA)


def per_event_max(diff, off):
    """(S,) max |diff| over each event's rows."""
    return np.array([np.abs(diff[int(a):int(b)]).max() for a, b in zip(off[:-1], off[1:])])


JUMP_T, JUMP_ROW0 = 1500, 600


@functools.lru_cache(maxsize=None)
def jump_data(N=N_NEURON, L=100):
    """(synth.make(N, L, 1500) data, segments (14, 2)): the latent path is sampled WITH
    jumps, and the LENS batch is laid over rows 600 .. 719, where it makes far moves (the
    jump state holds from row 631 to row 662)."""
    d = make(N, L, JUMP_T)
    d['y'].setflags(write=False)
    d['tuning'].setflags(write=False)
    off = offsets() + JUMP_ROW0
    seg = np.stack([off[:-1], off[1:]], 1)
    far = np.flatnonzero(np.abs(np.diff(d['latent'][:, 1])) > 10)
    assert np.sum((far >= seg[0, 0]) & (far < seg[-1, 1] - 1)) >= 10
    return d, seg
