"""Float64 reference of the per-neuron circular spike shuffle (pmg_segment_roll_prepare /
shuffle_test_segments(shuffle='neuron_circular'); TEST INFRASTRUCTURE ONLY).

roll_segments is the shuffle itself on the host: a per-segment, per-neuron np.roll.  The
reference log marginal of a shuffle is the Poisson log-likelihood of the rolled counts in
float64 (the oracle's loglikelihood_poisson_all, as tests/segments_ref.py forms it), filtered
per segment by scan_ref.forward_backward on the flat-band transition of tests/scan_ref.py.

Inputs of a case (L, band): N = 24 neurons with planted place fields (a Gaussian bump of peak
rate 3 per bin over a floor of 0.2, centres spread evenly over the line, width L / 8 but at
least half a bin) and, per event of the ragged batch tests/segments_ref.LENS (120 rows), a
planted sweep of the latent from one end of the line to the other, so every event of more than
a few rows carries spikes of several neurons at different times -- the structure this shuffle
destroys.  With one latent bin the log marginal is the sum of the rows' log-likelihoods, which
no roll changes: L = 1 is in the accuracy cases and not in the discrimination condition.

The shuffle set is fixed: R = 6 shift arrays (6, S, 24) from default_rng(13),
  row 0  zero;                 row 1  each event's own length (the identity);
  row 2  uniform on [0, len);  row 3  negative, uniform on (-3 len, 0);
  row 4  beyond len, uniform on (len, 5 len];
  row 5  uniform on [-2^20, 2^20].
tests/test_neuron_shuffle_host.py checks that an implementation which ignores shift, rolls
by -k, or takes neuron n + 1's shift moves the reference far more than the GPU bar;
tests/test_gpu_neuron_shuffle.py runs the cases.
"""
import functools

import numpy as np

from oracle import gplvm_oracle as O
from tests import scan_ref as S
from tests import segments_ref as R

LENS = R.LENS
N_NEURON = 24
N_SHUFFLE = 6
SEED = 13
MUTATIONS = ('ignore_shift', 'negate', 'next_neuron')


def roll_segments(y, off, shift):
    """y (T, N) with neuron n of rows off[s]:off[s + 1] rolled circularly by shift[s, n]
    (np.roll along time: out[t] = in[t - k]); every other row as it was.  shift (S, N), any
    integers."""
    y = np.asarray(y)
    off = np.asarray(off, np.int64)
    shift = np.asarray(shift)
    n_s, n = len(off) - 1, y.shape[1]
    if shift.shape != (n_s, n):
        raise ValueError(f"shift must be {(n_s, n)}, got {shift.shape}")
    out = y.copy()
    for s in range(n_s):
        a, b = int(off[s]), int(off[s + 1])
        if b - a < 1:
            continue
        for j in range(n):
            out[a:b, j] = np.roll(y[a:b, j], int(shift[s, j]) % (b - a))
    return out


def mutated(shift, mutate):
    """The shifts a wrong implementation effectively applies (one of MUTATIONS; None: shift)."""
    shift = np.asarray(shift, np.int64)
    if mutate is None:
        return shift
    if mutate == 'ignore_shift':
        return np.zeros_like(shift)
    if mutate == 'negate':
        return -shift
    if mutate == 'next_neuron':
        return np.roll(shift, -1, axis=-1)
    raise ValueError(mutate)


@functools.lru_cache(maxsize=None)
def shifts():
    """(6, S, 24) int64 of the fixed set.  Shared: read only."""
    rng = np.random.default_rng(SEED)
    lens = np.asarray(LENS, np.int64)[:, None]
    shape = (len(LENS), N_NEURON)
    sh = np.zeros((N_SHUFFLE,) + shape, np.int64)
    sh[1] = lens
    sh[2] = np.floor(rng.random(shape) * lens)
    sh[3] = -1 - np.floor(rng.random(shape) * (3 * lens - 1))
    sh[4] = lens + 1 + np.floor(rng.random(shape) * 4 * lens)
    sh[5] = rng.integers(-2 ** 20, 2 ** 20 + 1, size=shape)
    assert np.all(sh[3] < 0) and np.all(sh[3] > -3 * lens) and np.all(sh[4] > lens) and np.all(sh[4] <= 5 * lens)
    sh.setflags(write=False)
    return sh


@functools.lru_cache(maxsize=None)
def planted_data(L, seed=0):
    """{'y' (120, 24) float32 counts, 'tuning' (L, 24) float64, 'B' basis, 'latent' (120,)}.
    Shared: read only."""
    off = R.offsets(LENS)
    T = int(off[-1])
    centre = (np.arange(N_NEURON) + 0.5) / N_NEURON * L - 0.5
    width = max(L / 8.0, 0.5)
    x = np.arange(L)[:, None]
    tuning = 0.2 + 3.0 * np.exp(-0.5 * ((x - centre[None, :]) / width) ** 2)
    rng = np.random.default_rng(seed + 40)
    lat = np.empty(T, np.int64)
    for s, n in enumerate(LENS):
        a = int(off[s])
        if n == 1:
            lat[a] = int(rng.integers(L))
        else:
            sweep = np.rint(np.linspace(0, L - 1, n)).astype(np.int64)
            lat[a:a + n] = sweep if s % 2 == 0 else sweep[::-1]
    y = rng.poisson(tuning[lat]).astype(np.float32)
    assert y.max() <= 127
    out = dict(y=y, tuning=tuning, B=S._basis(L), latent=lat)
    for v in out.values():
        v.setflags(write=False)
    return out


def rolled_logz(y, tuning, K, A, off, shift, likelihood_scale=1.0):
    """(R, S) float64: forward_backward's logZ of every segment of every host-rolled copy."""
    out = np.empty((shift.shape[0], len(off) - 1))
    for r in range(shift.shape[0]):
        ll = O.loglikelihood_poisson_all(roll_segments(y, off, shift[r]), tuning)
        for s in range(len(off) - 1):
            a, b = int(off[s]), int(off[s + 1])
            out[r, s] = S.forward_backward(ll[a:b], K, A, likelihood_scale)[1]
    return out


@functools.lru_cache(maxsize=None)
def neuron_shuffle_reference(L, band, seed=0, likelihood_scale=1.0, mutate=None):
    """(data, transition, offsets, shift (6, S, 24) int64, logz (6, S)) of one case on the fixed
    shuffle set.  mutate: the reference of a wrong implementation.  Shared: read only."""
    off = R.offsets(LENS)
    d = planted_data(L, seed)
    tr = S.flat_transition(L, band)
    sh = shifts()
    logz = rolled_logz(d['y'], d['tuning'], S.dense_K(tr), S.device_A(tr), off, mutated(sh, mutate),
                       likelihood_scale)
    logz.setflags(write=False)
    off.setflags(write=False)
    return d, tr, off, sh, logz


def eligible(y, off, shift):
    """Boolean (R, S): the (shuffle, event) pairs where a wrong implementation must differ --
    at least 3 rows, and two neurons that spike in the event whose effective shifts
    (shift mod len) differ."""
    shift = np.asarray(shift, np.int64)
    out = np.zeros(shift.shape[:2], bool)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        if b - a < 3:
            continue
        spiking = np.flatnonzero(np.asarray(y)[a:b].sum(0) > 0)
        for r in range(shift.shape[0]):
            out[r, s] = len(np.unique(shift[r, s, spiking] % (b - a))) >= 2
    return out
