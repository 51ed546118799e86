"""Fast float64 reference of the banded E-step and the flat-band inputs of the
(lanes x band) kernel matrix (TEST INFRASTRUCTURE ONLY).

forward_backward is the model of oracle.gplvm_oracle.smooth_all_step_combined_ma_chunk
in linear space: dense K (2, L, L) [d_next, i_prev, j_next], A (2, 2) [d_prev, d_next],
a uniform (d, l) state "at t = -1", every step re-normalised.  It is pinned to the oracle
in tests/test_scan_ref_host.py and costs milliseconds where the oracle's dense
log-sum-exp costs seconds, so one case per kernel instantiation stays affordable.

flat_transition is a continuous kernel whose taps all carry weight: g falls linearly
from 1 to about 0.5 at the band edge and is 0 beyond it, so a wrong outermost tap moves
the posterior by orders of magnitude more than the parity bars (the RBF kernel of
banded_transition is below 1e-5 of its peak over the outer half of its band).
wide_step_data draws a latent that uses the whole band, so MAP paths step by exactly
+-band.  The case tables of the GPU matrix tests live here too: the host test checks
their inputs, the GPU tests run them.
"""
import functools

import numpy as np

from oracle import gplvm_oracle as O
from poor_man_gplvm_amd.gp_kernel import MAX_BAND, BandedTransition
from tests import viterbi_ref as V

P_DYN = (0.05, 0.02)            # (p_move_to_jump, p_jump_to_move) of the matrix cases
RAGGED_L = {1: 61, 2: 127, 4: 250, 8: 500, 16: 1000}    # J latents per lane -> a ragged line
SCAN_WP = (5, 9, 13, 17, 25, 32)
VIT_WP = (5, 9, 17, 32)
N_NEURON = 16


# ----------------------------------------------------------------------------- transition
def flat_transition(L, band, pmj=P_DYN[0], pjm=P_DYN[1]):
    """BandedTransition with g[k] = 1 - 0.5 k / (band + 1) for k <= band (0 beyond),
    rows normalised over the line; g and invz float32 as the device holds them."""
    L, band = int(L), int(band)
    if not 0 <= band <= min(MAX_BAND, max(L - 1, 0)):
        raise ValueError(f"band {band} outside [0, min({MAX_BAND}, L - 1)]")
    g = (1.0 - 0.5 * np.arange(band + 1) / (band + 1)).astype(np.float32)
    i = np.arange(L)
    dist = np.abs(i[:, None] - i[None, :])
    z = np.where(dist <= band, g.astype(np.float64)[np.minimum(dist, band)], 0.0).sum(1)
    A = np.array([[1 - pmj, pmj], [pjm, 1 - pjm]], np.float64)
    return BandedTransition(L=L, band=band, g=g, invz=(1.0 / z).astype(np.float32), A=A,
                            movement_variance=float('nan'))


def dense_K(tr, drop_outer_tap=False):
    """(2, L, L) float64 kernels [d_next, i_prev, j_next] of a BandedTransition at its float32
    device values (as viterbi_ref.banded_logK): K[0] = g[|i-j|] * invz[i] within the band, 0
    beyond; K[1] = 1 / L.  drop_outer_tap: g[band] taken as 0 (invz unchanged), the kernel
    of a scan that loses its outermost tap."""
    L, band = int(tr.L), int(tr.band)
    g = np.asarray(tr.g, np.float32).astype(np.float64).copy()
    if drop_outer_tap:
        g[band] = 0.0
    invz = np.asarray(tr.invz, np.float32).astype(np.float64)
    i = np.arange(L)
    dist = np.abs(i[:, None] - i[None, :])
    K0 = np.where(dist <= band, g[np.minimum(dist, band)] * invz[:, None], 0.0)
    return np.stack([K0, np.full((L, L), 1.0 / L)])


def device_A(tr):
    """(2, 2) float64 dynamics matrix at its float32 device values."""
    return np.asarray(tr.A, np.float64).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- reference
def forward_backward(ll, K, A, likelihood_scale=1.0):
    """ll (T, L) log-likelihood.  Returns (gamma (T, 2, L), logZ, alpha (T, 2, L), logc (T,)):
    smoothed and filtered posteriors and the log one-step predictive marginals."""
    ll = np.asarray(ll, np.float64)
    K = np.asarray(K, np.float64)
    A = np.asarray(A, np.float64)
    T, L = ll.shape
    post = np.full((2, L), 1.0 / (2 * L))
    alpha = np.empty((T, 2, L))
    prior = np.empty((T, 2, L))
    logc = np.empty(T)
    for t in range(T):
        a = A.T @ post                                        # [d', i]
        prior[t, 0] = a[0] @ K[0]
        prior[t, 1] = a[1] @ K[1]
        x = likelihood_scale * ll[t]
        m = x.max()
        u = prior[t] * np.exp(x - m)[None, :]
        c = u.sum()
        post = u / c
        alpha[t] = post
        logc[t] = np.log(c) + m
    gamma = np.empty((T, 2, L))
    gamma[T - 1] = alpha[T - 1]
    for t in range(T - 2, -1, -1):
        r = np.divide(gamma[t + 1], prior[t + 1], out=np.zeros((2, L)), where=prior[t + 1] > 0)
        v = np.stack([K[0] @ r[0], K[1] @ r[1]])              # [d', i]
        gamma[t] = alpha[t] * (A @ v)
    return gamma, float(logc.sum()), alpha, logc


# ----------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def _basis(L):
    return O.generate_basis(10.0, L).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wide_step_data(N, L, T, band, seed=0):
    """Basis and tuning of tests/synth.make; a latent that steps uniformly in [-band, band]
    (reflected at the ends of the line) and teleports uniformly on about 5 % of the steps;
    Poisson spikes from the oracle's sampler.  The returned arrays are shared: read only."""
    B = _basis(L)
    W = np.random.default_rng(seed).normal(size=(B.shape[1], N))
    tun = O.get_tuning_softplus(W, B)
    rng = np.random.default_rng(seed + 1)
    lat = np.empty(T, np.int64)
    l = int(rng.integers(L))
    step = rng.integers(-band, band + 1, size=T)
    jump = rng.random(T) < 0.05
    dest = rng.integers(L, size=T)
    for t in range(T):
        if jump[t]:
            l = int(dest[t])
        else:
            l += int(step[t])
            if l < 0:
                l = -l
            if l > L - 1:
                l = 2 * (L - 1) - l
        lat[t] = l
    assert lat.min() >= 0 and lat.max() < L
    y = O.sample_spikes(tun, lat, np.random.default_rng(seed + 2)).astype(np.float32)
    out = dict(y=y, B=B, tuning=tun, latent=lat, jump=jump)
    for v in out.values():
        v.setflags(write=False)
    return out


# ----------------------------------------------------------------------------- scan cases
def host_J(L):
    """Host mirror of the kernels' latents-per-lane choice (pmg_fwdbwd_lpad(L) / 64)."""
    for J in (1, 2, 4, 8, 16):
        if L <= 64 * J:
            return J
    raise ValueError(L)


def wp_interval(WP, table):
    """(lo, hi]: the bands a kernel set WP of `table` (SCAN_WP / VIT_WP) serves."""
    k = table.index(WP)
    return (table[k - 1] if k else -1), WP


def scan_runs(J, WP):
    """The two runs of scan pair (J, WP): dicts of L, band, T, chunk, warmup, seed."""
    return dict(
        ragged=dict(L=RAGGED_L[J], band=WP - 2, T=56, chunk=16, warmup=0, seed=0),
        full=dict(L=64 * J, band=WP, T=56, chunk=24, warmup=8, seed=0),
    )


SCAN_PAIRS = [(J, WP) for J in RAGGED_L for WP in SCAN_WP]
TINY_L = (1, 2, 3, 8, 33)


def tiny_run(L):
    return dict(L=L, band=min(L - 1, MAX_BAND), T=40, chunk=16, warmup=0, seed=0)


@functools.lru_cache(maxsize=None)
def scan_reference(L, band, T, seed, likelihood_scale=1.0, rbf_mv=None):
    """(data, transition, (gamma, logZ, alpha, logc)) of one run; rbf_mv: the package's RBF
    transition at that movement variance in place of the flat band."""
    d = wide_step_data(N_NEURON, L, T, band, seed)
    if rbf_mv is None:
        tr = flat_transition(L, band)
    else:
        from poor_man_gplvm_amd.gp_kernel import banded_transition
        tr = banded_transition(L, rbf_mv, *P_DYN)
        assert tr.band == band
    ll = O.loglikelihood_poisson_all(d['y'], d['tuning'])
    ref = forward_backward(ll, dense_K(tr), device_A(tr), likelihood_scale)
    for v in (ref[0], ref[2], ref[3]):
        v.setflags(write=False)
    return d, tr, ref


# ----------------------------------------------------------------------------- Viterbi cases
VIT_PAIRS = [(J, WP) for J in RAGGED_L for WP in VIT_WP]
VIT_TINY_L = (2, 8, 33)
# (L, band) -> (data seed, (p_move_to_jump, p_jump_to_move)) where seed 0 with P_DYN does not
# meet the input conditions checked in tests/test_scan_ref_host.py (a +-band step and a
# jump on the reference path, the path unchanged by rounding u to float32, the truncated
# optimum lower by more than B).  Where the band spans half the line or all of it, the
# continuous kernel reaches almost every latent and the MAP path never pays P_DYN's price
# for a change of dynamics: those cases take a faster-switching A.
VIT_INPUT = {
    (61, 7): (4, P_DYN), (61, 15): (15, P_DYN), (127, 15): (2, P_DYN), (250, 30): (4, P_DYN),
    (61, 30): (5, (0.2, 0.3)), (127, 30): (0, (0.2, 0.3)),
    (2, 1): (0, (0.3, 0.3)), (8, 7): (0, (0.3, 0.3)), (33, 32): (0, (0.3, 0.3)),
}


def _vit_run(L, band, T):
    seed, p = VIT_INPUT.get((L, band), (0, P_DYN))
    return dict(L=L, band=band, T=T, seed=seed, p=p)


def vit_run(J, WP):
    return _vit_run(RAGGED_L[J], WP - 2, 300 if J == 16 else 400)


def vit_tiny_run(L):
    return _vit_run(L, min(L - 1, MAX_BAND), 400)


@functools.lru_cache(maxsize=None)
def vit_inputs(L, band, T, seed, p=P_DYN):
    """(data, transition, u (T, L) float64 oracle emission) of one Viterbi case."""
    d = wide_step_data(N_NEURON, L, T, band, seed)
    tr = flat_transition(L, band, *p)
    u = O.loglikelihood_poisson_all(d['y'], d['tuning'])
    u.setflags(write=False)
    return d, tr, u


def vit_reference(tr, u, drop_outer_tap=False):
    """(path, score, M) of the float64 reference Viterbi on the device transition."""
    logK0, logA = V.banded_logK(tr), V.device_logA(tr)
    if drop_outer_tap:
        i = np.arange(tr.L)
        logK0 = np.where(np.abs(i[:, None] - i[None, :]) == tr.band, -np.inf, logK0)
    lp0 = V.log_pi0(V.banded_logK(tr), logA)
    path, score = V.viterbi(u, logK0, logA, lp0)
    _, M = V.path_score(path, u, V.banded_logK(tr), logA, lp0)
    return path, score, M
