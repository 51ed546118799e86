"""Host checks of tests/scan_ref.py (no GPU):

  1. the fast linear-space reference against the oracle's log-domain smoother: gamma, alpha
     and logc within 1e-11 relative (+ 1e-300), logZ within 1e-12 relative -- about 1000
     times the agreement measured (gamma 2e-14, logZ 4e-16), which leaves room for the
     oracle's own logsumexp rounding;
  2. the inputs of every case of the GPU matrices (tests/test_gpu_scan_matrix.py,
     tests/test_gpu_viterbi_matrix.py): each reaches the intended (J, WP) kernel set, and
     a kernel that lost only its outermost band tap would miss the GPU tests' bars by a
     wide margin -- the posterior moves by >= 100 times the close_prob bar, the Viterbi
     optimum falls by more than the rounding bound B, and the reference MAP path takes
     steps of exactly +-band and jumps.
"""
import numpy as np
import pytest

from oracle import gplvm_oracle as O
from poor_man_gplvm_amd import _native, banded_transition
from tests import scan_ref as S
from tests.synth import make

RT, AT = 1e-5, 1e-12        # close_prob of tests/test_gpu_parity.py


def _log(x):
    with np.errstate(divide='ignore'):
        return np.log(x)


def _pin(y, tuning, K, A, s=1.0, ma_latent=None):
    lpa, lz, lca, cs, _, ll = O.smooth_all_step_combined_ma_chunk(
        y, tuning, _log(K), _log(A), ma_latent=ma_latent, likelihood_scale=s, with_joint=False)
    gamma, logz, alpha, logc = S.forward_backward(ll, K, A, s)
    for name, got, want in (('gamma', gamma, np.exp(lpa)), ('alpha', alpha, np.exp(lca)), ('logc', logc, cs)):
        err = np.abs(got - want)
        rel = np.max(err / np.maximum(np.abs(want), 1e-280))
        print(f"{name}: max abs {err.max():.3e} max rel {rel:.3e}")
        assert np.all(err <= 1e-11 * np.abs(want) + 1e-300), name
    print(f"logZ: rel {abs(logz - lz) / abs(lz):.3e}")
    assert abs(logz - lz) <= 1e-12 * abs(lz)
    assert np.all(np.abs(gamma.sum((1, 2)) - 1.0) <= 1e-12)


@pytest.mark.parametrize("T", [300, 1, 2])
def test_reference_matches_oracle_rbf(T):
    N, L = 30, 100
    d = make(N, L, T)
    K, _, A, _ = O.create_transition_prob_1d(L, 1.0)
    _pin(d['y'], d['tuning'], K, A)


def test_reference_matches_oracle_flat_band_scaled():
    L, T, band = 127, 200, 11
    d = S.wide_step_data(S.N_NEURON, L, T, band)
    tr = S.flat_transition(L, band, 0.05, 0.02)
    _pin(d['y'], d['tuning'], S.dense_K(tr), S.device_A(tr), s=0.7)


def test_reference_matches_oracle_masked_latents():
    L, T, band = 80, 150, 9
    d = S.wide_step_data(S.N_NEURON, L, T, band, seed=3)
    ml = np.ones(L)
    ml[np.random.default_rng(2).choice(L, 30, replace=False)] = 0
    tr = S.flat_transition(L, band)
    _pin(d['y'], d['tuning'], S.dense_K(tr), S.device_A(tr), ma_latent=ml)


def test_flat_transition_is_row_stochastic_and_flat():
    tr = S.flat_transition(250, 30)
    assert tr.g.dtype == np.float32 and tr.invz.dtype == np.float32 and tr.g.shape == (31,)
    assert tr.g[0] == 1.0 and 0.5 < tr.g[-1] < 0.52 and np.all(np.diff(tr.g) < 0)
    K = S.dense_K(tr)
    assert np.all(np.abs(K.sum(2) - 1.0) <= 1e-6)
    i = np.arange(250)
    assert np.all((K[0] > 0) == (np.abs(i[:, None] - i[None, :]) <= 30))
    assert np.array_equal(S.dense_K(tr, True)[0] > 0, np.abs(i[:, None] - i[None, :]) < 30)


def test_wide_step_data_uses_the_whole_band():
    d = S.wide_step_data(S.N_NEURON, 250, 400, 15)
    step = np.abs(np.diff(d['latent']))[~d['jump'][1:]]
    assert step.max() == 15 and np.sum(step == 15) >= 10
    assert 5 <= d['jump'].sum() <= 40
    assert d['y'].dtype == np.float32 and d['y'].shape == (400, S.N_NEURON)


# ----------------------------------------------------------------------------- matrix inputs
def _lib_J(L):
    lpad = int(_native.load().pmg_fwdbwd_lpad(L))
    assert lpad % 64 == 0
    return lpad // 64


def _outer_tap_shift(run):
    """max over cells of |gamma(outer tap dropped) - gamma| / close_prob's bar."""
    d, tr, (gamma, *_) = S.scan_reference(run['L'], run['band'], run['T'], run['seed'])
    ll = O.loglikelihood_poisson_all(d['y'], d['tuning'])
    cut = S.forward_backward(ll, S.dense_K(tr, drop_outer_tap=True), S.device_A(tr))[0]
    return float(np.max(np.abs(cut - gamma) / (RT * np.abs(gamma) + AT)))


@pytest.mark.parametrize("J,WP", S.SCAN_PAIRS)
def test_scan_case_inputs(J, WP):
    lo, hi = S.wp_interval(WP, S.SCAN_WP)
    for name, run in S.scan_runs(J, WP).items():
        assert lo < run['band'] <= hi and run['band'] < run['L']
        assert S.host_J(run['L']) == J and _lib_J(run['L']) == J
        assert (run['band'] < WP) == (name == 'ragged')
        assert (run['L'] % 32 != 0) == (name == 'ragged')
        assert (run['T'] % run['chunk'] != 0) and run['T'] > 2 * run['chunk']
        ratio = _outer_tap_shift(run)
        print(f"J={J} WP={WP} {name}: outer tap moves gamma by {ratio:.3g} x the close_prob bar")
        assert ratio >= 100.0


@pytest.mark.parametrize("L", S.TINY_L)
def test_tiny_scan_case_inputs(L):
    run = S.tiny_run(L)
    assert run['band'] == min(L - 1, 32) and S.host_J(L) == 1 and _lib_J(L) == 1
    ratio = _outer_tap_shift(run)
    print(f"L={L}: outer tap moves gamma by {ratio:.3g} x the close_prob bar")
    assert ratio >= 100.0


def test_tiny_rbf_case_is_clamped_to_the_line():
    """banded_transition(8, 1.0): the RBF band of 9 clamped to L - 1 = 7.  Its outer taps
    are below 1e-20, so this case covers the clamp, not the outer taps."""
    tr = banded_transition(8, 1.0, *S.P_DYN)
    assert tr.band == 7 and tr.g.shape == (8,)
    S.scan_reference(8, 7, 40, 0, rbf_mv=1.0)


def _vit_inputs_ok(run):
    d, tr, u = S.vit_inputs(run['L'], run['band'], run['T'], run['seed'], run['p'])
    T, band = run['T'], run['band']
    path, score, M = S.vit_reference(tr, u)
    dl = np.abs(np.diff(path[:, 1].astype(np.int64)))
    cont = path[1:, 0] == 0
    n_edge, n_jump = int(np.sum(dl[cont] == band)), int(np.sum(~cont))
    assert np.all(dl[cont] <= band)
    path32 = S.vit_reference(tr, u.astype(np.float32).astype(np.float64))[0]
    cut_path, cut_score, cut_M = S.vit_reference(tr, u, drop_outer_tap=True)
    B = 16.0 * T * 2.0 ** -24 * max(M, cut_M)
    print(f"L={run['L']} band={band} T={T} seed={run['seed']} p={run['p']}: {n_edge} steps of +-band, {n_jump} jump steps, "
          f"truncated optimum lower by {score - cut_score:.3f} nats, B={B:.2e}, "
          f"f32-u path differs in {int(np.sum(np.any(path32 != path, axis=1)))} bins")
    assert n_edge >= 1 and n_jump >= 1
    assert np.array_equal(path32, path)
    assert score - cut_score > B


@pytest.mark.parametrize("J,WP", S.VIT_PAIRS)
def test_viterbi_case_inputs(J, WP):
    run = S.vit_run(J, WP)
    lo, hi = S.wp_interval(WP, S.VIT_WP)
    assert lo < run['band'] <= hi and WP - run['band'] == 2
    assert S.host_J(run['L']) == J and _lib_J(run['L']) == J
    assert int(0.005 * run['T']) >= 1
    _vit_inputs_ok(run)


@pytest.mark.parametrize("L", S.VIT_TINY_L)
def test_tiny_viterbi_case_inputs(L):
    run = S.vit_tiny_run(L)
    assert S.host_J(L) == 1 and run['band'] == min(L - 1, 32)
    _vit_inputs_ok(run)


def test_single_latent_kernels_are_exactly_one():
    """L = 1: continuous and jump kernels are both exactly 1, so no datum separates the two
    dynamics; the GPU case checks feasibility, optimality and the score, not agreement."""
    tr = S.flat_transition(1, 0)
    K = S.dense_K(tr)
    assert np.all(K == 1.0) and tr.invz[0] == 1.0
