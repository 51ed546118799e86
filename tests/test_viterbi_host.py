"""Host-side checks of the MAP (Viterbi) decoder: the float64 test reference against
exhaustive path enumeration, the C ABI's argument checks (no GPU needed) and the
host-side refusal of dense transitions."""
import ctypes

import numpy as np
import pytest

from poor_man_gplvm_amd import PoissonGPLVMJump1D, _native, banded_transition, viterbi_log_pi0
from tests import viterbi_ref as V


def _enumerate(u, logK0, logA, lp0):
    """Scores of all (2L)^T paths as a (2L,) * T array (state index d * L + l)."""
    T, L = u.shape
    S = 2 * L
    logK = np.stack([logK0, np.full((L, L), -np.log(L))])
    with np.errstate(invalid='ignore'):
        trans = (logA[:, :, None, None] + logK[None]).transpose(0, 2, 1, 3).reshape(S, S)   # [(d,i),(d',j)]
    ux = np.tile(u, (1, 2))                                                                 # (T, S)
    w = lp0.reshape(S) + ux[0]
    for t in range(1, T):
        w = w[..., None] + trans.reshape((1,) * (t - 1) + (S, S)) + ux[t]
    return w


def _random_case(seed, L, T, A):
    rng = np.random.default_rng(seed)
    K0 = rng.random((L, L)) + 0.05
    K0[rng.random((L, L)) < 0.25] = 0.0
    K0[np.arange(L), np.arange(L)] += 0.5          # no all-zero row
    K0 /= K0.sum(1, keepdims=True)
    with np.errstate(divide='ignore'):
        logK0, logA = np.log(K0), np.log(np.asarray(A, np.float64))
    u = rng.normal(size=(T, L)) * 3.0
    return u, logK0, logA, V.log_pi0(logK0, logA)


@pytest.mark.parametrize("seed,L,T,A", [
    (0, 4, 6, [[0.9, 0.1], [0.3, 0.7]]),
    (1, 3, 5, [[0.99, 0.01], [0.01, 0.99]]),
    (2, 4, 5, [[0.6, 0.4], [0.5, 0.5]]),
    (3, 4, 6, [[1.0, 0.0], [1.0, 0.0]]),           # the latent-only models' dynamics
])
def test_reference_matches_exhaustive_enumeration(seed, L, T, A):
    u, logK0, logA, lp0 = _random_case(seed, L, T, A)
    assert np.any(np.isinf(logK0))
    w = _enumerate(u, logK0, logA, lp0)
    best = np.unravel_index(int(np.argmax(w)), w.shape)
    path, score = V.viterbi(u, logK0, logA, lp0)
    assert [int(d) * L + int(l) for d, l in path] == [int(x) for x in best]
    assert abs(score - w[best]) <= 1e-12
    s2, M = V.path_score(path, u, logK0, logA, lp0)
    assert abs(s2 - w[best]) <= 1e-12
    assert np.isfinite(M) and M > 0


@pytest.mark.parametrize("L,mv,p", [(64, 1.0, (0.01, 0.01)), (100, 3.0, (0.2, 0.3)), (37, 0.5, (0.0, 1.0))])
def test_package_prior_matches_reference(L, mv, p):
    """gp_kernel.viterbi_log_pi0 (banded column sums) against the reference's dense form."""
    tr = banded_transition(L, mv, p[0], p[1])
    want = V.log_pi0(V.banded_logK(tr), V.device_logA(tr))
    got = viterbi_log_pi0(tr)
    assert got.shape == (2, L) and got.dtype == np.float64
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    assert np.array_equal(got[~fin], want[~fin])
    assert np.max(np.abs(got[fin] - want[fin])) <= 1e-12
    # a probability vector pushed through a (band-truncated) stochastic matrix whose g, invz
    # and A are each rounded to float32 (2^-24 relative apiece)
    assert np.exp(got).sum() <= 1.0 + 4 * 2.0 ** -24


def test_c_abi_workspace_and_argument_checks():
    lib = _native.load()
    one = lib.pmg_viterbi_workspace_size(1000, 512, 1)
    assert one >= 1000 * 512
    assert lib.pmg_viterbi_workspace_size(1000, 2000, 1) == 0       # L > 1024 unsupported
    assert lib.pmg_viterbi_workspace_size(0, 512, 1) == 0
    assert lib.pmg_viterbi_workspace_size(1000, 512, 0) == 0
    assert lib.pmg_viterbi_workspace_size(1000, 512, 3) > 2 * one > 0

    tr = _native.Transition()
    tr.L, tr.band = 64, 9
    one_ptr = ctypes.c_void_p(256)      # never dereferenced: every check precedes any HIP call

    def call(**kw):
        a = dict(delta=one_ptr, phi=one_ptr, rblk=one_ptr, T=10, R=1, tr=ctypes.byref(tr), log_pi0=one_ptr,
                 s=1.0, path_d=one_ptr, path_l=one_ptr, log_joint=one_ptr, ws=one_ptr, ws_bytes=1 << 30)
        a.update(kw)
        rc = lib.pmg_viterbi_decode(a['delta'], a['phi'], a['rblk'], a['T'], a['R'], a['tr'], a['log_pi0'], a['s'],
                                    a['path_d'], a['path_l'], a['log_joint'], a['ws'], a['ws_bytes'], None)
        return rc, lib.pmg_last_error()

    tr.invz = 256
    rc, msg = call(T=0)
    assert rc == -1 and b'T=0' in msg
    rc, msg = call(R=0)
    assert rc == -1 and b'R=0' in msg
    for name in ('delta', 'phi', 'rblk', 'log_pi0', 'path_d', 'path_l', 'log_joint'):
        rc, msg = call(**{name: None})
        assert rc == -1 and name.encode() in msg, (name, msg)
    rc, msg = call(ws=None)
    assert rc == -1 and b'workspace' in msg
    rc, msg = call(tr=None)
    assert rc == -1 and b'tr' in msg
    rc, msg = call(ws_bytes=16)
    assert rc == -1 and b'workspace_bytes' in msg
    tr.band = 40
    rc, msg = call()
    assert rc == -1 and b'band' in msg
    tr.band = 9
    tr.invz = None
    rc, msg = call()
    assert rc == -1 and b'invz' in msg


def test_workspace_sizes_of_the_two_entries_agree():
    """One carver serves both entries: R stacked sequences of T rows need what R segments over
    R T rows need, namely the back-pointer bytes, jump words, final states and f64 increments,
    each slice starting 256-byte aligned, plus 256; 0 on every degenerate argument."""
    lib = _native.load()
    seq, seg = lib.pmg_viterbi_workspace_size, lib.pmg_segment_viterbi_workspace_size

    def want(rows, L, chains):
        lpad = 64 * next(j for j in (1, 2, 4, 8, 16) if L <= 64 * j)
        off = 0
        for nbytes in (rows * lpad, 4 * rows, 8 * chains, 8 * rows):
            off = (off + 255) // 256 * 256 + nbytes
        return off + 256

    for T, L, R in [(1, 1, 1), (5, 65, 3), (200, 64, 7), (1000, 512, 1), (37, 1024, 65535), (3, 100, 2)]:
        assert seq(T, L, R) == seg(R * T, L, R) == want(R * T, L, R), (T, L, R)
    assert seg(200, 64, 70000) == want(200, 64, 70000)          # only the stacked entry bounds R
    for T, L, R in [(0, 64, 1), (-1, 64, 1), (10, 0, 1), (10, -5, 1), (10, 1025, 1), (10, 64, 0), (10, 64, -2)]:
        assert seq(T, L, R) == 0 and seg(T, L, R) == 0, (T, L, R)
    assert seq(10, 64, 65536) == 0


def test_dense_transition_is_refused_on_the_host():
    """A custom kernel, a band wider than 32 bins or n_latent_bin > 1024 resolve to the
    dense scans, which have no MAP decoder: NotImplementedError before any device object
    exists (this test runs without a GPU)."""
    rng = np.random.default_rng(0)
    N, L, T = 5, 16, 20
    y = rng.poisson(1.0, size=(T, N)).astype(np.float32)
    tun = rng.random((L, N)) + 0.1
    K = np.exp(-np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]) / 3.0)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, custom_transition_kernel=K)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        m.decode_latent_viterbi(y, tuning=tun)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        m.decode_latent_viterbi(y)          # the model's own tuning would need the device: never reached
    m = PoissonGPLVMJump1D(N, n_latent_bin=64)
    with pytest.raises(NotImplementedError, match="band"):
        m.decode_latent_viterbi(rng.poisson(1.0, size=(T, N)).astype(np.float32), tuning=rng.random((64, N)) + 0.1,
                                hyperparam={'movement_variance': 6.0})
