"""decode_latent_viterbi on the device against the float64 reference (tests/viterbi_ref.py)
on the same banded transition, with the oracle's float64 emission.

Every case checks
  (a) feasibility: continuous steps stay within the band, no masked latent, indices in range;
  (b) optimality: score_f64(reference path) - score_f64(device path) <= B = 16 T 2^-24 M,
      M the largest absolute per-step increment along either path.  The device takes the
      exact maximiser of scores evaluated in f32: each step adds three f32 terms and
      re-centres once, <= ~4 * 2^-24 M per step and path, twice (two paths), and 2x for
      the f32 rounding of delta and phi;
  (c) agreement: at most 0.5 % of the time bins differ from the reference path;
  (d) score: log_joint_map equals score_f64(device path) within B and is
      <= log_marginal_final of decode_marginals (slack 1e-6 |logZ|).
"""
import functools

import numpy as np
import pytest

from oracle import gplvm_oracle as O
from poor_man_gplvm_amd import (GaussianGPLVMJump1D, PoissonGPLVM1D, PoissonGPLVMJump1D, banded_transition)
from tests import viterbi_ref as V
from tests.synth import make

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _data(N, L, T, mv=1.0, seed=0):
    return make(N, L, T, mv=mv, seed=seed)


def _check(res, u, tr, logz, ma_latent=None, latent_only=False):
    """Conditions (a)-(d) for one sequence; returns the device path (T, 2)."""
    T, L = u.shape
    logK0, logA = V.banded_logK(tr), V.device_logA(tr)
    lp0 = V.log_pi0(logK0, logA)
    ref_path, ref_score = V.viterbi(u, logK0, logA, lp0)
    l = np.asarray(res['map_latent'])
    assert l.shape == (T,) and l.dtype == np.int32
    if latent_only:
        assert 'map_dynamics' not in res
        d = np.zeros(T, np.int32)
    else:
        d = np.asarray(res['map_dynamics'])
        assert d.shape == (T,) and d.dtype == np.int32
    # (a)
    assert l.min() >= 0 and l.max() < L and d.min() >= 0 and d.max() <= 1
    cont = d[1:] == 0
    assert np.all(np.abs(np.diff(l.astype(np.int64)))[cont] <= tr.band)
    if ma_latent is not None:
        assert np.all(np.asarray(ma_latent).astype(bool)[l])
    # (b)
    path = np.stack([d, l], axis=1)
    s_dev, M_dev = V.path_score(path, u, logK0, logA, lp0)
    s_ref, M_ref = V.path_score(ref_path, u, logK0, logA, lp0)
    assert abs(s_ref - ref_score) <= 1e-9 * abs(ref_score)
    B = 16.0 * T * 2.0 ** -24 * max(M_dev, M_ref)
    diff = float(np.mean(np.any(path != ref_path, axis=1)))
    lj = float(res['log_joint_map'])
    print(f"T={T} L={L} score_ref={s_ref:.6f} gap={s_ref - s_dev:.3e} B={B:.3e} differ={diff:.4%} "
          f"lj-score={lj - s_dev:.3e} logZ-lj={logz - lj:.3e} jump_frac={np.mean(ref_path[:, 0]):.3f}")
    assert np.isfinite(s_dev)
    assert s_ref - s_dev <= B
    # (c)
    assert diff <= 0.005
    # (d)
    assert abs(lj - s_dev) <= B
    assert lj <= logz + 1e-6 * abs(logz)
    return path


CASES = {
    'j1': dict(shape=(24, 64, 400)),
    'j1_masked': dict(shape=(24, 64, 400), mask=True),
    'j2_pad': dict(shape=(30, 100, 1000)),
    'j2_scale': dict(shape=(30, 100, 1000), scale=0.5),
    'j2_jumpy': dict(shape=(30, 100, 1000), p=(0.2, 0.3)),
    'halo': dict(shape=(40, 96, 1500), mv=3.0),
    'j4': dict(shape=(64, 256, 1200)),
    'j4_scale': dict(shape=(64, 256, 1200), scale=2.0),
    'j4_unaligned': dict(shape=(20, 150, 300)),      # L % 4 != 0 at J = 4: the scalar row loads
    'j8': dict(shape=(48, 512, 600), mv=2.0),
    'j16': dict(shape=(32, 1024, 300)),
    't1': dict(shape=(24, 64, 1)),
    't2': dict(shape=(24, 64, 2)),
    't65': dict(shape=(24, 64, 65)),
    't1037': dict(shape=(24, 64, 1037)),
}


def _run_case(c):
    N, L, T = c['shape']
    mv, p, scale = c.get('mv', 1.0), c.get('p', (0.01, 0.01)), c.get('scale', 1.0)
    dat = _data(N, L, T, mv)
    ma_latent = None
    if c.get('mask'):
        ma_latent = np.ones(L)
        ma_latent[np.random.default_rng(5).permutation(L)[:L // 3]] = 0
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, movement_variance=mv, p_move_to_jump=p[0], p_jump_to_move=p[1])
    kw = dict(tuning=dat['tuning'], ma_latent=ma_latent, likelihood_scale=scale)
    res = m.decode_latent_viterbi(dat['y'], **kw)
    logz = m.decode_marginals(dat['y'], **kw)['log_marginal_final']
    u = scale * O.loglikelihood_poisson_all(dat['y'], dat['tuning'], ma_latent=ma_latent)
    tr = banded_transition(L, mv, p[0], p[1])
    return res, u, tr, logz, ma_latent


@pytest.mark.parametrize("name", list(CASES))
def test_map_path_matches_reference(name):
    res, u, tr, logz, ma_latent = _run_case(CASES[name])
    assert isinstance(res['log_joint_map'], float)
    _check(res, u, tr, logz, ma_latent)


def test_latent_only_model():
    """PoissonGPLVM1D: A = [[1, 0], [1, 0]] (-inf logA), no map_dynamics."""
    N, L, T = 30, 100, 1000
    dat = _data(N, L, T)
    m = PoissonGPLVM1D(N, n_latent_bin=L)
    res = m.decode_latent_viterbi(dat['y'], tuning=dat['tuning'])
    logz = m.decode_marginals(dat['y'], tuning=dat['tuning'])['log_marginal_final']
    u = O.loglikelihood_poisson_all(dat['y'], dat['tuning'])
    path = _check(res, u, banded_transition(L, 1.0, 0.0, 1.0), logz, latent_only=True)
    assert np.all(path[:, 0] == 0)


def test_gaussian_model():
    N, L, T = 24, 64, 400
    dat = _data(N, L, T)
    m = GaussianGPLVMJump1D(N, noise_std=0.5, n_latent_bin=L)
    res = m.decode_latent_viterbi(dat['y'], tuning=dat['tuning'])
    logz = m.decode_marginals(dat['y'], tuning=dat['tuning'])['log_marginal_final']
    u = O.loglikelihood_gaussian_all(dat['y'], dat['tuning'], 0.5)
    _check(res, u, banded_transition(L, 1.0), logz)


def test_batched_sequences_equal_single_calls_bit_for_bit():
    N, L, T = 24, 64, 400
    ds = [_data(N, L, T, seed=s) for s in (0, 10, 20)]
    tun = ds[0]['tuning']
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    ys = np.stack([d['y'] for d in ds])
    rb = m.decode_latent_viterbi(ys, tuning=tun)
    assert rb['map_dynamics'].shape == (3, T) and rb['map_latent'].shape == (3, T)
    assert rb['log_joint_map'].shape == (3,) and rb['log_joint_map'].dtype == np.float64
    for r in range(3):
        one = m.decode_latent_viterbi(ds[r]['y'], tuning=tun)
        assert np.array_equal(one['map_dynamics'], rb['map_dynamics'][r])
        assert np.array_equal(one['map_latent'], rb['map_latent'][r])
        assert one['log_joint_map'] == rb['log_joint_map'][r]
    assert len({float(x) for x in rb['log_joint_map']}) == 3


def test_short_stacked_sequences_at_unaligned_L():
    """R = 3 sequences of T = 5 rows at L = 65 (J = 2, two of 128 padded latents used, the
    scalar row loads; T is no multiple of the ring depth): chain r of the equal-length table
    starts at row r T, and each equals its own single call bit for bit."""
    N, L, T = 12, 65, 5
    ds = [_data(N, L, T, seed=s) for s in (1, 11, 21)]
    tun = ds[0]['tuning']
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    rb = m.decode_latent_viterbi(np.stack([d['y'] for d in ds]), tuning=tun)
    assert rb['map_latent'].shape == (3, T) and rb['log_joint_map'].shape == (3,)
    for r in range(3):
        one = m.decode_latent_viterbi(ds[r]['y'], tuning=tun)
        assert np.array_equal(one['map_dynamics'], rb['map_dynamics'][r])
        assert np.array_equal(one['map_latent'], rb['map_latent'][r])
        assert one['log_joint_map'] == rb['log_joint_map'][r]
        assert np.isfinite(one['log_joint_map'])
    assert len({float(x) for x in rb['log_joint_map']}) == 3


def test_deterministic():
    res1 = _run_case(CASES['j2_jumpy'])[0]
    res2 = _run_case(CASES['j2_jumpy'])[0]
    assert np.array_equal(res1['map_dynamics'], res2['map_dynamics'])
    assert np.array_equal(res1['map_latent'], res2['map_latent'])
    assert res1['log_joint_map'] == res2['log_joint_map']
