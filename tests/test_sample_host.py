"""Host-side checks of sample_latent_segments / pmg_segment_sample (no GPU).

Input conditions of the GPU cases in tests/test_gpu_sample.py, on the float64 reference
sampler of tests/sample_ref.py with alpha rounded to float32, the ragged batch
tests/segments_ref.LENS and u = default_rng(7).random((256, 120), float32):
  1. the reference passes the teacher-forced check with 0 violations;
  2. the steps where u total lies within eps total of a CDF edge -- the only ones where float32
     rounding may move a draw, i.e. where the check's allowance is in play -- are <= 2 % of
     all steps (found: at most 0.77 % at L = 1000, band 30; <= 0.4 % for L <= 500);
  3. the check separates wrong samplers: one that loses its outermost tap violates >= 0.3 %
     of the steps wherever band >= 1 (found: 0.43 % at (33, 32), 2.3 % at (8, 7), 7.6-29 %
     elsewhere), one with a transposed A >= 2 % (found: 2.4-61 %);
  4. the statistical bar: the reference's own z against the smoothed posterior is <= 4.0 in
     every row of every case (found: max 3.78 at (1024, 32), <= 3.5 elsewhere), so the GPU
     test's z <= 5 is not met by luck.
Then the errors the model methods raise before any device work, the entry point's argument
checks, the new name in the header, the binding and the library, and the host-side raising
of a set status word (through the engine's own helper: the kernel's total == 0 path is not
provoked on a GPU).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from poor_man_gplvm_amd import _native
from poor_man_gplvm_amd import engine as E
from poor_man_gplvm_amd.core import (GaussianGPLVM1D, GaussianGPLVMJump1D, PoissonGPLVM1D, PoissonGPLVMJump1D,
                                     _checked_uniforms)
from tests import sample_ref as SR
from tests import scan_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(case):
    return f"L{case[0]}-band{case[1]}"


# ----------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("case", SR.CASES, ids=_id)
def test_reference_passes_and_wrong_samplers_do_not(case):
    L, band = case
    _, tr, off, alpha, gamma, (pd, pl) = SR.sample_reference(L, band)
    u = SR.uniforms()
    assert u.shape == (256, 120) and u.dtype == np.float32 and off[-1] == 120 and tr.band == band
    assert u.min() >= 0 and u.max() < 1
    rep = SR.step_report(alpha, tr, off, u, pd, pl)
    n = int(rep['owned'].sum())
    assert n == 256 * 120 and pd.min() >= 0 and pl.min() >= 0
    # 1. the reference itself
    assert SR.check_paths(alpha, tr, off, u, pd, pl) == 0
    # 2. rounding can matter at few steps only
    near = rep['near_edge'].sum() / n
    # 3. wrong samplers
    lost = None
    if band >= 1:
        bd, bl = SR.ffbs(alpha, tr, off, u, K0=S.dense_K(tr, drop_outer_tap=True)[0])
        lost = SR.check_paths(alpha, tr, off, u, bd, bl) / n
    bd, bl = SR.ffbs(alpha, tr, off, u, A=S.device_A(tr).T)
    transposed = SR.check_paths(alpha, tr, off, u, bd, bl) / n
    # 4. the statistical bar on the reference's own paths
    z_d, z_l = SR.z_scores(pd, pl, gamma)
    print(f"{_id(case)}: near an edge {near:.3%}, lost tap {lost if lost is None else format(lost, '.3%')}, "
          f"transposed A {transposed:.3%}, z_d {z_d.max():.2f}, z_l {z_l.max():.2f}")
    assert near <= 0.02
    assert lost is None or lost >= 0.003
    assert transposed >= 0.02
    assert max(z_d.max(), z_l.max()) <= 4.0


def test_weights_match_the_dense_joint_factorisation():
    """weights() against the definition p(x_t | x_{t+1}) ~ alpha_t[x_t] Trans[x_t, x_{t+1}] with the
    dense kernels of scan_ref (the jump kernel's 1 / L included: it cancels)."""
    L, band = 33, 5
    tr = S.flat_transition(L, band)
    K, A = S.dense_K(tr), S.device_A(tr)
    alpha_t = np.random.default_rng(0).random((2, L))
    for dn, ln in ((0, 0), (0, 17), (0, L - 1), (1, 4)):
        full = alpha_t * A[:, dn][:, None] * K[dn][:, ln][None, :]
        w = SR.weights(alpha_t, K[0], A, dn, ln)
        np.testing.assert_allclose(w / w.sum(), full.reshape(-1) / full.sum(), rtol=1e-13)
        if dn == 0:
            far = np.abs(np.arange(L) - ln) > band
            assert np.all(w.reshape(2, L)[:, far] == 0) and np.all(w.reshape(2, L)[:, ~far] > 0)
    np.testing.assert_array_equal(SR.weights(alpha_t, K[0], A, -1, 0), alpha_t.reshape(-1))


def test_check_paths_judges_every_step():
    """One flipped state is one or two violations (its own step and the step conditioned on
    it), a -1 is a violation, and rows that no segment owns are not judged."""
    L, band = 61, 3
    _, tr, off, alpha, _, (pd, pl) = SR.sample_reference(L, band)
    u = SR.uniforms()
    bd, bl = pd.copy(), pl.copy()
    t = int(off[10]) + 5                                  # inside the 33-row segment
    bl[3, t] = (bl[3, t] + 30) % L                        # far beyond the band of either neighbour
    assert 1 <= SR.check_paths(alpha, tr, off, u, bd, bl) <= 2
    bd, bl = pd.copy(), pl.copy()
    bd[7, t] = -1
    assert 1 <= SR.check_paths(alpha, tr, off, u, bd, bl) <= 2
    # a gap: rows [3, 6) unowned
    off2 = np.array([0, 3, 3], np.int64)
    off3 = np.array([0, 3], np.int64)
    qd, ql = SR.ffbs(alpha, tr, off3, u)
    assert np.all(qd[:, 3:] == -1) and np.all(ql[:, 3:] == -1)
    assert SR.check_paths(alpha, tr, off2, u, qd, ql) == 0


def test_eps_is_twice_the_rounding_count():
    assert SR.ROUNDINGS == 32 and SR.EPS == 64 * 2.0 ** -24


# ----------------------------------------------------------------------------- errors without a device
def test_errors_before_any_device_work():
    rng = np.random.default_rng(0)
    N, L, T = 5, 16, 20
    y = rng.poisson(1.0, size=(T, N)).astype(np.float32)
    tun = rng.random((L, N)) + 0.1
    seg = [[0, 5], [8, 20]]
    Ttot = 17
    K = np.exp(-np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]) / 3.0)
    # dense kernel
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, custom_transition_kernel=K)
    with pytest.raises(NotImplementedError, match="sample_latent_segments.*custom_transition_kernel"):
        m.sample_latent_segments(y, seg, tuning=tun)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        m.sample_latent_posterior(y, tuning=tun)
    g = GaussianGPLVMJump1D(N, n_latent_bin=L, custom_transition_kernel=K)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        g.sample_latent_segments(y, seg, tuning=tun)
    # band > 32
    m = PoissonGPLVMJump1D(N, n_latent_bin=64)
    with pytest.raises(NotImplementedError, match="band"):
        m.sample_latent_segments(y, seg, tuning=rng.random((64, N)) + 0.1, hyperparam={'movement_variance': 6.0})
    # latent-only models
    for cls in (PoissonGPLVM1D, GaussianGPLVM1D):
        with pytest.raises(NotImplementedError, match="latent-only"):
            cls(N, n_latent_bin=L).sample_latent_segments(y, seg, tuning=tun)
        with pytest.raises(NotImplementedError, match="latent-only"):
            cls(N, n_latent_bin=L).sample_latent_posterior(y, tuning=tun)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    # n_samples
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_samples"):
            m.sample_latent_segments(y, seg, n_samples=bad, tuning=tun)
    with pytest.raises(ValueError, match="n_samples"):
        m.sample_latent_posterior(y, n_samples=0, tuning=tun)
    # intervals
    for bad in ([[5, 5]], [[0, T + 1]], [[-2, 3]], [[0, 3, 4]]):
        with pytest.raises(ValueError):
            m.sample_latent_segments(y, bad, tuning=tun)
    with pytest.raises(ValueError, match="1-D ma_neuron"):
        m.sample_latent_segments([y[:5], y[5:]], ma_neuron=np.ones((T, N)), tuning=tun)
    # uniforms: shape, then range
    ok = rng.random((4, Ttot), np.float32)
    for bad in (ok[:3], ok[:, :-1], ok.T, ok[0], np.zeros((4, Ttot), np.int32)):
        with pytest.raises(ValueError, match="uniforms"):
            m.sample_latent_segments(y, seg, n_samples=4, uniforms=bad, tuning=tun)
    for v in (1.0, -1e-9, np.nan, 1.0 - 1e-12):           # the last one rounds to 1 in float32
        bad = ok.astype(np.float64)
        bad[2, 5] = v
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            m.sample_latent_segments(y, seg, n_samples=4, uniforms=bad, tuning=tun)
    with pytest.raises(ValueError, match="uniforms"):
        m.sample_latent_posterior(y, n_samples=4, uniforms=ok, tuning=tun)      # (4, 17), not (4, 20)


def test_checked_uniforms_accepts_arrays_and_tensors():
    import torch
    u = np.random.default_rng(1).random((3, 7))
    a = _checked_uniforms(u, 3, 7)
    assert a.dtype == torch.float32 and tuple(a.shape) == (3, 7)
    np.testing.assert_array_equal(a.numpy(), u.astype(np.float32))
    b = _checked_uniforms(torch.as_tensor(u.astype(np.float32)), 3, 7)
    assert torch.equal(a, b)
    assert float(_checked_uniforms(np.zeros((1, 1), np.float32), 1, 1)[0, 0]) == 0.0


def test_status_word_raises():
    """The host side of the kernel's total == 0 path, on host values: the engine's helper is what
    segment_sampler calls on the status word it read back."""
    E.sample_status_check(0)
    with pytest.raises(_native.NativeError, match="pmg_segment_sample.*summed to 0"):
        E.sample_status_check(1)


# ----------------------------------------------------------------------------- entry point
def test_header_binding_and_library_agree_on_the_new_name():
    txt = open(os.path.join(ROOT, 'include', 'pmg.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pmg_[a-z0-9_]+)\s*\(', txt))
    lib = ctypes.CDLL(_native.LIB_PATH)
    name = 'pmg_segment_sample'
    assert name in declared and name in _native.EXPORTED_SYMBOLS and name in _native._SIGS and hasattr(lib, name)
    assert len(_native._SIGS[name][0]) == 12
    assert os.path.exists(os.path.join(ROOT, 'poor_man_gplvm_amd', 'csrc', 'segment_sample.hip'))


def test_entry_point_argument_checks():
    """Every check precedes any HIP call (the pointers are never dereferenced)."""
    lib = _native.load()
    tr = _native.Transition()
    tr.L, tr.band = 64, 9
    tr.invz = 256
    one = ctypes.c_void_p(256)

    def call(**kw):
        a = dict(alpha=one, T=10, seg_off=one, S=2, order=None, tr=ctypes.byref(tr), uniforms=one, R=3,
                 path_d=one, path_l=one, status=one)
        a.update(kw)
        rc = lib.pmg_segment_sample(a['alpha'], a['T'], a['seg_off'], a['S'], a['order'], a['tr'], a['uniforms'],
                                    a['R'], a['path_d'], a['path_l'], a['status'], None)
        return rc, lib.pmg_last_error()

    rc, msg = call(T=0)
    assert rc == -1 and b'T=0' in msg
    rc, msg = call(S=0)
    assert rc == -1 and b'S=0' in msg
    rc, msg = call(R=0)
    assert rc == -1 and b'R=0' in msg
    rc, msg = call(S=1 << 20, R=1 << 20)
    assert rc == -1 and b'exceed' in msg
    for name in ('alpha', 'seg_off', 'uniforms', 'path_d', 'path_l', 'status'):
        rc, msg = call(**{name: None})
        assert rc == -1 and (b' ' + name.encode() + b' is null') in msg, (name, msg)
    rc, msg = call(tr=None)
    assert rc == -1 and b'tr is null' in msg
    tr.band = 40
    rc, msg = call()
    assert rc == -1 and b'band' in msg
    tr.band = 9
    tr.L = 1025
    rc, msg = call()
    assert rc == -3 and b'1024' in msg
    tr.L = 64
    tr.invz = None
    rc, msg = call()
    assert rc == -1 and b'invz' in msg
