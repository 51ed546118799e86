"""Host-side checks of decode_latent_segments(exact=True) / pmg_dense_segment_smoother (no GPU):
the entry point's export, binding and argument refusals, the public host refusals, and the
input condition of the GPU comparison (tests/test_gpu_dense_segments.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from poor_man_gplvm_amd import (GaussianGPLVM1D, GaussianGPLVMJump1D, PoissonGPLVM1D, PoissonGPLVMJump1D, _native)
from tests import dense_segments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pmg_dense_segment_smoother"


# ----------------------------------------------------------------------------- entry point
def test_entry_point_is_exported_declared_and_bound():
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, ENTRY)
    txt = open(os.path.join(ROOT, 'include', 'pmg.h')).read()
    assert re.search(r'#define\s+PMG_ABI_VERSION\s+4\b', txt)
    decl = re.search(r'\bint\s+' + ENTRY + r'\s*\((.*?)\)\s*;', re.sub(r'/\*.*?\*/', '', txt, flags=re.S), flags=re.S)
    assert decl, "not declared in include/pmg.h"
    args = [a.strip() for a in decl.group(1).split(',')]
    names = [re.split(r'[\s*]+', a)[-1] for a in args]
    assert names == ['delta', 'phi', 'll64', 'm', 'T', 'seg_off', 'S', 'order', 'tr', 'likelihood_scale', 'alpha',
                     'log_alpha', 'gamma', 'log_gamma', 'P', 'logc', 'logz', 'stream']
    assert ENTRY in _native.EXPORTED_SYMBOLS
    argt, rest = _native._SIGS[ENTRY]
    assert rest is ctypes.c_int32 and len(argt) == len(args)
    for a, t in zip(args, argt):                # header and binding agree, argument by argument
        want = (ctypes.c_int64 if a.startswith('int64_t ') else ctypes.c_int32 if a.startswith('int32_t ')
                else ctypes.c_double if a.startswith('double ') else None)
        if 'pmg_dense_transition' in a:
            assert t is ctypes.POINTER(_native.DenseTransition), a
        elif want is not None:
            assert t is want, a
        else:
            assert '*' in a and t is ctypes.c_void_p, a


def test_entry_point_argument_checks():
    """Every refusal precedes any HIP call (the pointers are never dereferenced; no device)."""
    lib = _native.load()
    tr = _native.DenseTransition()
    one = ctypes.c_void_p(256)
    tr.L = 64
    tr.logK = tr.logKT = tr.logK_lo = tr.logKT_lo = 256

    def call(**kw):
        a = dict(delta=one, phi=one, ll64=None, m=one, T=10, seg_off=one, S=2, order=None, tr=ctypes.byref(tr),
                 s=1.0, alpha=None, log_alpha=one, gamma=one, log_gamma=one, P=one, logc=one, logz=one)
        a.update(kw)
        rc = lib.pmg_dense_segment_smoother(a['delta'], a['phi'], a['ll64'], a['m'], a['T'], a['seg_off'], a['S'],
                                            a['order'], a['tr'], a['s'], a['alpha'], a['log_alpha'], a['gamma'],
                                            a['log_gamma'], a['P'], a['logc'], a['logz'], None)
        return rc, lib.pmg_last_error()

    rc, msg = call(T=0)
    assert rc == -1 and b'T=0' in msg
    rc, msg = call(T=-3)
    assert rc == -1 and b'T=-3' in msg
    rc, msg = call(S=-1)
    assert rc == -1 and b'S=-1' in msg
    for name in ('delta', 'phi', 'm', 'seg_off', 'log_alpha', 'logc', 'logz'):
        rc, msg = call(**{name: None})
        assert rc == -1 and (b' ' + name.encode() + b' is null') in msg, (name, msg)
    rc, msg = call(tr=None)
    assert rc == -1 and b'transition' in msg
    for field in ('logK', 'logKT', 'logK_lo', 'logKT_lo'):
        setattr(tr, field, None)
        rc, msg = call()
        assert rc == -1 and b'transition' in msg, field
        setattr(tr, field, 256)
    tr.L = 0
    rc, msg = call()
    assert rc == -1 and b'transition' in msg
    tr.L = 4097
    rc, msg = call()
    assert rc == -3 and b'4096' in msg
    rc, msg = call(S=0)                         # refusals come before the empty call's PMG_OK
    assert rc == -3
    tr.L = 4096
    assert call(S=0)[0] == 0                    # no segments: PMG_OK with no launch (no device here)
    assert call(S=0, alpha=None, gamma=None, log_gamma=None, P=None, ll64=None, order=None)[0] == 0
    rc, msg = call(S=0, logz=None)
    assert rc == -1 and b' logz is null' in msg


# ----------------------------------------------------------------------------- public refusals
def test_exact_refusals_before_any_device_work():
    rng = np.random.default_rng(0)
    N, L, T = 5, 16, 20
    y = rng.poisson(1.0, size=(T, N)).astype(np.float32)
    tun = rng.random((L, N)) + 0.1
    seg = [[0, 5], [8, 20]]
    K = R.custom_kernel(L)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, custom_transition_kernel=K)
    for bad in ([[5, 5]], [[0, T + 1]], [[-2, 3]], [[0, 3, 4]]):
        with pytest.raises(ValueError):
            m.decode_latent_segments(y, bad, tuning=tun, exact=True)
    with pytest.raises(ValueError, match="1-D ma_neuron"):
        m.decode_latent_segments([y[:5], y[5:]], tuning=tun, ma_neuron=np.ones((T, N)), exact=True)
    for cls in (PoissonGPLVMJump1D, GaussianGPLVMJump1D, PoissonGPLVM1D, GaussianGPLVM1D):
        small = cls(N, n_latent_bin=L)
        for bad in (1, 0, None, "yes", 1.0):
            with pytest.raises(TypeError, match="exact"):
                small.decode_latent_segments(y, seg, tuning=tun, exact=bad)
    for cls in (PoissonGPLVMJump1D, GaussianGPLVM1D):
        big = cls(N, n_latent_bin=L)
        big.n_latent_bin = 4097                 # the refusal reads the count alone (a 4097-bin basis takes 10 s)
        with pytest.raises(NotImplementedError, match="4096"):
            big.decode_latent_segments(y, seg, tuning=tun, exact=True)
    # the default path keeps its refusals
    with pytest.raises(NotImplementedError, match="decode_latent_segments.*custom_transition_kernel"):
        m.decode_latent_segments(y, seg, tuning=tun)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        m.decode_latent_segments(y, seg, tuning=tun, exact=False)


def test_latent_only_default_names_exact():
    rng = np.random.default_rng(0)
    y = rng.poisson(1.0, size=(20, 5)).astype(np.float32)
    for cls in (PoissonGPLVM1D, GaussianGPLVM1D):
        with pytest.raises(NotImplementedError, match=r"latent-only.*exact=True"):
            cls(5, n_latent_bin=16).decode_latent_segments(y, [[0, 5]], tuning=rng.random((16, 5)) + 0.1)


def test_banded_engine_refuses_the_dense_segment_smoother():
    """DeviceEM.segment_smoother_dense mirrors _need_banded (checked on the method's guard:
    an engine needs a device)."""
    from poor_man_gplvm_amd.engine import DeviceEM

    eng = DeviceEM.__new__(DeviceEM)            # no transition set: not dense (EngineBase.dense)
    with pytest.raises(NotImplementedError, match="segment_smoother_dense needs a dense transition"):
        eng.segment_smoother_dense(1.0, None)


def test_segment_dense_max_default_is_a_power_of_two():
    from poor_man_gplvm_amd.engine import ScanConfig
    w = ScanConfig().segment_dense_max
    assert 16 <= w <= ScanConfig().segment_wave_max and w & (w - 1) == 0


# ----------------------------------------------------------------------------- the comparison's inputs
def test_kernel_is_asymmetric():
    K = R.custom_kernel(61)
    assert np.abs(K - K.T).max() > 0.3


def test_reference_is_decode_latent_per_segment():
    """The shared reference (the oracle's smoother without the pairwise joint) equals
    oracle.decode_latent(y[a:b], tuning, custom_kernel=K) on every segment, bit for bit."""
    from oracle import gplvm_oracle as O
    L = 61
    d, K, off = R.inputs(L)
    ref = R.reference(L)
    for s, (a, b) in enumerate(zip(off[:-1], off[1:])):
        r = O.decode_latent(d['y'][a:b], d['tuning'], custom_kernel=K)
        assert np.array_equal(ref['gamma'][a:b], r['posterior_all'])
        assert np.array_equal(ref['log_gamma'][a:b], r['log_posterior_all'])
        assert np.array_equal(ref['logc'][a:b], r['log_one_step_predictive_marginals_all'])
        assert ref['logz'][s] == r['log_marginal_final']
    assert np.all(np.abs(ref['gamma'].sum((1, 2)) - 1) < 1e-12) and np.all(np.abs(ref['alpha'].sum((1, 2)) - 1) < 1e-12)


@pytest.mark.parametrize("L", sorted(set(R.FULL_L + R.BITWISE_L)))
def test_wrong_implementations_move_every_event(L):
    """A scan that reads the kernel transposed, and one chain run across the event
    boundaries, each move the posterior of every one of the 14 events by >= 1e-4, 10x the
    1e-5 bar of the GPU comparison.  Measured with these inputs: transposed 3.4e-4 .. 9.9e-2,
    concatenated 7.5e-3 .. 2.8e-1 over L = 2 .. 300.
    L = 1 cannot tell either apart, whatever the data: a 1 x 1 kernel is its own transpose,
    and with one latent both dynamics states see the same emission, so the uniform state is
    stationary and every posterior of every chain is (1/2, 1/2).  There the two must agree
    with the reference instead (the GPU test at L = 1 checks the thread line's guards)."""
    d, K, off = R.inputs(L)
    ref = R.reference(L)['gamma']
    assert len(off) - 1 == 14 and int(off[-1]) == 120
    tr = R.per_event_max(R.transposed_posterior(L) - ref, off)
    cc = R.per_event_max(R.concatenated_posterior(L) - ref, off)
    print(f"L={L}: transposed {tr.min():.2e} .. {tr.max():.2e}, concatenated {cc.min():.2e} .. {cc.max():.2e}")
    if L == 1:
        assert tr.max() < 1e-12 and cc.max() < 1e-12
        return
    assert tr.min() >= 1e-4, tr
    assert cc.min() >= 1e-4, cc
