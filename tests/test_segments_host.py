"""Host-side checks of decode_latent_segments / pmg_segment_smoother (no GPU).

Input conditions of the GPU cases in tests/test_gpu_segments.py, on the float64 reference:
a scan that lost its outermost tap, or a filter that ran straight across the gaps
between segments, would miss the parity bar 1e-5 |ref| + 1e-12 by a factor >= 100 in every
segment of every case.  Then the interval handling (validation, gathering, offsets, the
longest-first order, list input), the errors raised before any device work, and the entry
point's argument checks.
"""
import ctypes

import numpy as np
import pytest

from poor_man_gplvm_amd import _native
from poor_man_gplvm_amd import core as C
from poor_man_gplvm_amd.core import (GaussianGPLVM1D, GaussianGPLVMJump1D, PoissonGPLVM1D, PoissonGPLVMJump1D,
                                     gather_segments, segment_order)
from poor_man_gplvm_amd.engine import ScanConfig
from tests import segments_ref as R


def _ratio(x, ref):
    return np.abs(x - ref) / (1e-5 * np.abs(ref) + 1e-12)


def _case_id(run):
    return f"L{run['L']}-band{run['band']}"


# ----------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("run", [r for J, WP in R.SEG_PAIRS for r in R.seg_runs(J, WP).values()], ids=_case_id)
def test_inputs_separate_a_lost_tap_and_a_crossed_boundary(run):
    _, tr, off, (gamma, logz, alpha, logc) = R.segment_reference(run['L'], run['band'], R.LENS, run['seed'])
    assert tr.band == run['band'] and off[-1] == 120
    lost = R.lost_tap_reference(run['L'], run['band'], R.LENS, run['seed'])[0]
    cat = R.concatenated_reference(run['L'], run['band'], R.LENS, run['seed'])[0]
    worst_lost, worst_cat = np.inf, np.inf
    for s in range(len(R.LENS)):
        a, b = off[s], off[s + 1]
        worst_lost = min(worst_lost, _ratio(lost[a:b], gamma[a:b]).max())
        worst_cat = min(worst_cat, _ratio(cat[a:b], gamma[a:b]).max())
    print(f"{_case_id(run)}: lost tap >= {worst_lost:.3g} x bar, crossed boundary >= {worst_cat:.3g} x bar")
    assert worst_lost >= 100 and worst_cat >= 100
    # each segment is a normalised posterior of its own
    np.testing.assert_allclose(gamma.sum((1, 2)), 1.0, rtol=1e-12)
    for s in range(len(R.LENS)):
        np.testing.assert_allclose(logz[s], logc[off[s]:off[s + 1]].sum(), rtol=1e-13)


def test_lens_cover_the_ring_depths():
    lens = set(R.LENS)
    assert sum(R.LENS) == 120 and R.LENS[0] == 1
    for pf in R.RING_DEPTHS:
        assert {pf - 1, pf, pf + 1} <= lens
    assert max(lens) > 2 * max(R.RING_DEPTHS) + 1 and 2 * max(R.RING_DEPTHS) + 1 in lens
    k = R.LENS.index(max(R.LENS))
    assert min(R.LENS[k + 1:]) == 1                 # short segments after the longest


# ----------------------------------------------------------------------------- intervals
def test_gather_rows_offsets_and_order():
    rng = np.random.default_rng(0)
    T, N = 50, 4
    y = rng.poisson(1.0, size=(T, N)).astype(np.float64)
    seg = np.array([[40, 50], [3, 4], [10, 25], [0, 3], [12, 14]])       # unsorted, overlapping, one ends at T
    yc, off, ma = gather_segments(y, seg, np.ones(N))
    assert yc.dtype == np.float32 and yc.flags.c_contiguous and off.dtype == np.int64
    np.testing.assert_array_equal(off, [0, 10, 11, 26, 29, 31])
    for s, (a, b) in enumerate(seg):
        np.testing.assert_array_equal(yc[off[s]:off[s + 1]], y[a:b])
    assert ma.shape == (N,)
    order = segment_order(off)
    assert order.dtype == np.int32
    np.testing.assert_array_equal(order, [2, 0, 3, 4, 1])               # longest first, ties in index order
    np.testing.assert_array_equal(segment_order(np.array([0, 2, 4, 6])), [0, 1, 2])
    # a per-time mask follows its rows
    m2 = (rng.random((T, N)) > 0.3).astype(np.float32)
    _, _, mg = gather_segments(y, seg, m2)
    for s, (a, b) in enumerate(seg):
        np.testing.assert_array_equal(mg[off[s]:off[s + 1]], m2[a:b])
    # list input: the same compact layout
    yl, offl, _ = gather_segments([y[a:b] for a, b in seg], None, np.ones(N))
    np.testing.assert_array_equal(yl, yc)
    np.testing.assert_array_equal(offl, off)
    # integral floats are accepted as row indices
    np.testing.assert_array_equal(gather_segments(y, seg.astype(np.float64))[1], off)


@pytest.mark.parametrize("seg", [[[5, 5]], [[7, 3]], [[-1, 4]], [[0, 51]], [[50, 51]], [[0, 3, 5]], [0, 3], [],
                                 [[0.5, 3]]])
def test_bad_intervals(seg):
    y = np.zeros((50, 3), np.float32)
    with pytest.raises(ValueError):
        gather_segments(y, np.asarray(seg))


def test_bad_list_input():
    y = np.zeros((6, 3), np.float32)
    with pytest.raises(ValueError):
        gather_segments(y, None)                        # an array without intervals
    with pytest.raises(ValueError):
        gather_segments([], None)
    with pytest.raises(ValueError):
        gather_segments([y, np.zeros((0, 3))], None)    # an empty segment
    with pytest.raises(ValueError):
        gather_segments([y, np.zeros((4, 2))], None)    # another neuron count
    with pytest.raises(ValueError, match="1-D ma_neuron"):
        gather_segments([y, y], None, np.ones((12, 3)))
    with pytest.raises(ValueError, match="2-D ma_neuron"):
        gather_segments(y, [[0, 3]], np.ones((5, 3)))


def test_true_runs():
    assert C._true_runs([True, True, False, True, False, False, True]) == [(0, 2), (3, 4), (6, 7)]
    assert C._true_runs([False, False]) == [] and C._true_runs([True]) == [(0, 1)]


# ----------------------------------------------------------------------------- errors without a device
def test_errors_before_any_device_work():
    rng = np.random.default_rng(0)
    N, L, T = 5, 16, 20
    y = rng.poisson(1.0, size=(T, N)).astype(np.float32)
    tun = rng.random((L, N)) + 0.1
    seg = [[0, 5], [8, 20]]
    K = np.exp(-np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]) / 3.0)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, custom_transition_kernel=K)
    with pytest.raises(NotImplementedError, match="decode_latent_segments.*custom_transition_kernel"):
        m.decode_latent_segments(y, seg, tuning=tun)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        m.decode_latent_segments(y, seg)            # the model's own tuning would need the device: never reached
    m = PoissonGPLVMJump1D(N, n_latent_bin=64)
    with pytest.raises(NotImplementedError, match="band"):
        m.decode_latent_segments(y, seg, tuning=rng.random((64, N)) + 0.1, hyperparam={'movement_variance': 6.0})
    g = GaussianGPLVMJump1D(N, n_latent_bin=L, custom_transition_kernel=K)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        g.decode_latent_segments(y, seg, tuning=tun)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    for bad in ([[5, 5]], [[0, T + 1]], [[-2, 3]], [[0, 3, 4]]):
        with pytest.raises(ValueError):
            m.decode_latent_segments(y, bad)
    with pytest.raises(ValueError, match="1-D ma_neuron"):
        m.decode_latent_segments([y[:5], y[5:]], ma_neuron=np.ones((T, N)))
    for cls in (PoissonGPLVM1D, GaussianGPLVM1D):
        with pytest.raises(NotImplementedError, match="latent-only"):
            cls(N, n_latent_bin=L).decode_latent_segments(y, seg, tuning=tun)


def test_segment_wave_max_default_is_a_power_of_two():
    w = ScanConfig().segment_wave_max
    assert w >= 256 and w & (w - 1) == 0


# ----------------------------------------------------------------------------- entry point
def test_entry_point_argument_checks():
    """Every check precedes any HIP call (the pointers are never dereferenced)."""
    lib = _native.load()
    tr = _native.Transition()
    tr.L, tr.band = 64, 9
    tr.invz = 256
    one = ctypes.c_void_p(256)

    def call(**kw):
        a = dict(delta=one, phi=one, m=one, T=10, seg_off=one, S=2, order=None, tr=ctypes.byref(tr), s=1.0,
                 alpha=one, gamma=one, P=one, logc=one, logz=one)
        a.update(kw)
        rc = lib.pmg_segment_smoother(a['delta'], a['phi'], a['m'], a['T'], a['seg_off'], a['S'], a['order'], a['tr'],
                                      a['s'], a['alpha'], a['gamma'], a['P'], a['logc'], a['logz'], None)
        return rc, lib.pmg_last_error()

    rc, msg = call(T=0)
    assert rc == -1 and b'T=0' in msg
    rc, msg = call(S=0)
    assert rc == -1 and b'S=0' in msg
    for name in ('delta', 'phi', 'm', 'seg_off', 'alpha', 'logc', 'logz'):
        rc, msg = call(**{name: None})
        assert rc == -1 and (b' ' + name.encode() + b' is null') in msg, (name, msg)
    rc, msg = call(tr=None)
    assert rc == -1 and b'tr is null' in msg
    rc, msg = call(s=float('nan'))
    assert rc == -1 and b'likelihood_scale' in msg
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
