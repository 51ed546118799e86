"""Host-side checks of the per-neuron circular spike shuffle (no GPU):
shuffle_test_segments(shuffle='neuron_circular') / pmg_segment_roll_prepare.

(a) segment_neuron_shifts on a CPU generator and the launch blocking; (b) the host shuffle
roll_segments of tests/neuron_shuffle_ref.py; (c) the errors the model method raises before any
device work and the entry point's argument checks; (d) the input condition of
tests/test_gpu_neuron_shuffle.py: on the float64 reference with its fixed shifts, an
implementation that ignores shift, one that rolls by -k and one that takes neuron n + 1's shift
each move logZ by >= 1e-5 |logZ| -- 100 x the GPU bar of 1e-7 -- in >= 80 % of the eligible
(shuffle, event) pairs of every case with L > 1.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from poor_man_gplvm_amd import _native
from poor_man_gplvm_amd.core import (SHUFFLE_KINDS, GaussianGPLVM1D, GaussianGPLVMJump1D, PoissonGPLVM1D,
                                     PoissonGPLVMJump1D, _checked_neuron_shift, segment_neuron_shifts)
from tests import neuron_shuffle_ref as NS
from tests import sample_ref as SR
from tests import segments_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(case):
    return f"L{case[0]}-band{case[1]}"


# ----------------------------------------------------------------------------- (a) generated shifts
def test_shuffle_kinds_entry():
    assert SHUFFLE_KINDS == ('time_bin', 'column_cycle', 'both', 'neuron_circular')


def test_generated_shifts_range_and_min_shift_rule():
    lens = np.array([1, 2, 9, 10, 11, 12, 40], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    for min_shift in (0, 5):
        sh = segment_neuron_shifts(off, 400, 7, min_shift, torch.Generator().manual_seed(1), 'cpu')
        assert sh.dtype == torch.int32 and tuple(sh.shape) == (400, len(lens), 7)
        s = sh.numpy()
        for k, n in enumerate(lens):
            lo = min_shift if n > 2 * min_shift else 0      # len = 10 = 2 min_shift: the whole range
            hi = n - lo
            assert s[:, k].min() >= lo and s[:, k].max() <= hi - 1, (min_shift, n)
            if hi - lo <= 8:    # 2800 draws over at most 8 values: every value is drawn
                assert set(np.unique(s[:, k])) == set(range(lo, hi)), (min_shift, n)
        assert np.all(s[:, 0] == 0)                          # a one-row event cannot move
    s5 = segment_neuron_shifts(off, 400, 7, 5, torch.Generator().manual_seed(1), 'cpu').numpy()
    assert s5[:, 3].min() == 0 and s5[:, 3].max() == 9       # len 10: lo = 0
    assert s5[:, 4].min() == 5 and s5[:, 4].max() == 5       # len 11: the single value 5
    assert s5[:, 5].min() == 5 and s5[:, 5].max() == 6       # len 12: 5, 6
    # the same generator state gives the same shifts
    again = segment_neuron_shifts(off, 400, 7, 5, torch.Generator().manual_seed(1), 'cpu').numpy()
    assert np.array_equal(s5, again)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="min_shift"):
            segment_neuron_shifts(off, 2, 7, bad)


def test_draws_do_not_depend_on_the_batch_bytes():
    """A launch takes whole generation blocks, each drawn on its own: the sequence of draws of
    a call is the same whatever SHUFFLE_NEURON_BATCH_BYTES."""
    m = PoissonGPLVMJump1D(24, n_latent_bin=64)
    g = m.SHUFFLE_NEURON_GEN_BLOCK
    assert g == 8
    big = m._shuffle_neuron_batch(120, 14, 24, 1000, False)
    assert big % g == 0 and big >= 1000
    assert m._shuffle_neuron_batch(120, 14, 24, 1000, True) % g == 0
    m.SHUFFLE_NEURON_BATCH_BYTES = 1
    assert m._shuffle_neuron_batch(120, 14, 24, 1000, False) == g
    off = R.offsets(R.LENS)

    def draws(nb, n_shuffle=21):
        gen, out = torch.Generator().manual_seed(7), []
        for r0 in range(0, n_shuffle, nb):        # the loop of _shuffle_neuron_circular
            r1 = min(n_shuffle, r0 + nb)
            out += [segment_neuron_shifts(off, min(g, r1 - b0), 24, 2, gen, 'cpu') for b0 in range(r0, r1, g)]
        return torch.cat(out)
    assert torch.equal(draws(g), draws(3 * g)) and draws(g).shape[0] == 21


# ----------------------------------------------------------------------------- (b) the host shuffle
def test_roll_segments_keeps_counts_and_outside_rows():
    rng = np.random.default_rng(2)
    y = rng.poisson(1.5, size=(50, 6)).astype(np.float32)
    off = np.array([3, 4, 9, 9, 30, 47], np.int64)           # rows 0-2 and 47-49 outside, one empty event
    shift = rng.integers(-100, 100, size=(5, 6))
    out = NS.roll_segments(y, off, shift)
    assert out.dtype == y.dtype and out.shape == y.shape
    assert np.array_equal(out[:3], y[:3]) and np.array_equal(out[47:], y[47:])
    for s in range(5):
        a, b = off[s], off[s + 1]
        assert np.array_equal(np.sort(out[a:b], axis=0), np.sort(y[a:b], axis=0)), s
        for n in range(6):
            if b > a:
                assert np.array_equal(out[a:b, n], np.roll(y[a:b, n], shift[s, n])), (s, n)
    # out[t] = in[t - k]; multiples of the length and the int32 extremes
    col = np.arange(7, dtype=np.float32)[:, None]
    o1 = np.array([0, 7], np.int64)
    assert NS.roll_segments(col, o1, [[2]])[:, 0].tolist() == [5, 6, 0, 1, 2, 3, 4]
    for k in (0, 7, -7, 70):
        assert np.array_equal(NS.roll_segments(col, o1, [[k]]), col)
    assert np.array_equal(NS.roll_segments(col, o1, [[-2 ** 31]]), np.roll(col, (-2 ** 31) % 7, axis=0))
    assert np.array_equal(NS.roll_segments(col, o1, [[2 ** 31 - 1]]), np.roll(col, (2 ** 31 - 1) % 7, axis=0))
    with pytest.raises(ValueError):
        NS.roll_segments(col, o1, [[1, 2]])


def test_fixed_shift_set():
    sh = NS.shifts()
    lens = np.asarray(NS.LENS)[:, None]
    assert sh.shape == (6, len(NS.LENS), NS.N_NEURON)
    assert np.all(sh[0] == 0) and np.all(sh[1] == lens)
    assert np.all((sh[2] >= 0) & (sh[2] < lens)) and np.all(sh[3] < 0) and np.all(sh[4] > lens)
    assert np.abs(sh[5]).max() > 1000 and np.abs(sh).max() < 2 ** 31
    d = NS.planted_data(64)
    off = R.offsets(NS.LENS)
    assert np.array_equal(NS.roll_segments(d['y'], off, sh[0]), d['y'])
    assert np.array_equal(NS.roll_segments(d['y'], off, sh[1]), d['y'])
    assert not np.array_equal(NS.roll_segments(d['y'], off, sh[2]), d['y'])


# ----------------------------------------------------------------------------- (c) validation
def test_checked_neuron_shift():
    ok = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    t = _checked_neuron_shift(ok, 2, 3, 4)
    assert t.dtype == torch.int32 and np.array_equal(t.numpy(), ok)
    assert _checked_neuron_shift(torch.as_tensor(ok.astype(np.int16)), 2, 3, 4).dtype == torch.int32
    for bad in (ok[:1], ok[:, :2], ok[:, :, :3], ok.reshape(2, 12), ok.astype(np.float32), ok.astype(bool)):
        with pytest.raises(ValueError, match="shift"):
            _checked_neuron_shift(bad, 2, 3, 4)
    with pytest.raises(ValueError, match="int32"):
        _checked_neuron_shift(np.full((1, 1, 1), 2 ** 31, np.int64), 1, 1, 1)
    assert int(_checked_neuron_shift(np.full((1, 1, 1), -2 ** 31, np.int64), 1, 1, 1)[0, 0, 0]) == -2 ** 31


def test_errors_before_any_device_work():
    rng = np.random.default_rng(0)
    N, L, T = 5, 16, 20
    y = rng.poisson(1.0, size=(T, N)).astype(np.float32)
    tun = rng.random((L, N)) + 0.1
    seg = [[0, 5], [8, 20]]
    kind = dict(shuffle='neuron_circular')
    K = np.exp(-np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]) / 3.0)
    for cls in (PoissonGPLVMJump1D, GaussianGPLVMJump1D):
        m = cls(N, n_latent_bin=L, custom_transition_kernel=K)
        with pytest.raises(NotImplementedError, match="shuffle_test_segments.*custom_transition_kernel"):
            m.shuffle_test_segments(y, seg, tuning=tun, **kind)
    for cls in (PoissonGPLVM1D, GaussianGPLVM1D):
        with pytest.raises(NotImplementedError, match="latent-only"):
            cls(N, n_latent_bin=L).shuffle_test_segments(y, seg, tuning=tun, **kind)
    for cls in (PoissonGPLVMJump1D, GaussianGPLVMJump1D):
        m = cls(N, n_latent_bin=L)
        for bad in (0, -3, 2.5):
            with pytest.raises(ValueError, match="n_shuffle"):
                m.shuffle_test_segments(y, seg, n_shuffle=bad, tuning=tun, **kind)
        for bad in ([[5, 5]], [[0, T + 1]]):
            with pytest.raises(ValueError):
                m.shuffle_test_segments(y, bad, n_shuffle=4, tuning=tun, **kind)
        # a per-time neuron mask would have to roll with the spikes
        with pytest.raises(ValueError, match="1-D ma_neuron"):
            m.shuffle_test_segments(y, seg, n_shuffle=4, tuning=tun, ma_neuron=np.ones((T, N)), **kind)
        for bad in (-1, 0.5):
            with pytest.raises(ValueError, match="min_shift"):
                m.shuffle_test_segments(y, seg, n_shuffle=4, tuning=tun, min_shift=bad, **kind)
        # the caller's shifts: shape, dtype; they select the shuffle whatever `shuffle` says
        ok = np.zeros((4, 2, N), np.int64)
        for bad in (ok[:3], ok[:, :1], ok[:, :, :-1], ok[0], ok.astype(np.float64)):
            for kw in (kind, {}):
                with pytest.raises(ValueError, match="shift"):
                    m.shuffle_test_segments(y, seg, n_shuffle=4, tuning=tun, shift=bad, **kw)
        # not together with perm / rot
        ident = np.tile(np.arange(17, dtype=np.int32), (4, 1))
        for kw in (dict(shift=ok, perm=ident), dict(shift=ok, rot=ident), dict(perm=ident, **kind),
                   dict(rot=ident, **kind)):
            with pytest.raises(ValueError, match="perm / rot"):
                m.shuffle_test_segments(y, seg, n_shuffle=4, tuning=tun, **kw)


# ----------------------------------------------------------------------------- entry point
def test_header_binding_and_library_agree_on_the_new_name():
    txt = open(os.path.join(ROOT, 'include', 'pmg.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pmg_[a-z0-9_]+)\s*\(', txt))
    lib = ctypes.CDLL(_native.LIB_PATH)
    name = 'pmg_segment_roll_prepare'
    assert name in declared and name in _native.EXPORTED_SYMBOLS and name in _native._SIGS and hasattr(lib, name)
    assert len(_native._SIGS[name][0]) == 14
    assert os.path.exists(os.path.join(ROOT, 'poor_man_gplvm_amd', 'csrc', 'segment_roll.hip'))
    assert _native.ABI_VERSION == 4 == lib.pmg_abi_version()


def test_entry_point_argument_checks():
    """Every check precedes any HIP call (the pointers are never dereferenced)."""
    lib = _native.load()
    one = ctypes.c_void_p(256)

    def call(**kw):
        a = dict(y=one, yq=one, ma=None, T=10, N=5, Kp=128, seg_off=one, S=2, shift=one, R=3, y_out=ctypes.c_void_p(512),
                 yq_out=ctypes.c_void_p(1024), gconst_out=one)
        a.update(kw)
        rc = lib.pmg_segment_roll_prepare(a['y'], a['yq'], a['ma'], a['T'], a['N'], a['Kp'], a['seg_off'], a['S'],
                                          a['shift'], a['R'], a['y_out'], a['yq_out'], a['gconst_out'], None)
        return rc, lib.pmg_last_error()

    for kw, word in ((dict(T=0), b'T=0'), (dict(T=-4), b'T=-4'), (dict(N=0), b'N=0'), (dict(Kp=4), b'Kp=4'),
                     (dict(Kp=100), b'Kp=100'), (dict(N=200), b'Kp=128'), (dict(S=-1), b'S=-1'),
                     (dict(R=0), b'R=0'), (dict(R=-2), b'R=-2'),
                     (dict(S=1 << 20, R=1 << 20), b'exceed the grid'),
                     (dict(T=1 << 52, R=1 << 20, S=1), b'int64'),
                     (dict(y_out=None, yq_out=None, gconst_out=None), b'every output is null'),
                     (dict(y=None), b'y_out needs y'), (dict(yq=None), b'yq_out needs yq'),
                     (dict(y=None, yq=None, y_out=None, yq_out=None), b'gconst_out needs y or yq'),
                     (dict(seg_off=None), b'seg_off is null'), (dict(shift=None), b'shift is null'),
                     (dict(y_out=one), b'aliases'), (dict(yq_out=one), b'aliases')):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)


# ----------------------------------------------------------------------------- (d) the reference discriminates
@pytest.mark.parametrize("case", [c for c in SR.CASES if c[0] > 1], ids=_id)
def test_reference_moves_under_every_wrong_roll(case):
    L, band = case
    d, _, off, sh, ref = NS.neuron_shuffle_reference(L, band)
    assert ref.shape == (NS.N_SHUFFLE, len(NS.LENS)) and off[-1] == 120 and d['y'].shape == (120, NS.N_NEURON)
    assert d['y'].sum() > 120 and np.all(np.isfinite(ref))
    # rows 0 and 1 are the identity
    assert np.array_equal(ref[0], ref[1])
    # eligible: >= 3 rows and two spiking neurons whose effective shifts differ (rows 2-5 only)
    mask = NS.eligible(d['y'], off, sh)
    assert not mask[:2].any() and mask.sum() >= 30, int(mask.sum())
    shares = {}
    for mutate in NS.MUTATIONS:
        bad = NS.neuron_shuffle_reference(L, band, mutate=mutate)[4]
        moved = np.abs(bad - ref) >= 1e-5 * np.abs(ref)
        shares[mutate] = moved[mask].mean()
        rel = (np.abs(bad - ref) / np.abs(ref))[mask]
        print(f"{_id(case)} {mutate}: moved {shares[mutate]:.1%} of {int(mask.sum())} pairs, median move "
              f"{np.median(rel):.2e}")
        assert np.array_equal(bad[0], ref[0])       # the zero row moves under no mutation
    for mutate, share in shares.items():
        assert share >= 0.80, (mutate, share)
