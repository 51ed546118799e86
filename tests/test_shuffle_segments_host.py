"""Host-side checks of shuffle_test_segments / pmg_segment_shuffle_logz (no GPU).

(a) shuffle_p_values on hand cases; (b) the errors the model method raises before any device
work, the generated permutations and the entry point's argument checks; (c) the input
conditions of tests/test_gpu_shuffle_segments.py: on the float64 reference of
tests/shuffle_ref.py with its fixed shuffle set, a scan that ignores perm, one that ignores rot
and one that clamps l + rot to L - 1 where it should wrap each move logZ by >= 1e-5 |logZ| --
100 x the GPU bar of 1e-7 -- in >= 80 % of the eligible (shuffle, segment) pairs of every case
with L > 1.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from poor_man_gplvm_amd import _native
from poor_man_gplvm_amd.core import (GaussianGPLVM1D, GaussianGPLVMJump1D, PoissonGPLVM1D, PoissonGPLVMJump1D,
                                     _checked_shuffle_index, check_segment_permutations, segment_permutations,
                                     shuffle_p_values)
from tests import sample_ref as SR
from tests import segments_ref as R
from tests import shuffle_ref as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(case):
    return f"L{case[0]}-band{case[1]}"


# ----------------------------------------------------------------------------- (a) p-values
def test_shuffle_p_values_hand_cases():
    true = np.array([0.0, 5.0, -1.0, 2.0])
    shuf = np.array([[1.0, 1.0, -2.0, 2.0],
                     [-1.0, 2.0, -3.0, 2.0],
                     [0.5, 3.0, -1.5, 1.0]])
    p = shuffle_p_values(true, shuf)
    assert p.dtype == np.float64 and p.shape == (4,)
    # 2 of 3 above; none; none; two ties count as >=
    np.testing.assert_array_equal(p, np.array([3, 1, 1, 3]) / 4.0)
    # smallest and largest values a call can give
    assert shuffle_p_values([1.0], np.zeros((999, 1)))[0] == 1 / 1000
    assert shuffle_p_values([0.0], np.ones((9, 1)))[0] == 1.0
    # lists are fine; shapes are checked
    assert shuffle_p_values([0.0, 0.0], [[0.0, -1.0]]).tolist() == [1.0, 0.5]
    for bad in (([0.0], [0.0]), ([0.0, 1.0], [[0.0]]), ([[0.0]], [[0.0]]), ([0.0], np.zeros((0, 1)))):
        with pytest.raises(ValueError):
            shuffle_p_values(*bad)


def test_a_one_row_event_under_time_bin_has_p_one():
    """The only permutation of one row is the identity: every shuffle ties with the true score."""
    off = np.array([0, 1, 4], np.int64)
    perm = segment_permutations(off, 16, torch.Generator().manual_seed(0), 'cpu').numpy()
    assert np.all(perm[:, 0] == 0)
    true = np.array([-3.25, -7.0])
    shuf = np.stack([np.full(16, true[0]), true[1] - 1.0 - np.arange(16)], 1)   # event 0: the same value back
    p = shuffle_p_values(true, shuf)
    assert p[0] == 1.0 and p[1] == 1 / 17


# ----------------------------------------------------------------------------- (b) validation
def test_generated_permutations_stay_within_their_segments():
    off = R.offsets(R.LENS)
    gen = torch.Generator().manual_seed(3)
    perm = segment_permutations(off, 64, gen, 'cpu')
    assert perm.dtype == torch.int32 and tuple(perm.shape) == (64, 120)
    check_segment_permutations(perm, off)
    p = perm.numpy()
    for s in range(len(R.LENS)):
        a, b = int(off[s]), int(off[s + 1])
        assert np.array_equal(np.sort(p[:, a:b], axis=1), np.tile(np.arange(a, b), (64, 1))), s
    # they do shuffle: the 33-row event is the identity in no row, and rows differ
    a, b = int(off[10]), int(off[11])
    assert not np.any(np.all(p[:, a:b] == np.arange(a, b), axis=1))
    assert len({tuple(r) for r in p[:, a:b]}) == 64
    # the same generator state gives the same permutations
    again = segment_permutations(off, 64, torch.Generator().manual_seed(3), 'cpu')
    assert torch.equal(perm, again)
    # every position of a 3-row event is taken about equally often (2000 draws, 6 sigma)
    q = segment_permutations(np.array([0, 3], np.int64), 2000, torch.Generator().manual_seed(4), 'cpu').numpy()
    for t in range(3):
        for v in range(3):
            assert abs(np.mean(q[:, t] == v) - 1 / 3) < 6 * np.sqrt(2 / 9 / 2000)


def test_check_segment_permutations_and_index_arrays():
    off = np.array([0, 3, 5], np.int64)
    ok = np.array([[2, 0, 1, 4, 3], [0, 1, 2, 3, 4]], np.int32)
    check_segment_permutations(ok, off)
    check_segment_permutations(torch.as_tensor(ok.astype(np.int64)), off)
    for bad in ([[2, 0, 3, 4, 1]],        # crosses the boundary
                [[0, 0, 1, 3, 4]],        # a row twice
                [[0, 1, 2, 3, 5]],        # outside the rows
                [[0, 1, 2, 3, -1]]):
        with pytest.raises(ValueError, match="permutation of each segment"):
            check_segment_permutations(np.array(bad, np.int32), off)
    t = _checked_shuffle_index(ok.astype(np.int64), 'perm', 2, 5)
    assert t.dtype == torch.int32 and np.array_equal(t.numpy(), ok)
    assert _checked_shuffle_index(torch.as_tensor(ok), 'rot', 2, 5).dtype == torch.int32
    for bad in (ok[:1], ok[:, :4], ok.T, ok[0], ok.astype(np.float32), ok.astype(bool)):
        with pytest.raises(ValueError, match="rot"):
            _checked_shuffle_index(bad, 'rot', 2, 5)
    with pytest.raises(ValueError, match="int32"):
        _checked_shuffle_index(np.array([[2 ** 31]], np.int64), 'rot', 1, 1)


def test_errors_before_any_device_work():
    rng = np.random.default_rng(0)
    N, L, T = 5, 16, 20
    y = rng.poisson(1.0, size=(T, N)).astype(np.float32)
    tun = rng.random((L, N)) + 0.1
    seg = [[0, 5], [8, 20]]
    Ttot = 17
    K = np.exp(-np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]) / 3.0)
    # dense kernel
    for cls in (PoissonGPLVMJump1D, GaussianGPLVMJump1D):
        m = cls(N, n_latent_bin=L, custom_transition_kernel=K)
        with pytest.raises(NotImplementedError, match="shuffle_test_segments.*custom_transition_kernel"):
            m.shuffle_test_segments(y, seg, tuning=tun)
    # band > 32
    m = PoissonGPLVMJump1D(N, n_latent_bin=64)
    with pytest.raises(NotImplementedError, match="band"):
        m.shuffle_test_segments(y, seg, tuning=rng.random((64, N)) + 0.1, hyperparam={'movement_variance': 6.0})
    # latent-only models
    for cls in (PoissonGPLVM1D, GaussianGPLVM1D):
        with pytest.raises(NotImplementedError, match="latent-only"):
            cls(N, n_latent_bin=L).shuffle_test_segments(y, seg, tuning=tun)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="n_shuffle"):
            m.shuffle_test_segments(y, seg, n_shuffle=bad, tuning=tun)
    for bad in ('cell_identity', 'TIME_BIN', None):
        with pytest.raises(ValueError, match="shuffle must be one of"):
            m.shuffle_test_segments(y, seg, n_shuffle=4, shuffle=bad, tuning=tun)
    # intervals
    for bad in ([[5, 5]], [[0, T + 1]], [[-2, 3]], [[0, 3, 4]]):
        with pytest.raises(ValueError):
            m.shuffle_test_segments(y, bad, n_shuffle=4, tuning=tun)
    # caller-supplied shuffles: shape, dtype, then the permutation property
    ident = np.tile(np.arange(Ttot, dtype=np.int32), (4, 1))
    for name in ('perm', 'rot'):
        for bad in (ident[:3], ident[:, :-1], ident.T, ident[0], ident.astype(np.float64)):
            with pytest.raises(ValueError, match=name):
                m.shuffle_test_segments(y, seg, n_shuffle=4, tuning=tun, **{name: bad})
    bad = ident.copy()
    bad[2, 4], bad[2, 5] = 5, 4                      # rows 4 and 5 lie in different events
    with pytest.raises(ValueError, match="permutation of each segment"):
        m.shuffle_test_segments(y, seg, n_shuffle=4, perm=bad, tuning=tun)
    bad = ident.copy()
    bad[1, 7] = 8
    with pytest.raises(ValueError, match="permutation of each segment"):
        m.shuffle_test_segments(y, seg, n_shuffle=4, perm=torch.as_tensor(bad), tuning=tun)
    # a rotation together with a latent mask, generated or supplied
    mask = np.ones(L)
    mask[3] = 0
    for kw in (dict(shuffle='column_cycle'), dict(shuffle='both'), dict(rot=ident % L)):
        with pytest.raises(ValueError, match="ma_latent"):
            m.shuffle_test_segments(y, seg, n_shuffle=4, tuning=tun, ma_latent=mask, **kw)


def test_batches_are_whole_generation_blocks():
    m = PoissonGPLVMJump1D(3, n_latent_bin=8)
    g = m.SHUFFLE_GEN_BLOCK
    assert m._shuffle_batch(100, 1000) % g == 0 and m._shuffle_batch(100, 1000) >= 1000
    m.SHUFFLE_BATCH_BYTES = 1
    assert m._shuffle_batch(100, 1000) == g
    m.SHUFFLE_BATCH_BYTES = 24 * 100 * g * 3 + 5
    assert m._shuffle_batch(100, 1000) == 3 * g


# ----------------------------------------------------------------------------- entry point
def test_header_binding_and_library_agree_on_the_new_name():
    txt = open(os.path.join(ROOT, 'include', 'pmg.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pmg_[a-z0-9_]+)\s*\(', txt))
    lib = ctypes.CDLL(_native.LIB_PATH)
    name = 'pmg_segment_shuffle_logz'
    assert name in declared and name in _native.EXPORTED_SYMBOLS and name in _native._SIGS and hasattr(lib, name)
    assert len(_native._SIGS[name][0]) == 14
    assert os.path.exists(os.path.join(ROOT, 'poor_man_gplvm_amd', 'csrc', 'segment_shuffle.hip'))


def test_entry_point_argument_checks():
    """Every check precedes any HIP call (the pointers are never dereferenced)."""
    lib = _native.load()
    tr = _native.Transition()
    tr.L, tr.band = 64, 9
    tr.invz = 256
    one = ctypes.c_void_p(256)

    def call(**kw):
        a = dict(delta=one, phi=one, m=one, T=10, seg_off=one, S=2, order=None, tr=ctypes.byref(tr), scale=1.0,
                 perm=one, rot=one, R=3, logz=one)
        a.update(kw)
        rc = lib.pmg_segment_shuffle_logz(a['delta'], a['phi'], a['m'], a['T'], a['seg_off'], a['S'], a['order'],
                                          a['tr'], a['scale'], a['perm'], a['rot'], a['R'], a['logz'], None)
        return rc, lib.pmg_last_error()

    rc, msg = call(T=0)
    assert rc == -1 and b'T=0' in msg
    rc, msg = call(S=0)
    assert rc == -1 and b'S=0' in msg
    rc, msg = call(R=0)
    assert rc == -1 and b'R=0' in msg
    rc, msg = call(S=1 << 20, R=1 << 20)
    assert rc == -1 and b'exceed' in msg
    rc, msg = call(T=1 << 31)
    assert rc == -1 and b'int32' in msg
    for name in ('delta', 'phi', 'm', 'seg_off', 'logz'):
        rc, msg = call(**{name: None})
        assert rc == -1 and (b' ' + name.encode() + b' is null') in msg, (name, msg)
    rc, msg = call(scale=float('nan'))
    assert rc == -1 and b'NaN' in msg
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


# ----------------------------------------------------------------------------- (c) the reference discriminates
@pytest.mark.parametrize("case", [c for c in SR.CASES if c[0] > 1], ids=_id)
def test_reference_moves_under_every_wrong_scan(case):
    L, band = case
    _, _, off, perm, rot, ref = SH.shuffle_reference(L, band)
    assert ref.shape == (8, len(R.LENS)) and off[-1] == 120 and perm.shape == rot.shape == (8, 120)
    assert rot.min() >= 0 and rot.max() < L and np.all(rot[:3] == 0) and np.all(perm[3:5] == np.arange(120))
    ep, er = SH.eligible(off, perm, rot)
    assert ep.sum() >= 40 and er.sum() >= 50
    shares = {}
    for mutate, mask in (('ignore_perm', ep), ('ignore_rot', er), ('clamp_rot', er)):
        bad = SH.shuffle_reference(L, band, mutate=mutate)[5]
        moved = np.abs(bad - ref) >= 1e-5 * np.abs(ref)
        shares[mutate] = moved[mask].mean()
        rel = (np.abs(bad - ref) / np.abs(ref))[mask]
        print(f"{_id(case)} {mutate}: moved {shares[mutate]:.1%} of {int(mask.sum())} pairs, median move "
              f"{np.median(rel):.2e}")
        # pairs that are not eligible for a perm mutation because they carry no perm do not move at all
        if mutate == 'ignore_perm':
            assert np.array_equal(bad[3:5], ref[3:5])
        else:
            assert np.array_equal(bad[:3], ref[:3])
    for mutate, share in shares.items():
        assert share >= 0.80, (mutate, share)
