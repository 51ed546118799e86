"""Host-side checks of decode_latent_segments_viterbi / pmg_segment_viterbi (no GPU): the
two new names in the header, the binding and the library; the workspace query; the entry
point's argument checks; the errors the model method raises before any device work; and,
on the float64 reference, that decoding the concatenation of the events is no substitute
for decoding each event as a chain of its own."""
import ctypes
import os
import re

import numpy as np
import pytest

from poor_man_gplvm_amd import _native, banded_transition
from poor_man_gplvm_amd.core import GaussianGPLVM1D, GaussianGPLVMJump1D, PoissonGPLVM1D, PoissonGPLVMJump1D
from tests import viterbi_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pmg_segment_viterbi_workspace_size', 'pmg_segment_viterbi')


def test_header_binding_and_library_agree_on_the_new_names():
    txt = open(os.path.join(ROOT, 'include', 'pmg.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    declared = set(re.findall(r'\b(pmg_[a-z0-9_]+)\s*\(', txt))
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _native.EXPORTED_SYMBOLS, name
        assert name in _native._SIGS, name
        assert hasattr(lib, name), name
    assert re.search(r'#define\s+PMG_ABI_VERSION\s+4\b', txt)
    assert _native.ABI_VERSION == 4 and _native.load().pmg_abi_version() == 4


def test_workspace_query():
    lib = _native.load()
    assert lib.pmg_segment_viterbi_workspace_size(200, 64, 3) > 0
    assert lib.pmg_segment_viterbi_workspace_size(200, 2000, 3) == 0      # L > 1024 unsupported
    assert lib.pmg_segment_viterbi_workspace_size(0, 64, 3) == 0
    assert lib.pmg_segment_viterbi_workspace_size(200, 64, 0) == 0
    for T, L, S in ((200, 64, 3), (1000, 100, 40), (77, 150, 1), (300, 512, 7), (50, 1024, 50)):
        Lpad = lib.pmg_fwdbwd_lpad(L)
        need = lib.pmg_segment_viterbi_workspace_size(T, L, S)
        assert need >= T * Lpad
        # ~ T Lpad + 12 T bytes plus a few words per segment (256-byte aligned slices)
        assert need <= T * Lpad + 12 * T + 8 * S + 5 * 256


def test_entry_point_argument_checks():
    """Every check precedes any HIP call (the pointers are never dereferenced)."""
    lib = _native.load()
    tr = _native.Transition()
    tr.L, tr.band = 64, 9
    tr.invz = 256
    one = ctypes.c_void_p(256)

    def call(**kw):
        a = dict(delta=one, phi=one, rblk=one, T=10, seg_off=one, S=2, order=None, tr=ctypes.byref(tr), log_pi0=one,
                 s=1.0, path_d=one, path_l=one, log_joint=one, ws=one, ws_bytes=1 << 30)
        a.update(kw)
        rc = lib.pmg_segment_viterbi(a['delta'], a['phi'], a['rblk'], a['T'], a['seg_off'], a['S'], a['order'],
                                     a['tr'], a['log_pi0'], a['s'], a['path_d'], a['path_l'], a['log_joint'],
                                     a['ws'], a['ws_bytes'], None)
        return rc, lib.pmg_last_error()

    rc, msg = call(T=0)
    assert rc == -1 and b'T=0' in msg
    rc, msg = call(S=0)
    assert rc == -1 and b'S=0' in msg
    for name in ('delta', 'phi', 'rblk', 'seg_off', 'log_pi0', 'path_d', 'path_l', 'log_joint'):
        rc, msg = call(**{name: None})
        assert rc == -1 and (b' ' + name.encode() + b' is null') in msg, (name, msg)
    rc, msg = call(ws=None)
    assert rc == -1 and b'workspace is null' in msg
    rc, msg = call(tr=None)
    assert rc == -1 and b'tr is null' in msg
    rc, msg = call(s=float('nan'))
    assert rc == -1 and b'likelihood_scale' in msg
    rc, msg = call(ws_bytes=16)
    assert rc == -1 and b'workspace_bytes' in msg
    rc, msg = call(ws_bytes=lib.pmg_segment_viterbi_workspace_size(10, 64, 2) - 1)
    assert rc == -1 and b'workspace_bytes' in msg
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
    assert rc == -1 and b'invz' in msg and b'pmg_segment_viterbi' in msg


def test_errors_before_any_device_work():
    rng = np.random.default_rng(0)
    N, L, T = 5, 16, 20
    y = rng.poisson(1.0, size=(T, N)).astype(np.float32)
    tun = rng.random((L, N)) + 0.1
    seg = [[0, 5], [8, 20]]
    K = np.exp(-np.abs(np.arange(L)[:, None] - np.arange(L)[None, :]) / 3.0)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, custom_transition_kernel=K)
    with pytest.raises(NotImplementedError, match="decode_latent_segments_viterbi.*custom_transition_kernel"):
        m.decode_latent_segments_viterbi(y, seg, tuning=tun)
    with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
        m.decode_latent_segments_viterbi(y, seg)     # the model's own tuning would need the device: never reached
    m = PoissonGPLVMJump1D(N, n_latent_bin=64)
    with pytest.raises(NotImplementedError, match="band"):
        m.decode_latent_segments_viterbi(y, seg, tuning=rng.random((64, N)) + 0.1,
                                         hyperparam={'movement_variance': 6.0})
    m = PoissonGPLVMJump1D(N, n_latent_bin=1100)
    with pytest.raises(NotImplementedError):
        m.decode_latent_segments_viterbi(y, seg, tuning=rng.random((1100, N)) + 0.1)
    for cls in (GaussianGPLVMJump1D, PoissonGPLVM1D, GaussianGPLVM1D):
        with pytest.raises(NotImplementedError, match="custom_transition_kernel"):
            cls(N, n_latent_bin=L, custom_transition_kernel=K).decode_latent_segments_viterbi(y, seg, tuning=tun)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    for bad in ([[5, 5]], [[0, T + 1]], [[-2, 3]], [[0, 3, 4]]):
        with pytest.raises(ValueError):
            m.decode_latent_segments_viterbi(y, bad)
    with pytest.raises(ValueError):
        m.decode_latent_segments_viterbi(y)          # an array without intervals
    with pytest.raises(ValueError, match="1-D ma_neuron"):
        m.decode_latent_segments_viterbi([y[:5], y[5:]], ma_neuron=np.ones((T, N)))
    for cls in (PoissonGPLVM1D, GaussianGPLVM1D):    # the latent-only models do not refuse: bad intervals only
        with pytest.raises(ValueError):
            cls(N, n_latent_bin=L).decode_latent_segments_viterbi(y, [[5, 5]], tuning=tun)


def test_decoding_the_concatenation_is_no_substitute():
    """Two events whose latents are far apart: each event's own MAP path stays at its
    latent without a jump, while the MAP path of the concatenated rows must jump (or spend
    bins travelling) at the seam, and it scores the second event's first row with a
    transition instead of the prior."""
    L, n = 40, 6
    tr = banded_transition(L, 0.5, 0.01, 0.01)
    assert tr.band == 5
    logK0, logA = V.banded_logK(tr), V.device_logA(tr)
    lp0 = V.log_pi0(logK0, logA)
    lat = np.arange(L)
    u = np.concatenate([np.tile(-0.5 * (lat - 6.0) ** 2, (n, 1)), np.tile(-0.5 * (lat - 31.0) ** 2, (n, 1))])
    p1, s1 = V.viterbi(u[:n], logK0, logA, lp0)
    p2, s2 = V.viterbi(u[n:], logK0, logA, lp0)
    assert np.all(p1 == [0, 6]) and np.all(p2 == [0, 31])
    pc, sc = V.viterbi(u, logK0, logA, lp0)
    per_event = np.concatenate([p1, p2])
    assert not np.array_equal(pc, per_event)
    seam = pc[n - 1:n + 1]
    assert seam[1, 0] == 1 or abs(int(seam[1, 1]) - int(seam[0, 1])) <= tr.band    # a jump, or a move in the band
    assert pc[:, 0].sum() >= 1 or np.any(pc[:, 1] != per_event[:, 1])
    # the per-event path is not even feasible as one chain without the jump: 25 bins in one move
    assert V.path_score(per_event, u, logK0, logA, lp0)[0] == -np.inf
    assert np.isfinite(sc) and sc != s1 + s2
