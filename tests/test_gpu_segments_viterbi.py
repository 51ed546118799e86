"""decode_latent_segments_viterbi / pmg_segment_viterbi (csrc/viterbi.hip) on the
device: the MAP paths of many ragged events in one call.

Every case is one (N, L) shape -- the smallest that reach each lane layout J in {1, 2, 4, 8,
16} and both row-load forms -- crossed with movement_variance in {0.5, 1, 2, 3} (band taps
WP 5, 9, 17, 32), on a set of ~25 events that holds the lengths 1, 2, 3, the prefetch ring's
PF-1, PF, PF+1, 2 PF+1 (PF = 4, or 2 at J = 16) and the trace piece's NP-1, NP, NP+1, 2 NP+1
(NP = 64 rows for L <= 256, 32 for L <= 512, 16 for L <= 1024), cut from one recording at
random (unsorted, overlapping) starts.  Checked per case:
  1. bit identity: every event's map_dynamics, map_latent and log_joint_map equal
     decode_latent_viterbi on that event alone (tests/test_gpu_viterbi.py validates that call
     against the float64 reference);
  2. for a handful of events, conditions (a) feasibility, (b) optimality and (d) score of
     tests/test_gpu_viterbi.py against tests/viterbi_ref.py with its bound
     B = 16 T_s 2^-24 M (not its path-agreement cap (c): on a 3-bin event one near-tie
     flips the whole event; the score bound is the meaningful check);
  3. log_joint_map[s] <= log_marginal_final[s] of decode_latent_segments (slack 1e-6 |.|).
Then: independence of an event from the rest of the call (permutation, subset, `order`, list
input), rows that no segment owns and empty segments at the C-ABI level, masks, likelihood
scale, the Gaussian and the latent-only models, determinism.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import gplvm_oracle as O
from poor_man_gplvm_amd import (GaussianGPLVMJump1D, PoissonGPLVM1D, PoissonGPLVMJump1D, _native, banded_transition,
                                viterbi_log_pi0)
from poor_man_gplvm_amd.core import segment_order
from tests import viterbi_ref as V
from tests.synth import make

pytestmark = pytest.mark.gpu

T_REC = 700                                   # rows of the recording the events are cut from
SHAPES = [(24, 64), (30, 100), (20, 150), (64, 256), (48, 512), (32, 1024)]
MVS = [0.5, 1.0, 2.0, 3.0]
WP_OF_MV = {0.5: 5, 1.0: 9, 2.0: 17, 3.0: 32}


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


@functools.lru_cache(maxsize=None)
def _data(N, L, mv=1.0):
    return make(N, L, T_REC, mv=mv)


def ring_depth(L):
    return 2 if L > 512 else 4                # vit_pf<J>(): J = 16 for L > 512


def piece_rows(L):
    return 64 if L <= 256 else (32 if L <= 512 else 16)


def event_lengths(L):
    """The lengths every case holds, then 14 ordinary ones (3 .. 40 rows), shuffled."""
    PF, NP = ring_depth(L), piece_rows(L)
    must = [1, 2, 3, PF - 1, PF, PF + 1, 2 * PF + 1, NP - 1, NP, NP + 1, 2 * NP + 1]
    rng = np.random.default_rng(L)
    lens = np.array(must + list(rng.integers(3, 41, size=14)), np.int64)
    return must, lens[rng.permutation(len(lens))]


def intervals(L, seed=0):
    """(S, 2) [start, stop) rows of the recording: unsorted, overlapping."""
    _, lens = event_lengths(L)
    start = np.random.default_rng(100 + seed).integers(0, T_REC - lens + 1)
    return np.stack([start, start + lens], 1)


def test_event_set_covers_the_ring_and_the_trace_piece():
    for _, L in SHAPES:
        must, lens = event_lengths(L)
        assert set(must) <= set(lens.tolist()) and 20 <= len(lens) <= 40 and lens.sum() <= 1500
        assert {1, 2, 3} <= set(must)
        seg = intervals(L)
        assert np.any(seg[1:, 0] < seg[:-1, 0])                                        # unsorted
        order = np.argsort(seg[:, 0])
        assert np.any(seg[order][1:, 0] < np.maximum.accumulate(seg[order][:, 1])[:-1])   # overlapping


def _singles(m, y, seg, **kw):
    return [m.decode_latent_viterbi(y[a:b], **kw) for a, b in seg]


def _assert_events_equal(res, singles, latent_only=False):
    off = res['segment_offsets']
    assert off.dtype == np.int64 and len(off) == len(singles) + 1
    assert res['map_latent'].dtype == np.int32 and res['map_latent'].shape == (off[-1],)
    assert res['log_joint_map'].dtype == np.float64 and res['log_joint_map'].shape == (len(singles),)
    if latent_only:
        assert 'map_dynamics' not in res
    else:
        assert res['map_dynamics'].dtype == np.int32 and res['map_dynamics'].shape == (off[-1],)
    for s, one in enumerate(singles):
        a, b = int(off[s]), int(off[s + 1])
        assert np.array_equal(res['map_latent'][a:b], one['map_latent']), s
        if not latent_only:
            assert np.array_equal(res['map_dynamics'][a:b], one['map_dynamics']), s
        assert res['log_joint_map'][s] == one['log_joint_map'], (s, res['log_joint_map'][s], one['log_joint_map'])


def _check_against_reference(d, l, lj, u, tr, ma_latent=None, what=""):
    """Conditions (a), (b) and (d) of tests/test_gpu_viterbi.py for one event."""
    T, L = u.shape
    logK0, logA = V.banded_logK(tr), V.device_logA(tr)
    lp0 = V.log_pi0(logK0, logA)
    ref_path, ref_score = V.viterbi(u, logK0, logA, lp0)
    # (a)
    assert l.shape == (T,) and d.shape == (T,)
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
    print(f"{what} T_s={T} L={L} score_ref={s_ref:.6f} gap={s_ref - s_dev:.3e} B={B:.3e} "
          f"differ={int(np.sum(np.any(path != ref_path, axis=1)))} lj-score={lj - s_dev:.3e}")
    assert np.isfinite(s_dev)
    assert s_ref - s_dev <= B
    # (d)
    assert abs(lj - s_dev) <= B


def _handful(L, seg):
    """Events to take to the reference: the first of lengths 1, 2, PF + 1, NP + 1 and 2 PF + 1, and one ordinary."""
    lens = (seg[:, 1] - seg[:, 0]).tolist()
    want = [1, 2, ring_depth(L) + 1, 2 * ring_depth(L) + 1, piece_rows(L) + 1]
    idx = [lens.index(n) for n in want]
    idx.append(next(s for s, n in enumerate(lens) if s not in idx and 10 <= n <= 40))
    return sorted(set(idx))


@pytest.mark.parametrize("mv", MVS)
@pytest.mark.parametrize("N,L", SHAPES)
def test_events_equal_single_decodes_and_the_reference(N, L, mv):
    dat = _data(N, L, mv)
    y, tun = dat['y'], dat['tuning']
    seg = intervals(L)
    tr = banded_transition(L, mv, 0.01, 0.01)
    assert (tr.band <= 5, tr.band <= 9, tr.band <= 17, True).index(True) == MVS.index(mv)    # WP 5, 9, 17, 32
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, movement_variance=mv)
    res = m.decode_latent_segments_viterbi(y, seg, tuning=tun)
    off = res['segment_offsets']
    assert np.array_equal(np.diff(off), seg[:, 1] - seg[:, 0])
    # 1. bit identity with the per-event call
    _assert_events_equal(res, _singles(m, y, seg, tuning=tun))
    # 2. a handful of events against the float64 reference
    u_all = O.loglikelihood_poisson_all(y, tun)
    for s in _handful(L, seg):
        a, b = int(off[s]), int(off[s + 1])
        _check_against_reference(res['map_dynamics'][a:b], res['map_latent'][a:b], float(res['log_joint_map'][s]),
                                 u_all[seg[s, 0]:seg[s, 1]], tr, what=f"event {s}")
    # 3. a path's joint never exceeds the marginal
    logz = m.decode_latent_segments(y, seg, tuning=tun)['log_marginal_final']
    lj = res['log_joint_map']
    print(f"L={L} band={tr.band}: min (logZ - log_joint_map) = {np.min(logz - lj):.3e}")
    assert np.all(lj <= logz + 1e-6 * np.abs(logz))


# ----------------------------------------------------------------------------- independence
@pytest.mark.parametrize("N,L,mv", [(30, 100, 1.0), (48, 512, 2.0)])
def test_events_are_independent_bit_for_bit(N, L, mv):
    dat = _data(N, L, mv)
    y, tun = dat['y'], dat['tuning']
    seg = intervals(L)
    S = len(seg)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, movement_variance=mv)
    base = m.decode_latent_segments_viterbi(y, seg, tuning=tun)
    off = base['segment_offsets']

    def same(out, k, s):
        """event k of `out` == event s of `base`"""
        o = out['segment_offsets']
        for key in ('map_dynamics', 'map_latent'):
            assert np.array_equal(out[key][o[k]:o[k + 1]], base[key][off[s]:off[s + 1]]), (key, k, s)
        assert out['log_joint_map'][k] == base['log_joint_map'][s], (k, s)

    # permuting the events permutes the outputs
    perm = np.random.default_rng(3).permutation(S)
    outp = m.decode_latent_segments_viterbi(y, seg[perm], tuning=tun)
    for k, s in enumerate(perm):
        same(outp, k, s)
    # a subset reproduces its members
    sub = np.sort(np.random.default_rng(4).choice(S, size=S // 3, replace=False))
    outs = m.decode_latent_segments_viterbi(y, seg[sub], tuning=tun)
    for k, s in enumerate(sub):
        same(outs, k, s)
    # the list-of-arrays form equals the interval form
    outl = m.decode_latent_segments_viterbi([y[a:b] for a, b in seg], tuning=tun)
    assert np.array_equal(outl['segment_offsets'], off)
    for s in range(S):
        same(outl, s, s)
    # determinism
    again = m.decode_latent_segments_viterbi(y, seg, tuning=tun)
    for key in ('map_dynamics', 'map_latent', 'log_joint_map'):
        assert np.array_equal(again[key], base[key]), key


def _engine(m, y, tun, likelihood_scale=1.0):
    hp, _, _ = m._dynamics_decode_args(m._decode_hp({}))
    eng = m._decode_engine(np.ascontiguousarray(y, dtype=np.float32), tun, hp, None, None, exact=False)
    eng.emission(likelihood_scale)
    return eng


@pytest.mark.parametrize("N,L,mv", [(30, 100, 1.0), (32, 1024, 1.0)])
def test_order_changes_scheduling_only(N, L, mv):
    dat = _data(N, L, mv)
    seg = intervals(L)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L, movement_variance=mv)
    yc = np.concatenate([dat['y'][a:b] for a, b in seg])
    off = np.concatenate([[0], np.cumsum(seg[:, 1] - seg[:, 0])]).astype(np.int64)
    S = len(seg)
    eng = _engine(m, yc, dat['tuning'])
    so = torch.as_tensor(off, device='cuda')
    outs = []
    for order in (None, segment_order(off), np.random.default_rng(5).permutation(S).astype(np.int32)):
        od = None if order is None else torch.as_tensor(order, device='cuda')
        outs.append(tuple(t.cpu().numpy() for t in eng.segment_viterbi(1.0, so, od)))
    eng.check_status()
    for out in outs[1:]:
        for k in range(3):
            assert np.array_equal(outs[0][k], out[k]), k
    api = m.decode_latent_segments_viterbi(dat['y'], seg, tuning=dat['tuning'])
    assert np.array_equal(outs[0][0], api['map_dynamics']) and np.array_equal(outs[0][1], api['map_latent'])
    assert np.array_equal(outs[0][2], api['log_joint_map'])
    with pytest.raises(ValueError):
        eng.segment_viterbi(1.0, so.to(torch.int32))
    with pytest.raises(ValueError):
        eng.segment_viterbi(1.0, so, torch.zeros(S + 1, dtype=torch.int32, device='cuda'))


# ----------------------------------------------------------------------------- C ABI: unowned rows, empty segments
SENTINEL = -77


def _raw(eng, off, order=None, likelihood_scale=1.0):
    """pmg_segment_viterbi on the engine's emission with outputs pre-filled with a sentinel."""
    lib = _native.load()
    T, S = eng.T, len(off) - 1
    need = int(lib.pmg_segment_viterbi_workspace_size(T, eng.L, S))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    lp0 = torch.as_tensor(viterbi_log_pi0(eng._tr), device='cuda')
    pd = torch.full((T,), SENTINEL, dtype=torch.int32, device='cuda')
    pl = torch.full((T,), SENTINEL, dtype=torch.int32, device='cuda')
    lj = torch.full((S,), float(SENTINEL), dtype=torch.float64, device='cuda')
    so = torch.as_tensor(np.asarray(off, np.int64), device='cuda')
    od = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device='cuda')
    _native.check(lib.pmg_segment_viterbi(_native.ptr(eng.delta), _native.ptr(eng.phi), _native.ptr(eng.rblk), T,
                                          _native.ptr(so), S, _native.ptr(od), ctypes.byref(eng._tr_c),
                                          _native.ptr(lp0), float(likelihood_scale), _native.ptr(pd), _native.ptr(pl),
                                          _native.ptr(lj), _native.ptr(ws), ws.numel(), _native.stream_handle()),
                  "pmg_segment_viterbi")
    torch.cuda.synchronize()
    return pd.cpu().numpy(), pl.cpu().numpy(), lj.cpu().numpy()


@pytest.mark.parametrize("N,L", [(24, 64), (20, 150), (32, 1024)])
def test_unowned_rows_and_empty_segments(N, L):
    dat = _data(N, L)
    T = 90
    y = dat['y'][:T]
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    eng = _engine(m, y, dat['tuning'])
    # rows 0 .. 2 and 70 .. 89 belong to no segment; segment 1 is empty; segment 4 is one row
    off = [3, 10, 10, 45, 69, 70]
    pd, pl, lj = _raw(eng, off)
    owned = np.zeros(T, bool)
    owned[3:70] = True
    assert np.all(pd[~owned] == SENTINEL) and np.all(pl[~owned] == SENTINEL)
    assert lj[1] == 0.0
    for s in (0, 2, 3, 4):
        a, b = off[s], off[s + 1]
        one = m.decode_latent_viterbi(y[a:b], tuning=dat['tuning'])
        assert np.array_equal(pd[a:b], one['map_dynamics']) and np.array_equal(pl[a:b], one['map_latent']), s
        assert lj[s] == one['log_joint_map'], s
    # offsets past either end are clamped to 0 <= a <= b <= T (here: [0, 4), [4, 80), [80, 90), empty,
    # empty); entries of `order` outside 0 .. S-1 are skipped, so segments 1 and 4 get no workgroup
    off2 = [-5, 4, 80, 200, 150, 150]
    pd, pl, lj = _raw(eng, off2, order=[2, 7, 0, -1, 3])
    owned = np.zeros(T, bool)
    owned[0:4] = owned[80:90] = True
    assert np.all(pd[~owned] == SENTINEL) and np.all(pl[~owned] == SENTINEL)
    assert lj[3] == 0.0 and lj[1] == SENTINEL and lj[4] == SENTINEL
    for s, (a, b) in ((0, (0, 4)), (2, (80, 90))):
        one = m.decode_latent_viterbi(y[a:b], tuning=dat['tuning'])
        assert np.array_equal(pd[a:b], one['map_dynamics']) and np.array_equal(pl[a:b], one['map_latent']), s
        assert lj[s] == one['log_joint_map'], s
    eng.check_status()


# ----------------------------------------------------------------------------- masks, scale, models
def test_latent_mask_is_honoured():
    N, L = 24, 64
    dat = _data(N, L)
    y, tun, seg = dat['y'], dat['tuning'], intervals(L)
    ma_latent = np.ones(L)
    ma_latent[np.random.default_rng(5).permutation(L)[:L // 3]] = 0
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    res = m.decode_latent_segments_viterbi(y, seg, tuning=tun, ma_latent=ma_latent)
    assert np.all(ma_latent.astype(bool)[res['map_latent']])
    _assert_events_equal(res, _singles(m, y, seg, tuning=tun, ma_latent=ma_latent))
    off = res['segment_offsets']
    u_all = O.loglikelihood_poisson_all(y, tun, ma_latent=ma_latent)
    tr = banded_transition(L, 1.0, 0.01, 0.01)
    for s in _handful(L, seg):
        a, b = int(off[s]), int(off[s + 1])
        _check_against_reference(res['map_dynamics'][a:b], res['map_latent'][a:b], float(res['log_joint_map'][s]),
                                 u_all[seg[s, 0]:seg[s, 1]], tr, ma_latent, what=f"masked event {s}")


@pytest.mark.parametrize("scale", [0.5, 2.0])
def test_likelihood_scale(scale):
    N, L = 64, 256
    dat = _data(N, L)
    y, tun, seg = dat['y'], dat['tuning'], intervals(L)
    m = PoissonGPLVMJump1D(N, n_latent_bin=L)
    res = m.decode_latent_segments_viterbi(y, seg, tuning=tun, likelihood_scale=scale)
    _assert_events_equal(res, _singles(m, y, seg, tuning=tun, likelihood_scale=scale))
    off = res['segment_offsets']
    u_all = scale * O.loglikelihood_poisson_all(y, tun)
    tr = banded_transition(L, 1.0, 0.01, 0.01)
    for s in _handful(L, seg):
        a, b = int(off[s]), int(off[s + 1])
        _check_against_reference(res['map_dynamics'][a:b], res['map_latent'][a:b], float(res['log_joint_map'][s]),
                                 u_all[seg[s, 0]:seg[s, 1]], tr, what=f"scale {scale} event {s}")
    one = m.decode_latent_segments_viterbi(y, seg, tuning=tun)
    assert not np.array_equal(one['log_joint_map'], res['log_joint_map'])


def test_gaussian_model():
    N, L = 24, 64
    dat = _data(N, L)
    y, tun, seg = dat['y'], dat['tuning'], intervals(L)
    m = GaussianGPLVMJump1D(N, noise_std=0.5, n_latent_bin=L)
    res = m.decode_latent_segments_viterbi(y, seg, tuning=tun)
    _assert_events_equal(res, _singles(m, y, seg, tuning=tun))
    off = res['segment_offsets']
    u_all = O.loglikelihood_gaussian_all(y, tun, 0.5)
    tr = banded_transition(L, 1.0)
    for s in _handful(L, seg):
        a, b = int(off[s]), int(off[s + 1])
        _check_against_reference(res['map_dynamics'][a:b], res['map_latent'][a:b], float(res['log_joint_map'][s]),
                                 u_all[seg[s, 0]:seg[s, 1]], tr, what=f"gaussian event {s}")
    logz = m.decode_latent_segments(y, seg, tuning=tun)['log_marginal_final']
    assert np.all(res['log_joint_map'] <= logz + 1e-6 * np.abs(logz))


def test_latent_only_model():
    """PoissonGPLVM1D does not refuse (its MAP path runs on the band): no map_dynamics, and
    every event equals its own decode_latent_viterbi."""
    N, L = 30, 100
    dat = _data(N, L)
    y, tun, seg = dat['y'], dat['tuning'], intervals(L)
    m = PoissonGPLVM1D(N, n_latent_bin=L)
    res = m.decode_latent_segments_viterbi(y, seg, tuning=tun)
    assert sorted(res) == ['log_joint_map', 'map_latent', 'segment_offsets']
    _assert_events_equal(res, _singles(m, y, seg, tuning=tun), latent_only=True)
    off = res['segment_offsets']
    u_all = O.loglikelihood_poisson_all(y, tun)
    tr = banded_transition(L, 1.0, 0.0, 1.0)
    for s in _handful(L, seg):
        a, b = int(off[s]), int(off[s + 1])
        l = res['map_latent'][a:b]
        _check_against_reference(np.zeros_like(l), l, float(res['log_joint_map'][s]), u_all[seg[s, 0]:seg[s, 1]], tr,
                                 what=f"latent-only event {s}")
