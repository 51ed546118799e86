"""The shuffle kernel (pmg_segment_shuffle_logz: one wave per (segment, shuffle),
csrc/segment_shuffle.hip) and shuffle_test_segments.

DeviceEM is driven directly (emission, then segment_shuffle_logz) on the flat-band transition,
the ragged batch tests/segments_ref.LENS (120 rows) and the fixed shuffle set of
tests/shuffle_ref.py (R = 8: perm-only, rot-only and both).  tests/test_shuffle_segments_host.py shows
that a scan which ignores perm, ignores rot or clamps the rotation moves the reference by
>= 1e-5 |logZ| in >= 80 % of the eligible pairs, 100 x the bar here.

1. every (shuffle, segment) value against the float64 reference at 1e-7 |ref|, the segment
   smoother's own bar for the same step arithmetic (tests/test_gpu_segments.py);
2. rot == NULL: bit for bit the segment smoother's logz on the rows gathered by perm[r];
3. independence, bit for bit: of the other segments, of `order`, of R and r, of rot +- L;
4. a one-way dynamics matrix and likelihood_scale != 1 at the bar of 1;
5. the public API of both observation models;
6. a planted sequence gets a smaller p than rate-matched noise (direction only).
No test feeds the kernel an index outside its range.
"""
import functools

import numpy as np
import pytest
import torch

from tests import sample_ref as SR
from tests import scan_ref as S
from tests import segments_ref as R
from tests import shuffle_ref as SH
from tests.test_gpu_sample import _api_model

pytestmark = pytest.mark.gpu

BAR = 1e-7     # |logz - ref| <= BAR |ref|: tests/test_gpu_segments.py's logZ bar


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _engine(d, tr, L, y=None):
    from poor_man_gplvm_amd.engine import DeviceEM, SpikeData
    eng = DeviceEM(SpikeData(np.ascontiguousarray(d['y'] if y is None else y)), L, basis=d['B'])
    eng.set_transition(tr)
    eng.set_ma_latent(None)
    eng.set_tuning(d['tuning'])
    return eng


def _i64(x):
    return torch.as_tensor(np.asarray(x, np.int64), device='cuda')


def _i32(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, np.int32), device='cuda')


def _shuffle(d, tr, L, off, perm=None, rot=None, order=None, n_shuffle=1, likelihood_scale=1.0, rows=None):
    """Emission + one segment_shuffle_logz call over d['y'][rows]; the (R, S) host array."""
    y = d['y'] if rows is None else d['y'][rows[0]:rows[1]]
    eng = _engine(d, tr, L, y)
    eng.emission(likelihood_scale)
    lz = eng.segment_shuffle_logz(likelihood_scale, _i64(off), _i32(order), _i32(perm), _i32(rot), n_shuffle)
    eng.emission_status()
    eng.check_status()
    assert lz.dtype == torch.float64
    return lz.cpu().numpy()


def _gathered_smoother(d, tr, L, off, perm_r, likelihood_scale=1.0):
    """The materialised shuffle: delta, phi and m gathered by perm_r with torch, then
    segment_smoother forward only.  Host logz (S,)."""
    eng = _engine(d, tr, L)
    eng.emission(likelihood_scale)
    idx = _i64(perm_r)
    eng.delta.copy_(eng.delta[idx])
    eng.phi.copy_(eng.phi[idx])
    eng.mref.copy_(eng.mref[idx])
    _, _, lz = eng.segment_smoother(likelihood_scale, _i64(off))
    eng.check_status()
    return lz.cpu().numpy()


def _id(case):
    return f"L{case[0]}-band{case[1]}"


def _worst(lz, ref):
    return float(np.max(np.abs(lz - ref) / (BAR * np.abs(ref))))


# ----------------------------------------------------------------------------- 1. the float64 reference
@pytest.mark.parametrize("case", SR.CASES, ids=_id)
def test_every_pair_against_the_reference(case):
    L, band = case
    d, tr, off, perm, rot, ref = SH.shuffle_reference(L, band)
    lz = _shuffle(d, tr, L, off, perm, rot)
    assert lz.shape == ref.shape == (SH.N_SHUFFLE, len(SH.LENS))
    print(f"{_id(case)}: worst |logz - ref| / (1e-7 |ref|) = {_worst(lz, ref):.3f}")
    assert np.all(np.abs(lz - ref) <= BAR * np.abs(ref))


# ----------------------------------------------------------------------------- 2. exactness, rot == NULL
@pytest.mark.parametrize("L,band", [(250, 7), (500, 30), (64, 5), (1024, 32)], ids=lambda v: str(v))
def test_perm_only_is_the_smoother_on_the_gathered_rows(L, band):
    d, tr, off, perm, _, _ = SH.shuffle_reference(L, band)
    lz = _shuffle(d, tr, L, off, perm)
    for r in range(SH.N_SHUFFLE):
        assert np.array_equal(lz[r], _gathered_smoother(d, tr, L, off, perm[r])), r
    true = _gathered_smoother(d, tr, L, off, np.arange(120))
    none = _shuffle(d, tr, L, off, n_shuffle=SH.N_SHUFFLE)
    assert none.shape == (SH.N_SHUFFLE, len(SH.LENS))
    for r in range(SH.N_SHUFFLE):
        assert np.array_equal(none[r], true), r
    # rows 3 and 4 of the set carry the identity
    assert np.array_equal(lz[3], true) and np.array_equal(lz[4], true)


# ----------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("L,band", [(127, 7), (1000, 15)], ids=lambda v: str(v))
def test_values_are_exact_functions_of_their_own_rows(L, band):
    from poor_man_gplvm_amd.core import segment_order
    d, tr, off, perm, rot, _ = SH.shuffle_reference(L, band)
    n_s = len(SH.LENS)
    base = _shuffle(d, tr, L, off, perm, rot)
    assert np.array_equal(base, _shuffle(d, tr, L, off, perm, rot))
    # one segment alone in a call
    for s in range(n_s):
        a, b = int(off[s]), int(off[s + 1])
        one = _shuffle(d, tr, L, [0, b - a], perm[:, a:b] - a, rot[:, a:b], rows=(a, b))
        assert np.array_equal(base[:, s], one[:, 0]), s
    # order: given, reversed, None (base)
    for order in (segment_order(off), np.arange(n_s)[::-1].copy()):
        assert np.array_equal(base, _shuffle(d, tr, L, off, perm, rot, order=order))
    # shuffle r alone (R = 1), and as another row index
    for r in range(SH.N_SHUFFLE):
        assert np.array_equal(base[r], _shuffle(d, tr, L, off, perm[r:r + 1], rot[r:r + 1])[0]), r
    flip = _shuffle(d, tr, L, off, perm[::-1], rot[::-1])
    assert np.array_equal(base, flip[::-1])
    # rot is reduced mod L on the device, negative values included
    for shift in (L, -L, 3 * L, -2 * L):
        assert np.array_equal(base, _shuffle(d, tr, L, off, perm, rot + shift)), shift
    # rot alone and rot = 0 through the rotating kernel
    assert np.array_equal(base[3:5], _shuffle(d, tr, L, off, None, rot[3:5]))
    assert np.array_equal(base[:3], _shuffle(d, tr, L, off, perm[:3], np.zeros_like(rot[:3])))


# ----------------------------------------------------------------------------- 4. dynamics matrix, scale
@pytest.mark.parametrize("L,band", [(250, 7), (61, 3)], ids=lambda v: str(v))
def test_one_way_dynamics_and_likelihood_scale(L, band):
    d, tr, off, perm, rot, ref = SH.shuffle_reference(L, band, pmj=0.0, pjm=0.3)
    assert tr.A[0, 1] == 0
    lz = _shuffle(d, tr, L, off, perm, rot)
    print(f"L={L} one-way A: worst ratio {_worst(lz, ref):.3f}")
    assert np.all(np.abs(lz - ref) <= BAR * np.abs(ref))
    d, tr, off, perm, rot, ref = SH.shuffle_reference(L, band, likelihood_scale=0.37)
    lz = _shuffle(d, tr, L, off, perm, rot, likelihood_scale=0.37)
    print(f"L={L} likelihood_scale 0.37: worst ratio {_worst(lz, ref):.3f}")
    assert np.all(np.abs(lz - ref) <= BAR * np.abs(ref))


# ----------------------------------------------------------------------------- 5. public API
_API_SEGMENTS = np.array([[395, 400], [10, 40], [0, 1], [200, 233], [41, 49], [100, 117], [300, 302], [60, 64]])


@pytest.mark.parametrize("kind", ["poisson", "gaussian"])
def test_shuffle_test_segments_api(kind):
    from poor_man_gplvm_amd.core import gather_segments, shuffle_p_values
    cls, args, kw, y, tun, _, mn = _api_model(kind)
    seg = _API_SEGMENTS
    m = cls(*args, **kw)
    L, n, S_ = kw['n_latent_bin'], 16, len(seg)
    common = dict(tuning=tun, ma_neuron=mn)
    res = {}
    for how in ('time_bin', 'column_cycle', 'both'):
        r = m.shuffle_test_segments(y, seg, n_shuffle=n, shuffle=how, key=5, **common)
        assert list(r) == ['segment_offsets', 'log_marginal_final', 'log_marginal_shuffle', 'p_value']
        off = r['segment_offsets']
        assert off.dtype == np.int64 and np.array_equal(np.diff(off), seg[:, 1] - seg[:, 0])
        assert r['log_marginal_final'].shape == (S_,) and r['log_marginal_final'].dtype == np.float64
        assert r['log_marginal_shuffle'].shape == (n, S_) and r['log_marginal_shuffle'].dtype == np.float64
        assert r['p_value'].shape == (S_,) and r['p_value'].dtype == np.float64
        assert np.all(np.isfinite(r['log_marginal_shuffle']))
        assert np.array_equal(r['p_value'], shuffle_p_values(r['log_marginal_final'], r['log_marginal_shuffle']))
        assert r['p_value'].min() >= 1 / (n + 1) and r['p_value'].max() <= 1
        # the same key gives the same arrays, another key other shuffles
        r2 = m.shuffle_test_segments(y, seg, n_shuffle=n, shuffle=how, key=5, **common)
        r3 = m.shuffle_test_segments(y, seg, n_shuffle=n, shuffle=how, key=6, **common)
        for k in r:
            assert np.array_equal(r[k], r2[k]), (how, k)
        assert not np.array_equal(r['log_marginal_shuffle'], r3['log_marginal_shuffle'])
        assert np.array_equal(r['log_marginal_final'], r3['log_marginal_final'])
        res[how] = r
    # the true score is decode_latent_segments' (every event here is a one-wave event)
    q = m.decode_latent_segments(y, seg, **common)
    for how in res:
        assert np.array_equal(res[how]['log_marginal_final'], q['log_marginal_final']), how
    # the one-row event under time_bin: every shuffle is the identity
    assert res['time_bin']['p_value'][2] == 1.0
    assert np.all(res['time_bin']['log_marginal_shuffle'][:, 2] == res['time_bin']['log_marginal_final'][2])
    # a tiny batch budget (one generation block per launch) gives the same bits as one batch
    n_big = 3 * m.SHUFFLE_GEN_BLOCK + 5
    for how in ('time_bin', 'both'):
        one = m.shuffle_test_segments(y, seg, n_shuffle=n_big, shuffle=how, key=9, **common)
        small = cls(*args, **kw)
        small.SHUFFLE_BATCH_BYTES = 1
        assert small._shuffle_batch(int(off[-1]), n_big) == m.SHUFFLE_GEN_BLOCK < m._shuffle_batch(int(off[-1]), n_big)
        many = small.shuffle_test_segments(y, seg, n_shuffle=n_big, shuffle=how, key=9, **common)
        for k in one:
            assert np.array_equal(one[k], many[k]), (how, k)
    # caller perm / rot (array or device tensor) reproduce the engine-level values
    Ttot = int(off[-1])
    rng = np.random.default_rng(21)
    perm = np.tile(np.arange(Ttot, dtype=np.int64), (n, 1))
    for r_ in range(n):
        for s in range(S_):
            a, b = int(off[s]), int(off[s + 1])
            perm[r_, a:b] = a + rng.permutation(b - a)
    rot = rng.integers(-L, 2 * L, size=(n, Ttot))
    yc, off2, ma = gather_segments(y, seg, mn)
    eng = m._decode_engine(yc, tun, m._decode_hp({}), ma, m.ma_latent_default, exact=False)
    eng.emission(1.0)
    for p_, q_ in ((perm, None), (None, rot), (perm, rot)):
        want = eng.segment_shuffle_logz(1.0, _i64(off2), None, _i32(p_), _i32(q_)).cpu().numpy()
        got = m.shuffle_test_segments(y, seg, n_shuffle=n, perm=p_, rot=q_, key=1, **common)
        assert np.array_equal(got['log_marginal_shuffle'], want)
        assert np.array_equal(got['log_marginal_final'], q['log_marginal_final'])
        dev = m.shuffle_test_segments(y, seg, n_shuffle=n, perm=None if p_ is None else _i32(p_),
                                      rot=None if q_ is None else torch.as_tensor(q_), key=2, **common)
        for k in got:
            assert np.array_equal(got[k], dev[k]), k
    # list input equals interval input
    rl = m.shuffle_test_segments([y[a:b] for a, b in seg], n_shuffle=n, perm=perm, rot=rot, **common)
    for k in got:
        assert np.array_equal(got[k], rl[k]), k


# ----------------------------------------------------------------------------- 6. planted sequences
def test_planted_sequences_beat_rate_matched_noise():
    """Events sampled from the model itself on a smooth trajectory (no jumps) against events of
    independent Poisson counts at each planted event's own mean rates: the median p of the
    planted events is below the median p of the noise events.  A direction, not a threshold.
    The walk has to cross tuning curves within an event for the order of its rows to matter
    (30 steps of variance 1 stay within one tuning width of 10 bins, and such an event's rows
    are nearly exchangeable): tuning width 3 bins, movement variance 3."""
    import poor_man_gplvm_amd as P
    from tests.synth import make
    N, L, T_ev, n_ev = 30, 100, 30, 6
    tun = make(N, L, 10, ls=3.0)['tuning']
    m = P.PoissonGPLVMJump1D(N, n_latent_bin=L, tuning_lengthscale=3., movement_variance=3.)
    rng = np.random.default_rng(5)
    planted, noise = [], []
    for k in range(n_ev):
        _, yk = m.sample(T_ev, hyperparam={'p_move_to_jump': 0.0, 'p_jump_to_move': 1.0}, key=100 + k,
                         init_dynamics=0, tuning=tun)
        yk = np.asarray(yk, np.float32)
        planted.append(yk)
        noise.append(rng.poisson(yk.mean(0, keepdims=True), size=yk.shape).astype(np.float32))
    r = m.shuffle_test_segments(planted + noise, n_shuffle=200, shuffle='time_bin', key=0, tuning=tun)
    p = r['p_value']
    print(f"planted p {np.round(p[:n_ev], 3)}, noise p {np.round(p[n_ev:], 3)}")
    assert np.median(p[:n_ev]) < np.median(p[n_ev:])
