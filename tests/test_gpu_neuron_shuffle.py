"""The per-neuron circular spike shuffle on the device: pmg_segment_roll_prepare
(csrc/segment_roll.hip), SpikeData.rolled and shuffle_test_segments(shuffle='neuron_circular').

A. contract 1 at the C-ABI level: yq_out, gconst_out and y_out byte for byte what
   pmg_spikes_prepare writes for the host-rolled rows (tests/neuron_shuffle_ref.roll_segments);
B. rows that no clamped segment owns keep their sentinels;
C. every (shuffle, event) log marginal against the float64 reference at 1e-7 |ref|, the bar
   tests/test_gpu_shuffle_segments.py holds the same filter to.  tests/test_neuron_shuffle_host.py
   shows that a roll which ignores shift, rolls by -k or takes the next neuron's shift moves
   the reference by >= 1e-5 |logZ| in >= 80 % of the eligible pairs, 100 x the bar here;
D. the public call against decode_latent_segments on the host-rolled rows;
E. independence, bit for bit; F. the other options; G. planted sequences (direction only).
No test feeds the kernel an index outside its range.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import neuron_shuffle_ref as NS
from tests import sample_ref as SR
from tests.test_gpu_sample import _api_model

pytestmark = pytest.mark.gpu

BAR = 1e-7
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
A_LENS = (1, 2, 3, 7, 63, 64, 65, 130)


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _dt(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x, dtype), device='cuda')


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _special_shifts(rng, R, lens, N):
    """(R, S, N) int64: random values with 0, len, -1, 2 len + 3 and the int32 extremes planted
    in every segment (where there are neurons enough) and in the first and last neuron."""
    ln = np.asarray(lens, np.int64)[None, :, None]
    sh = rng.integers(-5 * ln, 5 * ln + 1, size=(R, len(lens), N))
    special = [np.zeros_like(ln), ln, -np.ones_like(ln), 2 * ln + 3, np.full_like(ln, I32_MIN),
               np.full_like(ln, I32_MAX)]
    for j, v in enumerate(special):
        for r in range(R):
            if N >= len(special):       # neuron (j + r) of every segment
                sh[r, :, (j + r) % N] = v[0, :, 0]
            else:                       # few neurons: neuron 0 of every sixth segment
                for s in range((j + r) % len(special), len(lens), len(special)):
                    sh[r, s, 0] = v[0, s, 0]
    if N >= len(special):
        sh[0, :, N - 1] = I32_MIN
    return sh


def _roll_call(src, off, shift, T, with_y, from_y, sentinel=False):
    """One pmg_segment_roll_prepare call through ctypes.  Returns host (yq_out, gconst_out, y_out)."""
    from poor_man_gplvm_amd import _native as nat
    R, S = int(shift.shape[0]), len(off) - 1
    Tp = -(-R * T // 64) * 64
    yq_o = torch.full((Tp, src.Kp), 0x55, dtype=torch.int8, device='cuda')
    gc_o = torch.full((R * T,), -7.25, dtype=torch.float64, device='cuda')
    y_o = torch.full((R * T, src.N), -3.5, dtype=torch.float32, device='cuda') if with_y else None
    off_d, shift_d = _dt(off, np.int64), _dt(shift, np.int32)      # both alive until the call is done
    nat.check(nat.load().pmg_segment_roll_prepare(nat.ptr(src.y if (from_y or with_y) else None), nat.ptr(src.yq),
                                                  nat.ptr(src.ma), T, src.N, src.Kp, nat.ptr(off_d), S,
                                                  nat.ptr(shift_d), R, nat.ptr(y_o), nat.ptr(yq_o),
                                                  nat.ptr(gc_o), nat.stream_handle()), "pmg_segment_roll_prepare")
    torch.cuda.synchronize()
    return yq_o.cpu().numpy(), gc_o.cpu().numpy(), None if y_o is None else y_o.cpu().numpy()


def _want(y, ma, off, shift_r):
    """What pmg_spikes_prepare writes for the host-rolled rows: (yq (T, Kp), gconst (T,), y)."""
    from poor_man_gplvm_amd.engine import SpikeData
    yr = NS.roll_segments(y, off, shift_r)
    sp = SpikeData(yr, ma)
    T = y.shape[0]
    return sp.yq[:T].cpu().numpy(), sp.gconst.cpu().numpy(), yr


# ----------------------------------------------------------------------------- A. contract 1
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("N", [1, 5, 64, 132, 260])
def test_outputs_are_spikes_prepare_of_the_host_rolled_rows(N, R):
    from poor_man_gplvm_amd.engine import SpikeData
    rng = np.random.default_rng(100 * N + R)
    off = _offsets(A_LENS)
    T = int(off[-1])
    y = rng.poisson(2.0, size=(T, N)).astype(np.float32)
    y[rng.random((T, N)) < 0.05] = 127.0
    y[rng.random((T, N)) < 0.05] = 126.0
    ma = (rng.random(N) > 0.3).astype(np.float32)
    if N > 1:
        ma[0], ma[N - 1] = 0.0, 1.0
    shift = _special_shifts(rng, R, A_LENS, N)
    src = SpikeData(y, ma)
    assert src.int_path and src.Kp > N
    want = [_want(y, ma, off, shift[r]) for r in range(R)]
    for with_y, from_y in ((True, True), (False, True), (False, False)):    # the last: the int8 values alone
        yq_o, gc_o, y_o = _roll_call(src, off, shift, T, with_y, from_y)
        for r in range(R):
            wq, wg, wy = want[r]
            assert np.array_equal(yq_o[r * T:(r + 1) * T], wq), (with_y, from_y, r)       # columns N .. Kp-1 too
            assert np.array_equal(gc_o[r * T:(r + 1) * T].view(np.int64), wg.view(np.int64)), (with_y, from_y, r)
            if with_y:
                assert np.array_equal(y_o[r * T:(r + 1) * T].view(np.int32), wy.view(np.int32)), r
        assert not yq_o[R * T:].any()                                                     # the padding rows
        assert not yq_o[:, N:].any()
    assert (R * T) % 64 != 0


def test_non_integer_counts_take_the_f32_path():
    from poor_man_gplvm_amd.engine import SpikeData
    rng = np.random.default_rng(9)
    N, R = 20, 2
    off = _offsets(A_LENS)
    T = int(off[-1])
    y = (rng.gamma(1.0, 2.0, size=(T, N)) * (rng.random((T, N)) < 0.7)).astype(np.float32)
    y[3, 2], y[70, 5] = 200.0, 1e4        # beyond the lgamma table
    ma = (rng.random(N) > 0.3).astype(np.float32)
    shift = _special_shifts(rng, R, A_LENS, N)
    src = SpikeData(y, ma)
    assert not src.int_path
    yq_o, gc_o, y_o = _roll_call(src, off, shift, T, True, True)
    for r in range(R):
        wq, wg, wy = _want(y, ma, off, shift[r])
        assert np.array_equal(yq_o[r * T:(r + 1) * T], wq)
        assert np.array_equal(gc_o[r * T:(r + 1) * T].view(np.int64), wg.view(np.int64))
        assert np.array_equal(y_o[r * T:(r + 1) * T].view(np.int32), wy.view(np.int32))
    # SpikeData.rolled makes the same buffers, y among them off the integer path
    sp = SpikeData.rolled(src, _dt(off, np.int64), _dt(shift, np.int32))
    assert sp.T == R * T and sp.y is not None and sp.yext is None and sp.ybt is None and not sp.int_path
    assert np.array_equal(sp.yq.cpu().numpy(), yq_o) and np.array_equal(sp.y.cpu().numpy(), y_o)
    assert np.array_equal(sp.gconst.cpu().numpy().view(np.int64), gc_o.view(np.int64))


# ----------------------------------------------------------------------------- B. sentinels
@pytest.mark.parametrize("off", [(2, 5, 5, 12, 26), (-7, 5, 5, 12, 64), (30, 30), (40, 50, 60)],
                         ids=["gapped", "clamped", "empty", "beyond"])
def test_rows_no_segment_owns_keep_their_sentinels(off):
    from poor_man_gplvm_amd.engine import SpikeData
    rng = np.random.default_rng(4)
    T, N, R = 30, 8, 2
    off = np.asarray(off, np.int64)
    S = len(off) - 1
    y = rng.poisson(1.5, size=(T, N)).astype(np.float32)
    shift = rng.integers(-50, 50, size=(R, S, N))
    src = SpikeData(y, None)
    yq_o, gc_o, y_o = _roll_call(src, off, shift, T, True, True)
    a = np.clip(off[:-1], 0, T)
    b = np.clip(np.maximum(off[1:], a), 0, T)
    owned = np.zeros(T, bool)
    for s in range(S):
        owned[a[s]:b[s]] = True
    for r in range(R):
        yr = y.copy()
        for s in range(S):       # each clamped segment rolled on its own
            yr = NS.roll_segments(yr, np.array([a[s], b[s]]), shift[r, s:s + 1])
        sp = SpikeData(yr, None)
        rows = slice(r * T, (r + 1) * T)
        assert np.array_equal(yq_o[rows][owned], sp.yq[:T].cpu().numpy()[owned])
        assert np.array_equal(gc_o[rows][owned].view(np.int64), sp.gconst.cpu().numpy()[owned].view(np.int64))
        assert np.array_equal(y_o[rows][owned], yr[owned])
        assert np.all(yq_o[rows][~owned] == 0x55) and np.all(gc_o[rows][~owned] == -7.25)
        assert np.all(y_o[rows][~owned] == -3.5)
    assert not yq_o[R * T:].any()


# ----------------------------------------------------------------------------- C. the float64 reference
def _stacked_logz(d, tr, L, off, shift, likelihood_scale=1.0):
    from poor_man_gplvm_amd.core import segment_order
    from poor_man_gplvm_amd.engine import DeviceEM, SpikeData
    R, S, T = shift.shape[0], len(off) - 1, int(off[-1])
    src = SpikeData(np.ascontiguousarray(d['y']))
    assert src.int_path
    sp = SpikeData.rolled(src, _dt(off, np.int64), _dt(shift, np.int32))
    assert sp.y is None and sp.yext is None and sp.T == R * T
    eng = DeviceEM(sp, L, basis=d['B'])
    eng.set_transition(tr)
    eng.set_ma_latent(None)
    eng.set_tuning(d['tuning'])
    eng.emission(likelihood_scale)
    so = np.concatenate([(np.arange(R)[:, None] * T + off[None, :-1]).reshape(-1), [R * T]]).astype(np.int64)
    lz = eng.segment_shuffle_logz(likelihood_scale, _dt(so, np.int64), _dt(segment_order(so), np.int32))
    eng.emission_status()
    eng.check_status()
    return lz.cpu().numpy().reshape(R, S)


@pytest.mark.parametrize("case", SR.CASES, ids=lambda c: f"L{c[0]}-band{c[1]}")
def test_every_pair_against_the_reference(case):
    L, band = case
    d, tr, off, sh, ref = NS.neuron_shuffle_reference(L, band)
    lz = _stacked_logz(d, tr, L, off, sh)
    assert lz.shape == ref.shape == (NS.N_SHUFFLE, len(NS.LENS))
    worst = float(np.max(np.abs(lz - ref) / (BAR * np.abs(ref))))
    print(f"L{L}-band{band}: worst |logz - ref| / (1e-7 |ref|) = {worst:.3f}")
    assert np.all(np.abs(lz - ref) <= BAR * np.abs(ref))
    assert np.array_equal(lz[0], lz[1])          # shift = len is the identity


# ----------------------------------------------------------------------------- D. the public call
_SEG = np.array([[395, 400], [10, 40], [0, 1], [200, 233], [41, 49], [100, 117], [300, 302], [60, 64]])


def _api_shift(rng, n, seg, N):
    ln = (seg[:, 1] - seg[:, 0])[None, :, None]
    return rng.integers(-3 * ln, 3 * ln + 1, size=(n, len(seg), N))


@pytest.mark.parametrize("kind", ["poisson", "gaussian"])
def test_public_call_equals_decode_of_the_host_rolled_rows(kind):
    from poor_man_gplvm_amd.core import shuffle_p_values
    cls, args, kw, y, tun, _, mn = _api_model(kind)
    m = cls(*args, **kw)
    seg, n = _SEG, 3
    common = dict(tuning=tun, ma_neuron=mn)
    shift = _api_shift(np.random.default_rng(31), n, seg, y.shape[1])
    r = m.shuffle_test_segments(y, seg, n_shuffle=n, shift=shift, **common)
    assert list(r) == ['segment_offsets', 'log_marginal_final', 'log_marginal_shuffle', 'p_value']
    off = r['segment_offsets']
    assert r['log_marginal_shuffle'].shape == (n, len(seg)) and r['log_marginal_shuffle'].dtype == np.float64
    assert np.array_equal(r['p_value'], shuffle_p_values(r['log_marginal_final'], r['log_marginal_shuffle']))
    parts = [y[a:b] for a, b in seg]
    yc = np.concatenate(parts)
    true = m.decode_latent_segments(y, seg, **common)['log_marginal_final']
    worst = 0.0
    for k in range(n):
        yr = NS.roll_segments(yc, off, shift[k])
        want = m.decode_latent_segments([yr[off[s]:off[s + 1]] for s in range(len(seg))], **common)
        want = want['log_marginal_final']
        if kind == 'poisson':       # the integer emission is exact: a row's value cannot depend on its place
            assert np.array_equal(r['log_marginal_shuffle'][k], want), k
        worst = max(worst, float(np.max(np.abs(r['log_marginal_shuffle'][k] - want) / np.abs(want))))
        assert np.all(np.abs(r['log_marginal_shuffle'][k] - want) <= BAR * np.abs(want)), k
    if kind == 'poisson':
        assert np.array_equal(r['log_marginal_final'], true)
    worst = max(worst, float(np.max(np.abs(r['log_marginal_final'] - true) / np.abs(true))))
    print(f"{kind}: largest relative difference from the host-rolled decode {worst:.3e}")
    assert np.all(np.abs(r['log_marginal_final'] - true) <= BAR * np.abs(true))
    # a device tensor and shuffle='neuron_circular' alongside shift give the same arrays
    r2 = m.shuffle_test_segments(y, seg, n_shuffle=n, shuffle='neuron_circular',
                                 shift=torch.as_tensor(shift, device='cuda'), **common)
    rl = m.shuffle_test_segments(parts, n_shuffle=n, shift=shift.astype(np.int32), **common)
    for k in r:
        assert np.array_equal(r[k], r2[k]) and np.array_equal(r[k], rl[k]), k


# ----------------------------------------------------------------------------- E. independence
def test_values_are_exact_functions_of_their_own_event_and_shifts():
    cls, args, kw, y, tun, _, mn = _api_model('poisson')
    m = cls(*args, **kw)
    seg, n = _SEG, 8
    S_, N = len(seg), y.shape[1]
    common = dict(tuning=tun, ma_neuron=mn)
    shift = _api_shift(np.random.default_rng(32), n, seg, N)
    base = m.shuffle_test_segments(y, seg, n_shuffle=n, shift=shift, **common)
    lz, true = base['log_marginal_shuffle'], base['log_marginal_final']
    for s in range(S_):         # one event alone
        one = m.shuffle_test_segments(y, seg[s:s + 1], n_shuffle=n, shift=shift[:, s:s + 1], **common)
        assert np.array_equal(one['log_marginal_shuffle'][:, 0], lz[:, s]), s
        assert one['log_marginal_final'][0] == true[s]
    rev = m.shuffle_test_segments(y, seg[::-1], n_shuffle=n, shift=shift[:, ::-1], **common)
    assert np.array_equal(rev['log_marginal_shuffle'][:, ::-1], lz)
    assert np.array_equal(rev['log_marginal_final'][::-1], true)
    first = m.shuffle_test_segments(y, seg, n_shuffle=1, shift=shift[:1], **common)
    assert np.array_equal(first['log_marginal_shuffle'][0], lz[0]) and np.array_equal(first['log_marginal_final'], true)
    ln = (seg[:, 1] - seg[:, 0])[None, :, None]
    for k in (1, -1, 4, -7):    # shift is reduced mod len on the device
        moved = m.shuffle_test_segments(y, seg, n_shuffle=n, shift=shift + k * ln, **common)
        assert np.array_equal(moved['log_marginal_shuffle'], lz), k
    # generated shifts: one generation block per launch against one launch; keys
    n_big = 3 * m.SHUFFLE_NEURON_GEN_BLOCK + 5
    one = m.shuffle_test_segments(y, seg, n_shuffle=n_big, shuffle='neuron_circular', key=9, **common)
    small = cls(*args, **kw)
    small.SHUFFLE_NEURON_BATCH_BYTES = 1
    Ttot = int(base['segment_offsets'][-1])
    assert (small._shuffle_neuron_batch(Ttot, S_, N, n_big, False) == m.SHUFFLE_NEURON_GEN_BLOCK
            < m._shuffle_neuron_batch(Ttot, S_, N, n_big, False))
    many = small.shuffle_test_segments(y, seg, n_shuffle=n_big, shuffle='neuron_circular', key=9, **common)
    again = m.shuffle_test_segments(y, seg, n_shuffle=n_big, shuffle='neuron_circular', key=9, **common)
    other = m.shuffle_test_segments(y, seg, n_shuffle=n_big, shuffle='neuron_circular', key=10, **common)
    for k in one:
        assert np.array_equal(one[k], many[k]) and np.array_equal(one[k], again[k]), k
    assert not np.array_equal(one['log_marginal_shuffle'], other['log_marginal_shuffle'])
    assert np.array_equal(one['log_marginal_final'], other['log_marginal_final'])
    assert np.array_equal(one['log_marginal_final'], true)
    assert np.all(np.isfinite(one['log_marginal_shuffle']))
    # the one-row event cannot move: every shuffle ties with the true score
    assert one['p_value'][2] == 1.0 and np.all(one['log_marginal_shuffle'][:, 2] == true[2])
    # the existing kinds are untouched by the new arguments' defaults
    tb = m.shuffle_test_segments(y, seg, n_shuffle=4, shuffle='time_bin', key=5, **common)
    assert np.array_equal(tb['log_marginal_final'], true)


# ----------------------------------------------------------------------------- F. other options
def test_latent_mask_likelihood_scale_and_min_shift():
    from poor_man_gplvm_amd.core import segment_neuron_shifts
    cls, args, kw, y, tun, ml, mn = _api_model('poisson')
    m = cls(*args, **kw)
    seg, n = _SEG, 3
    N = y.shape[1]
    shift = _api_shift(np.random.default_rng(33), n, seg, N)
    yc = np.concatenate([y[a:b] for a, b in seg])
    for opts in (dict(ma_latent=ml), dict(likelihood_scale=0.37), dict(ma_latent=ml, likelihood_scale=0.37)):
        common = dict(tuning=tun, ma_neuron=mn, **opts)
        r = m.shuffle_test_segments(y, seg, n_shuffle=n, shift=shift, **common)
        off = r['segment_offsets']
        assert np.array_equal(r['log_marginal_final'], m.decode_latent_segments(y, seg, **common)['log_marginal_final'])
        for k in range(n):
            yr = NS.roll_segments(yc, off, shift[k])
            want = m.decode_latent_segments([yr[off[s]:off[s + 1]] for s in range(len(seg))], **common)
            assert np.array_equal(r['log_marginal_shuffle'][k], want['log_marginal_final']), (list(opts), k)
    # min_shift = 5 on events on both sides of 10 rows: the generated shuffles are those of the
    # same draws passed in as the caller's own
    common = dict(tuning=tun, ma_neuron=mn)
    n_gen, g = 11, m.SHUFFLE_NEURON_GEN_BLOCK
    r = m.shuffle_test_segments(y, seg, n_shuffle=n_gen, shuffle='neuron_circular', key=3, min_shift=5, **common)
    off = r['segment_offsets']
    gen = torch.Generator(device='cuda')
    gen.manual_seed(3)
    sh = torch.cat([segment_neuron_shifts(off, min(g, n_gen - b0), N, 5, gen, 'cuda') for b0 in range(0, n_gen, g)])
    assert sh.dtype == torch.int32 and tuple(sh.shape) == (n_gen, len(seg), N)
    s = sh.cpu().numpy()
    for k, ln in enumerate(seg[:, 1] - seg[:, 0]):
        lo = 5 if ln > 10 else 0
        assert s[:, k].min() >= lo and s[:, k].max() <= ln - lo - 1, (k, ln)
    own = m.shuffle_test_segments(y, seg, n_shuffle=n_gen, shift=sh, **common)
    for k in r:
        assert np.array_equal(r[k], own[k]), k
    r0 = m.shuffle_test_segments(y, seg, n_shuffle=n_gen, shuffle='neuron_circular', key=3, **common)
    assert not np.array_equal(r0['log_marginal_shuffle'], r['log_marginal_shuffle'])


# ----------------------------------------------------------------------------- G. planted sequences
def test_planted_sequences_beat_rate_matched_noise():
    """The events of tests/test_gpu_shuffle_segments.py's direction test (a smooth walk across
    narrow tuning curves against independent Poisson counts at each event's own mean rates)
    under the per-neuron circular shuffle: the median p of the planted events is below the
    median p of the noise events.  A direction, not a threshold."""
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
    r = m.shuffle_test_segments(planted + noise, n_shuffle=200, shuffle='neuron_circular', key=0, tuning=tun)
    p = r['p_value']
    print(f"planted p {np.round(p[:n_ev], 3)}, noise p {np.round(p[n_ev:], 3)}")
    assert np.median(p[:n_ev]) < np.median(p[n_ev:])
