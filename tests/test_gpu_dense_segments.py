"""The dense segment smoother (pmg_dense_segment_smoother: one 256-thread workgroup per
segment, csrc/dense_scan.hip) and decode_latent_segments(exact=True) on the GPU.

Inputs and the per-segment float64 reference: tests/dense_segments_ref.py (a shifted,
asymmetric custom kernel; tests/test_dense_segments_host.py shows that a transposed kernel
or a chain run across the event boundaries moves every event by >= 1e-4).  Bars, all from
tests/test_gpu_dense.py: close_prob (rtol 1e-5, atol 1e-12) on gamma, alpha and P;
|logz - ref| <= 1e-7 |ref| per event; logc at rtol 1e-6, atol 1e-5; log_gamma at atol 2e-4
where the reference is > -60 and finite wherever the reference is finite.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import gplvm_oracle as O
from tests import dense_segments_ref as R
from tests.test_gpu_parity import argmax_match, close_prob

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
OUT_KEYS = ('alpha', 'log_alpha', 'gamma', 'log_gamma', 'P', 'logc')


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _make_engine(y, tuning, K, L):
    from poor_man_gplvm_amd.engine import DeviceEM, ScanConfig, SpikeData
    from poor_man_gplvm_amd.gp_kernel import dense_transition
    eng = DeviceEM(SpikeData(np.array(y, np.float32), None), L, scan=ScanConfig())
    eng.set_transition(dense_transition(L, 1.0, 0.01, 0.01, K))
    eng.set_tuning(tuning)
    eng.emission(1.0)
    return eng


@functools.lru_cache(maxsize=None)
def _engine(L, lens=R.LENS):
    """A dense engine over the batch's rows with its emission done (shared: the tests below
    call the entry point with output buffers of their own)."""
    d, K, off = R.inputs(L, lens)
    return _make_engine(d['y'], d['tuning'], K, L), off


def _dev_t(a, dtype):
    return torch.as_tensor(np.asarray(a, dtype), device='cuda')


def _outputs(T, L, smooth=True):
    f32, f64 = torch.float32, torch.float64
    o = dict(alpha=torch.full((T, 2, L), SENTINEL, dtype=f32, device='cuda'),
             log_alpha=torch.full((T, 2, L), SENTINEL, dtype=f64, device='cuda'),
             logc=torch.full((T,), SENTINEL, dtype=f64, device='cuda'))
    if smooth:
        o.update(gamma=torch.full((T, 2, L), SENTINEL, dtype=f32, device='cuda'),
                 log_gamma=torch.full((T, 2, L), SENTINEL, dtype=f32, device='cuda'),
                 P=torch.full((T, L), SENTINEL, dtype=f32, device='cuda'))
    return o


def _call(eng, seg_off, order=None, smooth=True, ll64=True, scale=1.0):
    """pmg_dense_segment_smoother on all of eng's rows into sentinel-filled buffers."""
    from poor_man_gplvm_amd import _native as nat
    T, L = eng.T, eng.L
    S = len(seg_off) - 1
    o = _outputs(T, L, smooth)
    o['logz'] = torch.full((S,), SENTINEL, dtype=torch.float64, device='cuda')
    so = _dev_t(seg_off, np.int64)
    od = None if order is None else _dev_t(order, np.int32)
    nat.check(eng.lib.pmg_dense_segment_smoother(
        nat.ptr(eng.delta), nat.ptr(eng.phi), nat.ptr(eng.ll64) if ll64 else None, nat.ptr(eng.mref), T,
        nat.ptr(so), S, nat.ptr(od), ctypes.byref(eng._tr_d), float(scale), nat.ptr(o['alpha']),
        nat.ptr(o['log_alpha']), nat.ptr(o.get('gamma')), nat.ptr(o.get('log_gamma')), nat.ptr(o.get('P')),
        nat.ptr(o['logc']), nat.ptr(o['logz']), nat.stream_handle()), "pmg_dense_segment_smoother")
    torch.cuda.synchronize()
    return o


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b, what=""):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _check(out, ref, off, what=""):
    """The bars of the module docstring; out: numpy arrays over the compact rows."""
    close_prob(out['gamma'], ref['gamma'])
    if 'alpha' in out:
        close_prob(out['alpha'], ref['alpha'])
    if 'P' in out:
        close_prob(out['P'], ref['gamma'].sum(1))
        if out['P'].shape[1] > 1:
            argmax_match(out['P'], ref['gamma'].sum(1))
    lz, rz = np.asarray(out['logz'], np.float64), ref['logz']
    print(f"{what}: max |gamma - ref| {np.abs(out['gamma'] - ref['gamma']).max():.2e}, "
          f"max rel logz {np.max(np.abs(lz - rz) / np.abs(rz)):.2e}")
    assert np.all(np.abs(lz - rz) <= 1e-7 * np.abs(rz)), (what, lz, rz)
    np.testing.assert_allclose(out['logc'], ref['logc'], rtol=1e-6, atol=1e-5)
    lg, rg = np.asarray(out['log_gamma'], np.float64), ref['log_gamma']
    fin = np.isfinite(rg)
    assert np.all(np.isfinite(lg[fin])), what
    keep = rg > -60
    np.testing.assert_allclose(lg[keep], rg[keep], atol=2e-4)


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


# ----------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("L", R.FULL_L)
def test_full_batch_vs_float64(L):
    """Through the engine's call site (DeviceEM.segment_smoother_dense), longest first."""
    from poor_man_gplvm_amd.core import segment_order
    eng, off = _engine(L)
    T = eng.T
    o = _outputs(T, L)
    la, logc, logz = eng.segment_smoother_dense(1.0, _dev_t(off, np.int64), _dev_t(segment_order(off), np.int32),
                                                gamma=o['gamma'], log_gamma=o['log_gamma'], P=o['P'])
    assert la.data_ptr() == eng.log_alpha.data_ptr() and la.dtype == torch.float64 and logz.shape == (len(off) - 1,)
    out = _np(dict(gamma=o['gamma'], log_gamma=o['log_gamma'], P=o['P'], alpha=eng.alpha, logc=logc, logz=logz))
    _check(out, R.reference(L), off, f"L={L}")
    close_prob(np.exp(la.cpu().numpy()), R.reference(L)['alpha'])


@pytest.mark.parametrize("L", R.SHORT_L)
def test_short_batch_vs_float64(L):
    eng, off = _engine(L, R.SHORT)
    _check(_np(_call(eng, off)), R.reference(L, R.SHORT), off, f"L={L}")


def test_likelihood_scale_vs_float64():
    eng, off = _engine(61)
    eng.emission(0.37)                     # the row reference depends on the scale
    try:
        out = _np(_call(eng, off, scale=0.37))
    finally:
        eng.emission(1.0)
    _check(out, R.reference(61, R.LENS, 0.37), off, "scale 0.37")


# ----------------------------------------------------------------------------- 2. contract 1
@pytest.mark.parametrize("with_ll64", [True, False])
@pytest.mark.parametrize("L", R.BITWISE_L)
def test_bit_identical_to_the_chunk_parallel_scans_per_segment(L, with_ll64):
    """Every output equals pmg_dense_forward + pmg_dense_backward on the segment's rows alone
    with chunk = len, warmup = 0 (one chunk: nothing to warm up or repair), bit for bit."""
    from poor_man_gplvm_amd import _native as nat
    eng, off = _engine(L)
    lib = eng.lib
    got = _call(eng, off, ll64=with_ll64)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        n = b - a
        o = _outputs(n, L)
        lz = torch.full((1,), SENTINEL, dtype=torch.float64, device='cuda')
        ws = torch.zeros(int(lib.pmg_dense_workspace_size(n, L, n)), dtype=torch.uint8, device='cuda')
        ll = nat.ptr(eng.ll64[a:b]) if with_ll64 else None
        nat.check(lib.pmg_dense_forward(nat.ptr(eng.delta[a:b]), nat.ptr(eng.phi[a:b]), ll, nat.ptr(eng.mref[a:b]), n,
                                        ctypes.byref(eng._tr_d), 1.0, n, 0, 3e-6, nat.ptr(o['alpha']),
                                        nat.ptr(o['log_alpha']), nat.ptr(o['logc']), nat.ptr(lz), nat.ptr(ws),
                                        ws.numel(), nat.stream_handle()), "pmg_dense_forward")
        nat.check(lib.pmg_dense_backward(nat.ptr(eng.delta[a:b]), nat.ptr(eng.phi[a:b]), ll, nat.ptr(o['log_alpha']),
                                         n, ctypes.byref(eng._tr_d), 1.0, n, 0, 3e-6, nat.ptr(o['P']),
                                         nat.ptr(o['gamma']), nat.ptr(o['log_gamma']), None, None, nat.ptr(ws),
                                         ws.numel(), nat.stream_handle()), "pmg_dense_backward")
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            _same(got[k][a:b], o[k], (L, s, k))
        _same(got['logz'][s:s + 1], lz, (L, s, 'logz'))


# ----------------------------------------------------------------------------- 3. contract 2
def _same_rows(x, y, a, b, a2=None, keys=OUT_KEYS, what=""):
    a2 = a if a2 is None else a2
    for k in keys:
        _same(x[k][a:b], y[k][a2:a2 + (b - a)], (what, k, a, b))


@pytest.mark.parametrize("L", [61, 300])
def test_segments_are_independent_bit_for_bit(L):
    from poor_man_gplvm_amd.core import segment_order
    eng, off = _engine(L)
    S, T = len(off) - 1, eng.T
    base = _call(eng, off)
    for k in OUT_KEYS + ('logz',):
        assert not torch.any(base[k] == SENTINEL), k            # every row is owned
    # the scheduling order changes no value
    first = segment_order(off)
    assert np.array_equal(np.diff(off)[first[:2]], [33, 17])
    for order in (first, first[::-1].copy(), np.arange(S, dtype=np.int32)[::-1].copy()):
        o = _call(eng, off, order=order)
        _same_rows(o, base, 0, T, what="order")
        _same(o['logz'], base['logz'], "order logz")
    # an order entry outside 0 .. S-1 is skipped: its workgroup writes nothing
    bad = first.copy()
    bad[3], bad[5] = S, -1
    o = _call(eng, off, order=bad)
    for s in range(S):
        a, b = int(off[s]), int(off[s + 1])
        if s in (first[3], first[5]):
            for k in OUT_KEYS:
                assert torch.all(o[k][a:b] == SENTINEL), (k, s)
            assert o['logz'][s] == SENTINEL
        else:
            _same_rows(o, base, a, b, what="skipped")
            _same(o['logz'][s:s + 1], base['logz'][s:s + 1])
    # one event alone (the longest, a one-row one, the last)
    for s in (10, 0, S - 1):
        a, b = int(off[s]), int(off[s + 1])
        o = _call(eng, [a, b])
        _same_rows(o, base, a, b, what="alone")
        _same(o['logz'], base['logz'][s:s + 1], "alone logz")
        for k in OUT_KEYS:
            assert torch.all(o[k][:a] == SENTINEL) and torch.all(o[k][b:] == SENTINEL), k
    # forward only: the filter outputs of the full call, nothing else
    o = _call(eng, off, smooth=False)
    _same_rows(o, base, 0, T, keys=('alpha', 'log_alpha', 'logc'), what="forward only")
    _same(o['logz'], base['logz'], "forward only logz")
    # the batch reversed: every event keeps its values at its new rows
    d, K, _ = R.inputs(L)
    lens = np.diff(off)[::-1]
    roff = R.offsets(tuple(int(x) for x in lens))
    idx = np.concatenate([np.arange(off[s], off[s + 1]) for s in range(S - 1, -1, -1)])
    reng = _make_engine(d['y'][idx], d['tuning'], K, L)
    ro = _call(reng, roff)
    for s in range(S):
        a, b = int(off[s]), int(off[s + 1])
        _same_rows(base, ro, a, b, a2=int(roff[S - 1 - s]), what="reversed")
        _same(ro['logz'][S - 1 - s:S - s], base['logz'][s:s + 1], "reversed logz")


def test_unowned_rows_are_not_written():
    """A seg_off with rows no segment owns, one clamped at both ends, and an empty segment:
    the sentinels survive outside the clamped segments, the empty one only gets logz = 0."""
    L = 61
    eng, _ = _engine(L)
    T = eng.T
    assert T == 120
    for seg_off, owned in (([5, 20, 20, 50], [(5, 20), (20, 20), (20, 50)]),
                           ([100, 110, 500], [(100, 110), (110, 120)]),
                           ([-4, 6, 6], [(0, 6), (6, 6)]),
                           ([130, 140], [(120, 120)])):
        o = _call(eng, seg_off)
        mask = np.zeros(T, bool)
        for s, (a, b) in enumerate(owned):
            mask[a:b] = True
            if a == b:
                assert float(o['logz'][s]) == 0.0
                continue
            one = _call(eng, [a, b])
            _same_rows(o, one, a, b, what=str(seg_off))
            _same(o['logz'][s:s + 1], one['logz'], "logz")
        free = torch.as_tensor(~mask, device='cuda')
        for k in OUT_KEYS:
            assert torch.all(o[k][free] == SENTINEL), (seg_off, k)
            assert not torch.any(o[k][~free] == SENTINEL), (seg_off, k)


# ----------------------------------------------------------------------------- 4. public API
JUMP_KEYS = ['segment_offsets', 'posterior_all', 'posterior_latent_marg', 'posterior_dynamics_marg',
             'log_causal_posterior_all', 'log_one_step_predictive_marginals_all', 'log_likelihood_all',
             'log_marginal_final', 'log_posterior_all']
LATENT_KEYS = ['segment_offsets', 'posterior_all', 'log_posterior_all', 'log_causal_posterior_all',
               'log_one_step_predictive_marginals_all', 'log_likelihood_all', 'log_marginal_final']


def _segments(off):
    return np.stack([off[:-1], off[1:]], 1)


def _check_jump(r, ref, off, L, what="", keep=None):
    """A jump model's exact=True result against a reference over the compact rows."""
    Ttot, S = int(off[-1]), len(off) - 1
    assert list(r) == JUMP_KEYS
    np.testing.assert_array_equal(r['segment_offsets'], off)
    assert r['segment_offsets'].dtype == np.int64 and r['log_marginal_final'].dtype == np.float64
    for k, shape in (('posterior_all', (Ttot, 2, L)), ('posterior_latent_marg', (Ttot, L)),
                     ('posterior_dynamics_marg', (Ttot, 2)), ('log_causal_posterior_all', (Ttot, 2, L)),
                     ('log_posterior_all', (Ttot, 2, L)), ('log_one_step_predictive_marginals_all', (Ttot,)),
                     ('log_likelihood_all', (Ttot, L)), ('log_marginal_final', (S,))):
        assert r[k].shape == shape, k
    keep = np.ones(L, bool) if keep is None else keep
    out = dict(gamma=r['posterior_all'][:, :, keep], P=r['posterior_latent_marg'][:, keep],
               alpha=np.exp(r['log_causal_posterior_all'][:, :, keep].astype(np.float64)),
               log_gamma=r['log_posterior_all'][:, :, keep], logc=r['log_one_step_predictive_marginals_all'],
               logz=r['log_marginal_final'])
    ref = dict(ref, gamma=ref['gamma'][:, :, keep], alpha=ref['alpha'][:, :, keep],
               log_gamma=ref['log_gamma'][:, :, keep])
    _check(out, ref, off, what)
    close_prob(r['posterior_dynamics_marg'], ref['gamma'].sum(2))
    if not keep.all():                  # masked latents carry the reference's -1e20, not log(0)
        for k in ('log_posterior_all', 'log_causal_posterior_all'):
            assert np.all(r[k][:, :, ~keep] == np.float32(-1e20)), k


def _oracle_segments(y, tuning, off, logK, logA, ma_neuron=None, **kw):
    """Every segment on its own through the oracle (R.oracle_segment), over the compact rows."""
    return R._pack([R.oracle_segment(y[a:b], tuning, logK, logA,
                                     ma_neuron=ma_neuron[a:b] if np.ndim(ma_neuron) == 2 else ma_neuron, **kw)
                    for a, b in zip(off[:-1], off[1:])], off)


def test_public_custom_kernel_vs_oracle():
    import poor_man_gplvm_amd as P
    L = 80
    d, K, off = R.inputs(L)
    m = P.PoissonGPLVMJump1D(R.N_NEURON, n_latent_bin=L, tuning_lengthscale=10., custom_transition_kernel=K)
    r = m.decode_latent_segments(d['y'], _segments(off), tuning=d['tuning'], exact=True)
    _check_jump(r, R.reference(L), off, L, "custom kernel")
    rl = m.decode_latent_segments([d['y'][a:b] for a, b in _segments(off)], tuning=d['tuning'], exact=True)
    for k in r:                         # list-of-arrays input: the same call
        assert np.array_equal(r[k], rl[k], equal_nan=True), k


def test_public_wide_movement_variance_vs_oracle():
    """movement_variance = 5 at L = 128 needs a 42-bin band: exact=False refuses it."""
    import poor_man_gplvm_amd as P
    L, N = 128, R.N_NEURON
    off = R.offsets()
    d = R.make(N, L, int(off[-1]), mv=5.0)
    m = P.PoissonGPLVMJump1D(N, n_latent_bin=L, tuning_lengthscale=10., movement_variance=5.0)
    with pytest.raises(NotImplementedError, match="band"):
        m.decode_latent_segments(d['y'], _segments(off), tuning=d['tuning'])
    r = m.decode_latent_segments(d['y'], _segments(off), tuning=d['tuning'], exact=True)
    _, logK, _, logA = O.create_transition_prob_1d(L, 5.0, 0.01, 0.01)
    _check_jump(r, _oracle_segments(d['y'], d['tuning'], off, logK, logA), off, L, "mv 5")


def test_public_gaussian_custom_kernel_vs_oracle():
    import poor_man_gplvm_amd as P
    L, N = 80, R.N_NEURON
    _, K, off = R.inputs(L)
    T = int(off[-1])
    rng = np.random.default_rng(12)
    tun = rng.normal(size=(L, N)).cumsum(0) * 0.2
    lat = O.sample_latent(T, L, np.random.default_rng(13), 1.0)[:, 1]
    y = (tun[lat] + 0.5 * rng.normal(size=(T, N))).astype(np.float32)
    m = P.GaussianGPLVMJump1D(N, noise_std=0.5, n_latent_bin=L, tuning_lengthscale=10., custom_transition_kernel=K)
    r = m.decode_latent_segments(y, _segments(off), tuning=tun, exact=True)
    _, logK, _, logA = O.create_transition_prob_1d(L, custom_kernel=K)
    _check_jump(r, _oracle_segments(y, tun, off, logK, logA, noise_std=0.5), off, L, "gaussian")


def test_public_masks_scale_and_2d_neuron_mask_vs_oracle():
    import poor_man_gplvm_amd as P
    L, N = 80, R.N_NEURON
    d, K, off = R.inputs(L)
    T = int(off[-1])
    rng = np.random.default_rng(11)
    ml = (rng.random(L) > 0.2).astype(np.float32)
    mn = (rng.random((T, N)) > 0.2).astype(np.float32)
    m = P.PoissonGPLVMJump1D(N, n_latent_bin=L, tuning_lengthscale=10., custom_transition_kernel=K)
    r = m.decode_latent_segments(d['y'], _segments(off), tuning=d['tuning'], ma_neuron=mn, ma_latent=ml,
                                 likelihood_scale=0.37, exact=True)
    _, logK, _, logA = O.create_transition_prob_1d(L, custom_kernel=K)
    ref = _oracle_segments(d['y'], d['tuning'], off, logK, logA, mn, ma_latent=ml, likelihood_scale=0.37)
    _check_jump(r, ref, off, L, "masks", keep=ml.astype(bool))


def _latent_only_bar(ours, exact, mimic32):
    """test_gpu_parity.latent_only_close's bar over the whole batch: max abs error < 1e-5
    and < 10 % of the float32 reference-mimic's own deviation."""
    dev = np.abs(np.asarray(ours, np.float64) - exact).max()
    ref_noise = np.abs(mimic32 - exact).max()
    print(f"latent-only: dev {dev:.2e}, float32 mimic {ref_noise:.2e}")
    assert dev < 1e-5 and dev < 0.1 * ref_noise, (dev, ref_noise)


@pytest.mark.parametrize("gaussian", [False, True])
def test_public_latent_only_vs_oracle(gaussian):
    """PoissonGPLVM1D / GaussianGPLVM1D at L = 100 on data sampled WITH jumps, so the far
    moves (weights like exp(-1000)) are present."""
    import poor_man_gplvm_amd as P
    L, N = 100, R.N_NEURON
    d, seg = R.jump_data(N, L)
    off = R.offsets()
    T, S = int(off[-1]), len(seg)
    _, logK = O.create_transition_prob_latent_1d(L, 1.0)
    if gaussian:
        rng = np.random.default_rng(12)
        tun = rng.normal(size=(L, N)).cumsum(0) * 0.2
        y = (tun[d['latent'][:, 1]] + 0.5 * rng.normal(size=(R.JUMP_T, N))).astype(np.float32)
        m, ns = P.GaussianGPLVM1D(N, noise_std=0.5, n_latent_bin=L, tuning_lengthscale=10.), 0.5
    else:
        tun, y = d['tuning'], d['y']
        m, ns = P.PoissonGPLVM1D(N, n_latent_bin=L, tuning_lengthscale=10.), None
    r = m.decode_latent_segments(y, seg, tuning=tun, exact=True)
    assert list(r) == LATENT_KEYS
    np.testing.assert_array_equal(r['segment_offsets'], off)
    for k, shape in (('posterior_all', (T, L)), ('log_posterior_all', (T, L)), ('log_causal_posterior_all', (T, L)),
                     ('log_one_step_predictive_marginals_all', (T,)), ('log_likelihood_all', (T, L)),
                     ('log_marginal_final', (S,))):
        assert r[k].shape == shape, k
    exact, mimic, causal = [], [], []
    for s, (a, b) in enumerate(seg):
        lpa, lz, lca, cs, _, _ = O.smooth_latent_only(y[a:b], tun, logK, noise_std=ns)
        with O.working_precision(np.float32), np.errstate(over='ignore'):
            m32 = O.smooth_latent_only(np.asarray(y[a:b], np.float32), np.asarray(tun, np.float32),
                                       np.asarray(logK, np.float32), noise_std=ns)[0]
        exact.append(np.exp(lpa))
        causal.append(np.exp(lca))
        mimic.append(np.exp(m32.astype(np.float64)))
        assert abs(r['log_marginal_final'][s] - lz) <= 1e-7 * abs(lz), (s, r['log_marginal_final'][s], lz)
        np.testing.assert_allclose(r['log_one_step_predictive_marginals_all'][off[s]:off[s + 1]], cs, rtol=1e-6,
                                   atol=1e-5)
    exact, mimic, causal = np.concatenate(exact), np.concatenate(mimic), np.concatenate(causal)
    _latent_only_bar(r['posterior_all'], exact, mimic)
    _latent_only_bar(np.exp(r['log_posterior_all'].astype(np.float64)), exact, mimic)
    argmax_match(r['posterior_all'], exact)
    assert np.abs(np.exp(r['log_causal_posterior_all'].astype(np.float64)) - causal).max() < 1e-5


# ----------------------------------------------------------------------------- 5. the banded models
def test_exact_agrees_with_the_default_and_with_a_decode_latent_loop():
    import poor_man_gplvm_amd as P
    L, N = 100, R.N_NEURON
    d, seg = R.jump_data(N, L)
    off = R.offsets()
    m = P.PoissonGPLVMJump1D(N, n_latent_bin=L, tuning_lengthscale=10.)
    e = m.decode_latent_segments(d['y'], seg, tuning=d['tuning'], exact=True)
    f = m.decode_latent_segments(d['y'], seg, tuning=d['tuning'])
    assert list(f) == JUMP_KEYS[:-1] and list(e) == JUMP_KEYS
    for k in ('posterior_all', 'posterior_latent_marg', 'posterior_dynamics_marg'):
        close_prob(e[k], f[k])
    close_prob(np.exp(e['log_causal_posterior_all'].astype(np.float64)),
               np.exp(f['log_causal_posterior_all'].astype(np.float64)))
    assert np.all(np.abs(e['log_marginal_final'] - f['log_marginal_final']) <= 1e-7 * np.abs(f['log_marginal_final']))
    np.testing.assert_allclose(e['log_one_step_predictive_marginals_all'], f['log_one_step_predictive_marginals_all'],
                               rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(e['log_likelihood_all'], f['log_likelihood_all'], rtol=2e-7, atol=1e-5)
    parts = []
    for a, b in seg:
        q = m.decode_latent(d['y'][a:b], tuning=d['tuning'])
        parts.append(dict(gamma=q['posterior_all'].astype(np.float64),
                          log_gamma=q['log_posterior_all'].astype(np.float64),
                          logc=q['log_one_step_predictive_marginals_all'], logz=q['log_marginal_final']))
    loop = R._pack(parts, off)
    out = dict(gamma=e['posterior_all'], P=e['posterior_latent_marg'], log_gamma=e['log_posterior_all'], logc=e['log_one_step_predictive_marginals_all'],
               logz=e['log_marginal_final'])
    _check(out, loop, off, "decode_latent loop")


# ----------------------------------------------------------------------------- 6. the long-event route
def test_long_events_take_the_chunk_parallel_dense_scans():
    """segment_wave_max = 16: the 17- and 33-row events go to the chunk-parallel dense scans
    and are spliced in (log_alpha included); the result stays within the bars of the
    all-one-workgroup result, and the other events keep their values bit for bit."""
    import poor_man_gplvm_amd as P
    from poor_man_gplvm_amd.engine import ScanConfig
    L = 80
    d, K, off = R.inputs(L)
    kw = dict(n_latent_bin=L, tuning_lengthscale=10., custom_transition_kernel=K)
    routed = P.PoissonGPLVMJump1D(R.N_NEURON, scan_config=ScanConfig(segment_wave_max=16), **kw)
    plain = P.PoissonGPLVMJump1D(R.N_NEURON, **kw)
    lens = np.diff(off)
    assert min(plain.scan_config.segment_wave_max, plain.scan_config.segment_dense_max) >= lens.max()
    assert sorted(lens[lens > 16]) == [17, 33]
    r = routed.decode_latent_segments(d['y'], _segments(off), tuning=d['tuning'], exact=True)
    q = plain.decode_latent_segments(d['y'], _segments(off), tuning=d['tuning'], exact=True)
    ref = dict(gamma=q['posterior_all'].astype(np.float64), log_gamma=q['log_posterior_all'].astype(np.float64),
               alpha=np.exp(q['log_causal_posterior_all'].astype(np.float64)),
               logc=q['log_one_step_predictive_marginals_all'], logz=q['log_marginal_final'])
    _check_jump(r, ref, off, L, "routed vs one workgroup")
    _check_jump(r, R.reference(L), off, L, "routed vs float64")
    for s in np.flatnonzero(lens <= 16):
        sl = slice(int(off[s]), int(off[s + 1]))
        for k in JUMP_KEYS[1:]:
            if k != 'log_marginal_final':
                assert np.array_equal(r[k][sl], q[k][sl], equal_nan=True), (s, k)
        assert r['log_marginal_final'][s] == q['log_marginal_final'][s]
