"""The segment smoother (pmg_segment_smoother: one wave per segment, csrc/segments.hip) and
decode_latent_segments against per-segment float64 references.

Every (J latents per lane, WP band taps) instantiation (J in {1, 2, 4, 8, 16} x WP in
{5, 9, 17, 32}) runs the standard ragged batch tests/segments_ref.LENS twice, as
tests/test_gpu_scan_matrix.py does for the chunk-parallel scans: a ragged line
(L = 61 .. 1000, band = WP - 2) and a full-lane line (L = 64 J, band = WP), on the flat-band
transition, driven through DeviceEM directly.  tests/test_segments_host.py shows that a lost
outer tap or a filter run across a segment boundary would miss these bars by a factor
>= 100 in every segment.  Bars: those of test_forward_backward_vs_oracle
(tests/test_gpu_parity.py), per segment.

Then tiny lines, bit-for-bit independence of a segment from the rest of the call,
likelihood_scale, the public API of both observation models, and the routing of long
segments to the chunk-parallel scans.
"""
import numpy as np
import pytest
import torch

from oracle import gplvm_oracle as O
from tests import scan_ref as S
from tests import segments_ref as R
from tests.synth import make
from tests.test_gpu_parity import argmax_match, close_prob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _engine(d, tr, L):
    from poor_man_gplvm_amd.engine import DeviceEM, SpikeData
    eng = DeviceEM(SpikeData(d['y']), L, basis=d['B'])
    eng.set_transition(tr)
    eng.set_ma_latent(None)
    eng.set_tuning(d['tuning'])
    return eng


def _smooth(d, tr, L, off, order=None, likelihood_scale=1.0, rows=None):
    """One emission + segment_smoother call over d['y'][rows]; host arrays
    (gamma, P, alpha, logc, logz), with the status words checked."""
    y = d['y'] if rows is None else d['y'][rows[0]:rows[1]]
    eng = _engine(dict(d, y=np.ascontiguousarray(y)), tr, L)
    T = eng.T
    gamma = torch.full((T, 2, L), float('nan'), dtype=torch.float32, device='cuda')
    P = torch.full((T, L), float('nan'), dtype=torch.float32, device='cuda')
    eng.emission(likelihood_scale)
    so = torch.as_tensor(np.asarray(off, np.int64), device='cuda')
    od = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device='cuda')
    alpha, logc, logz = eng.segment_smoother(likelihood_scale, so, od, gamma=gamma, P=P)
    eng.emission_status()
    eng.check_status()
    return tuple(t.cpu().numpy() for t in (gamma, P, alpha, logc, logz))


def _check(out, ref, off, L, what=""):
    gamma, P, alpha, logc, logz = out
    ref_gamma, ref_logz, ref_alpha, ref_logc = ref
    err = np.abs(gamma - ref_gamma) / (1e-5 * np.abs(ref_gamma) + 1e-12)
    print(f"{what} L={L} gamma err / bar {err.max():.3f} "
          f"logZ rel {np.max(np.abs(logz - ref_logz) / np.abs(ref_logz)):.2e}")
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        close_prob(gamma[a:b], ref_gamma[a:b])
        close_prob(gamma[a:b].sum(1), ref_gamma[a:b].sum(1))
        close_prob(P[a:b], ref_gamma[a:b].sum(1))
        if L > 1:
            argmax_match(gamma[a:b].sum(1), ref_gamma[a:b].sum(1))
        close_prob(alpha[a:b], ref_alpha[a:b])
        assert abs(logz[s] - ref_logz[s]) <= 1e-7 * abs(ref_logz[s]), (s, logz[s], ref_logz[s])
        np.testing.assert_allclose(logc[a:b], ref_logc[a:b], rtol=1e-6, atol=1e-5)


def _run(run, likelihood_scale=1.0):
    L = run['L']
    d, tr, off, ref = R.segment_reference(L, run['band'], R.LENS, run['seed'], likelihood_scale)
    out = _smooth(d, tr, L, off, likelihood_scale=likelihood_scale)
    _check(out, ref, off, L, f"band={tr.band}")
    return out


@pytest.mark.parametrize("J,WP", R.SEG_PAIRS)
def test_segment_pair(J, WP):
    runs = R.seg_runs(J, WP)
    _run(runs['ragged'])
    _run(runs['full'])


@pytest.mark.parametrize("L", R.TINY_L)
def test_tiny_line(L):
    _run(R.tiny_run(L))


def test_likelihood_scale():
    _run(R.seg_runs(4, 9)['ragged'], likelihood_scale=0.5)


@pytest.mark.parametrize("L,band", [(250, 7), (1000, 15)])
def test_segments_are_independent_bit_for_bit(L, band):
    d, tr, off, _ = R.segment_reference(L, band, R.LENS, 0)
    S_ = len(R.LENS)
    base = _smooth(d, tr, L, off)

    def same(out, s, a, b):
        """segment s of `base` == rows [a, b) of `out` with logz index given by the caller"""
        for k in range(4):
            assert np.array_equal(base[k][off[s]:off[s + 1]], out[k][a:b]), (s, k)

    # each segment equals its own S = 1 call
    for s in range(S_):
        a, b = int(off[s]), int(off[s + 1])
        one = _smooth(d, tr, L, [0, b - a], rows=(a, b))
        same(one, s, 0, b - a)
        assert base[4][s] == one[4][0]
    # the batch with its segments permuted
    perm = np.random.default_rng(3).permutation(S_)
    yp = np.concatenate([d['y'][off[s]:off[s + 1]] for s in perm])
    offp = R.offsets([R.LENS[s] for s in perm])
    outp = _smooth(dict(d, y=yp), tr, L, offp)
    for k, s in enumerate(perm):
        same(outp, s, int(offp[k]), int(offp[k + 1]))
        assert base[4][s] == outp[4][k]
    # order: scheduling only
    from poor_man_gplvm_amd.core import segment_order
    for order in (np.arange(S_)[::-1].copy(), segment_order(off)):
        out = _smooth(d, tr, L, off, order=order)
        for k in range(5):
            assert np.array_equal(base[k], out[k]), k


# ----------------------------------------------------------------------------- public API
_API_SEGMENTS = np.array([[395, 400], [10, 40], [0, 1], [200, 233], [41, 49], [100, 117], [300, 302], [60, 64],
                          [350, 359], [120, 125], [5, 12], [250, 266]])


def _api_inputs():
    N, L, T = 30, 100, 400
    d = make(N, L, T, mv=1.0)
    rng = np.random.default_rng(11)
    ml = (rng.random(L) > 0.2).astype(np.float32)
    mn = (rng.random(N) > 0.2).astype(np.float32)
    return N, L, T, d, ml, mn


def test_decode_latent_segments_poisson_vs_oracle():
    import poor_man_gplvm_amd as P
    N, L, T, d, ml, mn = _api_inputs()
    seg = _API_SEGMENTS
    assert seg[0, 1] == T and np.any(np.diff(seg[:, 0]) < 0)
    m = P.PoissonGPLVMJump1D(N, n_latent_bin=L, tuning_lengthscale=10., movement_variance=1.)
    r = m.decode_latent_segments(d['y'], seg, tuning=d['tuning'], ma_neuron=mn, ma_latent=ml)
    assert list(r) == ['segment_offsets', 'posterior_all', 'posterior_latent_marg', 'posterior_dynamics_marg',
                       'log_causal_posterior_all', 'log_one_step_predictive_marginals_all', 'log_likelihood_all',
                       'log_marginal_final']
    off = r['segment_offsets']
    assert off.dtype == np.int64 and r['log_marginal_final'].dtype == np.float64
    np.testing.assert_array_equal(np.diff(off), seg[:, 1] - seg[:, 0])
    Ttot = int(off[-1])
    assert r['posterior_all'].shape == (Ttot, 2, L) and r['posterior_latent_marg'].shape == (Ttot, L)
    assert r['posterior_dynamics_marg'].shape == (Ttot, 2) and r['log_causal_posterior_all'].shape == (Ttot, 2, L)
    assert r['log_one_step_predictive_marginals_all'].shape == (Ttot,) and r['log_likelihood_all'].shape == (Ttot, L)
    assert r['log_marginal_final'].shape == (len(seg),)
    _, logK, _, logA = O.create_transition_prob_1d(L, 1.0, 0.01, 0.01)
    keep = ml.astype(bool)
    for s, (a, b) in enumerate(seg):
        ys = d['y'][a:b]
        ref = O.decode_latent(ys, d['tuning'], 1.0, 0.01, 0.01, ma_neuron=mn, ma_latent=ml)
        lca = O.smooth_all_step_combined_ma_chunk(ys.astype(np.float64), d['tuning'], logK, logA, mn, ml,
                                                  with_joint=False)[2]
        sl = slice(int(off[s]), int(off[s + 1]))
        close_prob(r['posterior_all'][sl], ref['posterior_all'])
        close_prob(r['posterior_latent_marg'][sl], ref['posterior_latent_marg'])
        close_prob(r['posterior_dynamics_marg'][sl], ref['posterior_dynamics_marg'])
        argmax_match(r['posterior_latent_marg'][sl], ref['posterior_latent_marg'])
        close_prob(np.exp(r['log_causal_posterior_all'][sl].astype(np.float64)), np.exp(lca))
        # masked latents carry the reference's -1e20, not log(0)
        np.testing.assert_allclose(r['log_causal_posterior_all'][sl][:, :, ~keep], lca[:, :, ~keep], rtol=1e-6)
        assert abs(r['log_marginal_final'][s] - ref['log_marginal_final']) <= 1e-7 * abs(ref['log_marginal_final'])
        np.testing.assert_allclose(r['log_one_step_predictive_marginals_all'][sl],
                                   ref['log_one_step_predictive_marginals_all'], rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(r['log_likelihood_all'][sl][:, keep], ref['log_likelihood_all'][:, keep],
                                   rtol=2e-7, atol=1e-5)


def test_decode_latent_segments_gaussian_vs_single_decodes():
    """Against model.decode_marginals on each segment alone (the chunk-parallel GPU path of
    the parent commit, not the code under test), with one list-input call."""
    import poor_man_gplvm_amd as P
    N, L, T, d, ml, mn = _api_inputs()
    seg = _API_SEGMENTS
    rng = np.random.default_rng(12)
    tun = rng.normal(size=(L, N)).cumsum(0) * 0.2
    lat = O.sample_latent(T, L, np.random.default_rng(13), 1.0)[:, 1]
    y = (tun[lat] + 0.5 * rng.normal(size=(T, N))).astype(np.float32)
    m = P.GaussianGPLVMJump1D(N, noise_std=0.5, n_latent_bin=L, tuning_lengthscale=10., movement_variance=1.)
    r = m.decode_latent_segments(y, seg, tuning=tun, ma_neuron=mn, ma_latent=ml)
    rl = m.decode_latent_segments([y[a:b] for a, b in seg], tuning=tun, ma_neuron=mn, ma_latent=ml)
    for k in r:
        assert np.array_equal(r[k], rl[k], equal_nan=True), k
    off = r['segment_offsets']
    for s, (a, b) in enumerate(seg):
        ref = m.decode_marginals(y[a:b], tuning=tun, ma_neuron=mn, ma_latent=ml)
        sl = slice(int(off[s]), int(off[s + 1]))
        close_prob(r['posterior_dynamics_marg'][sl], ref['posterior_dynamics_marg'])
        assert abs(r['log_marginal_final'][s] - ref['log_marginal_final']) <= 1e-7 * abs(ref['log_marginal_final'])
        np.testing.assert_allclose(r['log_one_step_predictive_marginals_all'][sl],
                                   ref['log_one_step_predictive_marginals_all'], rtol=1e-6, atol=1e-5)


def test_long_segments_take_the_chunk_parallel_scans():
    """segment_wave_max = 16 on lengths [5, 40, 300, 9]: the two long segments are decoded
    by the chunk-parallel scans and spliced in; every segment meets the reference bars and
    the short ones equal the all-short call bit for bit."""
    import poor_man_gplvm_amd as P
    from poor_man_gplvm_amd.engine import ScanConfig
    N, L = S.N_NEURON, 100
    lens = (5, 40, 300, 9)
    off = R.offsets(lens)
    d = make(N, L, int(off[-1]), mv=1.0)
    seg = np.stack([off[:-1], off[1:]], 1)
    kw = dict(n_latent_bin=L, tuning_lengthscale=10., movement_variance=1.)
    routed = P.PoissonGPLVMJump1D(N, scan_config=ScanConfig(segment_wave_max=16), **kw)
    plain = P.PoissonGPLVMJump1D(N, **kw)
    assert plain.scan_config.segment_wave_max >= max(lens)
    r = routed.decode_latent_segments(d['y'], seg, tuning=d['tuning'])
    q = plain.decode_latent_segments(d['y'], seg, tuning=d['tuning'])
    _, logK, _, logA = O.create_transition_prob_1d(L, 1.0, 0.01, 0.01)
    for s in range(len(lens)):
        sl = slice(int(off[s]), int(off[s + 1]))
        lpa, lz, lca, cs, _, ll = O.smooth_all_step_combined_ma_chunk(d['y'][sl].astype(np.float64), d['tuning'],
                                                                      logK, logA, with_joint=False)
        for res in (r, q):
            close_prob(res['posterior_all'][sl], np.exp(lpa))
            close_prob(res['posterior_latent_marg'][sl], np.exp(lpa).sum(1))
            close_prob(res['posterior_dynamics_marg'][sl], np.exp(lpa).sum(2))
            argmax_match(res['posterior_latent_marg'][sl], np.exp(lpa).sum(1))
            close_prob(np.exp(res['log_causal_posterior_all'][sl].astype(np.float64)), np.exp(lca))
            assert abs(res['log_marginal_final'][s] - lz) <= 1e-7 * abs(lz)
            np.testing.assert_allclose(res['log_one_step_predictive_marginals_all'][sl], cs, rtol=1e-6, atol=1e-5)
            np.testing.assert_allclose(res['log_likelihood_all'][sl], ll, rtol=2e-7, atol=1e-5)
        if lens[s] <= 16:
            for k in r:
                if k not in ('segment_offsets', 'log_marginal_final'):
                    assert np.array_equal(r[k][sl], q[k][sl]), (s, k)
            assert r['log_marginal_final'][s] == q['log_marginal_final'][s]
