"""The posterior path sampler (pmg_segment_sample: one wave per (segment, sample),
csrc/segment_sample.hip) and sample_latent_segments / sample_latent_posterior.

The kernel draws no random numbers: its paths are a deterministic function of (alpha,
transition, uniforms), so every step of every path is judged on its own by
tests/sample_ref.check_paths (teacher forced, float64 weights rebuilt from the device's own
float32 alpha, allowance eps = 64 x 2^-24 of the step's total for the float32 prefix sums).
tests/test_sample_host.py shows on the reference sampler that the allowance is in play at
< 1 % of the steps, that a sampler with a lost outer tap or a transposed A fails the check
at >= 0.3 % / >= 2 % of the steps, and that the reference's own z against the smoothed
posterior stays <= 4.0 with these uniforms.

Throughout: the ragged batch tests/segments_ref.LENS (120 rows), R = 256 samples,
u = default_rng(7).random((256, 120), float32), the flat-band transition, DeviceEM driven
directly (emission, segment_smoother forward only, segment_sampler).  Then exactness
(repeatability, independence of a segment from the rest of the call, of `order` and of R), a
latent mask and a one-way dynamics matrix, and the public API of both observation models.
The kernel's total == 0 path is not provoked here; the host side of its status word is
covered in tests/test_sample_host.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import gplvm_oracle as O
from tests import sample_ref as SR
from tests import scan_ref as S
from tests import segments_ref as R
from tests.synth import make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _engine(d, tr, L, ma_latent=None):
    from poor_man_gplvm_amd.engine import DeviceEM, SpikeData
    eng = DeviceEM(SpikeData(np.ascontiguousarray(d['y'])), L, basis=d['B'])
    eng.set_transition(tr)
    eng.set_ma_latent(ma_latent)
    eng.set_tuning(d['tuning'])
    return eng


def _dev_i64(x):
    return torch.as_tensor(np.asarray(x, np.int64), device='cuda')


def _sample(d, tr, L, off, u, order=None, rows=None, ma_latent=None, gamma=False):
    """Emission, forward filter (segment_smoother with gamma = P = None) and segment_sampler
    over d['y'][rows] with the matching columns of u.  Host arrays (path_d, path_l, alpha), and
    the device's own smoothed gamma from a second segment_smoother call if asked for."""
    y = d['y'] if rows is None else d['y'][rows[0]:rows[1]]
    u = u if rows is None else u[:, rows[0]:rows[1]]
    eng = _engine(dict(d, y=y), tr, L, ma_latent)
    so = _dev_i64(off)
    od = None if order is None else torch.as_tensor(np.asarray(order, np.int32), device='cuda')
    eng.emission(1.0)
    eng.segment_smoother(1.0, so, od)
    pd, pl = eng.segment_sampler(so, torch.tensor(np.ascontiguousarray(u), device='cuda'), od)
    alpha = eng.alpha.cpu().numpy()
    out = [pd.cpu().numpy(), pl.cpu().numpy(), alpha]
    if gamma:
        g = torch.full((eng.T, 2, L), float('nan'), dtype=torch.float32, device='cuda')
        eng.segment_smoother(1.0, so, od, gamma=g)
        assert np.array_equal(eng.alpha.cpu().numpy(), alpha)       # the same forward kernel
        out.append(g.cpu().numpy())
    eng.emission_status()
    eng.check_status()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _case(L, band):
    d, tr, off, _ = R.segment_reference(L, band, SR.LENS, 0)
    return d, tr, off, _sample(d, tr, L, off, SR.uniforms(), gamma=True)


def _id(case):
    return f"L{case[0]}-band{case[1]}"


# ----------------------------------------------------------------------------- every J, VEC, band extreme
@pytest.mark.parametrize("case", SR.CASES, ids=_id)
def test_every_step_of_every_path(case):
    L, band = case
    d, tr, off, (pd, pl, alpha, _) = _case(L, band)
    u = SR.uniforms()
    assert pd.shape == pl.shape == (SR.N_SAMPLES, 120) and pd.dtype == pl.dtype == np.int32
    bad = SR.check_paths(alpha, tr, off, u, pd, pl)
    rep = SR.step_report(alpha, tr, off, u, pd, pl)
    ref_d, ref_l = SR.ffbs(alpha, tr, off, u)
    print(f"{_id(case)}: violations {bad} of {pd.size}, not positive {int((~rep['positive']).sum())}, steps that "
          f"differ from the float64 draw {int(((pd != ref_d) | (pl != ref_l)).sum())}")
    assert bad == 0
    assert pd.min() >= 0 and pd.max() <= 1 and pl.min() >= 0 and pl.max() < L
    # a continuous move never leaves the band: exact, no allowance
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        step = np.abs(pl[:, a:b - 1] - pl[:, a + 1:b])
        assert np.all(step[pd[:, a + 1:b] == 0] <= band), s


@pytest.mark.parametrize("case", SR.CASES, ids=_id)
def test_frequencies_match_the_device_smoother(case):
    """Two independent kernels: the sampled frequencies of d = 1 and of the posterior-mode
    latent against the backward smoother's gamma, z <= 5 in every row."""
    L, band = case
    _, _, _, (pd, pl, _, gamma) = _case(L, band)
    z_d, z_l = SR.z_scores(pd, pl, gamma)
    print(f"{_id(case)}: z_d {z_d.max():.2f}, z_l {z_l.max():.2f}")
    assert z_d.max() <= 5 and z_l.max() <= 5


# ----------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("L,band", [(250, 7), (1000, 15)])
def test_samples_are_exact_functions_of_their_own_rows(L, band):
    d, tr, off, _ = R.segment_reference(L, band, SR.LENS, 0)
    u = SR.uniforms()
    S_ = len(SR.LENS)
    base = _sample(d, tr, L, off, u)
    # two calls
    again = _sample(d, tr, L, off, u)
    for k in range(3):
        assert np.array_equal(base[k], again[k]), k
    # each event equals its own S = 1 call on its rows with its columns of u
    for s in range(S_):
        a, b = int(off[s]), int(off[s + 1])
        one = _sample(d, tr, L, [0, b - a], u, rows=(a, b))
        for k in range(2):
            assert np.array_equal(base[k][:, a:b], one[k]), (s, k)
    # the batch with its events permuted, u's columns permuted to match, and another order
    from poor_man_gplvm_amd.core import segment_order
    perm = np.random.default_rng(3).permutation(S_)
    cols = np.concatenate([np.arange(off[s], off[s + 1]) for s in perm])
    offp = R.offsets([SR.LENS[s] for s in perm])
    order = segment_order(offp)
    assert not np.array_equal(order, np.arange(S_))
    outp = _sample(dict(d, y=d['y'][cols]), tr, L, offp, u[:, cols], order=order)
    for k, s in enumerate(perm):
        for i in range(2):
            assert np.array_equal(base[i][:, off[s]:off[s + 1]], outp[i][:, offp[k]:offp[k + 1]]), (s, i)
    for order in (np.arange(S_)[::-1].copy(), segment_order(off)):
        out = _sample(d, tr, L, off, u, order=order)
        for k in range(2):
            assert np.array_equal(base[k], out[k]), k
    # sample r does not depend on R
    few = _sample(d, tr, L, off, u[:3])
    for k in range(2):
        assert few[k].shape == (3, 120) and np.array_equal(base[k][:3], few[k]), k


# ----------------------------------------------------------------------------- zeros are never drawn
def test_masked_latents_and_a_zero_of_A_are_never_drawn():
    """ma_latent with a block of zeros: no masked latent in any path, exactly.
    p_move_to_jump = 0 (A[0, 1] = 0): no path goes from d = 0 to d = 1 forward in time."""
    L, band = 127, 7
    d = S.wide_step_data(S.N_NEURON, L, 120, band, 0)
    tr = S.flat_transition(L, band, pmj=0.0, pjm=0.3)
    assert tr.A[0, 1] == 0
    mask = np.ones(L, np.float32)
    mask[40:60] = 0
    mask[L - 3:] = 0
    off = R.offsets(SR.LENS)
    u = SR.uniforms()
    pd, pl, alpha = _sample(d, tr, L, off, u, ma_latent=mask)
    assert np.all(alpha[:, :, mask == 0] == 0)
    assert pd.min() >= 0 and pl.min() >= 0
    assert np.all(mask[pl] != 0)
    assert SR.check_paths(alpha, tr, off, u, pd, pl) == 0
    seen = 0
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        assert not np.any((pd[:, a:b - 1] == 0) & (pd[:, a + 1:b] == 1)), s
        seen += int((pd[:, a:b] == 1).sum())
    assert seen > 0                        # d = 1 does occur (at the start of events), so the rule binds


# ----------------------------------------------------------------------------- public API
_API_SEGMENTS = np.array([[395, 400], [10, 40], [0, 1], [200, 233], [41, 49], [100, 117], [300, 302], [60, 64],
                          [350, 359], [120, 125], [5, 12], [250, 266]])


def _api_model(kind):
    import poor_man_gplvm_amd as P
    N, L, T = 30, 100, 400
    d = make(N, L, T, mv=1.0)
    rng = np.random.default_rng(11)
    ml = (rng.random(L) > 0.2).astype(np.float32)
    mn = (rng.random(N) > 0.2).astype(np.float32)
    kw = dict(n_latent_bin=L, tuning_lengthscale=10., movement_variance=1.)
    if kind == 'poisson':
        return P.PoissonGPLVMJump1D, (N,), kw, d['y'], d['tuning'], ml, mn
    rng = np.random.default_rng(12)
    tun = rng.normal(size=(L, N)).cumsum(0) * 0.2
    lat = O.sample_latent(T, L, np.random.default_rng(13), 1.0)[:, 1]
    y = (tun[lat] + 0.5 * rng.normal(size=(T, N))).astype(np.float32)
    return P.GaussianGPLVMJump1D, (N,), dict(kw, noise_std=0.5), y, tun, ml, mn


class _Spy:
    """Records what DeviceEM.segment_sampler saw (that call's alpha, transition, offsets and
    uniforms) and passes the call on."""

    def __init__(self, monkeypatch):
        from poor_man_gplvm_amd.engine import DeviceEM
        self.calls = []
        orig = DeviceEM.segment_sampler
        spy = self

        def wrapped(eng, seg_off, uniforms, order=None):
            spy.calls.append(dict(alpha=eng.alpha.cpu().numpy(), tr=eng._tr, off=seg_off.cpu().numpy(),
                                  u=uniforms.cpu().numpy()))
            return orig(eng, seg_off, uniforms, order)
        monkeypatch.setattr(DeviceEM, 'segment_sampler', wrapped)


@pytest.mark.parametrize("kind", ["poisson", "gaussian"])
def test_sample_latent_segments_api(kind, monkeypatch):
    from poor_man_gplvm_amd.core import gather_segments
    cls, args, kw, y, tun, ml, mn = _api_model(kind)
    seg = _API_SEGMENTS
    m = cls(*args, **kw)
    L, n = kw['n_latent_bin'], 64
    common = dict(tuning=tun, ma_neuron=mn, ma_latent=ml)
    spy = _Spy(monkeypatch)
    r = m.sample_latent_segments(y, seg, n_samples=n, key=5, **common)
    assert list(r) == ['segment_offsets', 'sample_dynamics', 'sample_latent', 'log_marginal_final']
    off = r['segment_offsets']
    Ttot = int(off[-1])
    assert off.dtype == np.int64 and np.array_equal(np.diff(off), seg[:, 1] - seg[:, 0])
    for k in ('sample_dynamics', 'sample_latent'):
        assert r[k].shape == (n, Ttot) and r[k].dtype == np.int32
    assert r['log_marginal_final'].shape == (len(seg),) and r['log_marginal_final'].dtype == np.float64
    pd, pl = r['sample_dynamics'], r['sample_latent']
    assert pd.min() >= 0 and pd.max() <= 1 and pl.min() >= 0 and pl.max() < L and np.all(ml[pl] != 0)
    # the generated uniforms, and every step of the call judged against that call's alpha
    c = spy.calls[-1]
    assert c['u'].shape == (n, Ttot) and c['u'].dtype == np.float32 and c['u'].min() >= 0 and c['u'].max() < 1
    assert SR.check_paths(c['alpha'], c['tr'], off, c['u'], pd, pl) == 0
    # log_marginal_final is decode_latent_segments' (the same forward kernel)
    q = m.decode_latent_segments(y, seg, **common)
    assert np.array_equal(r['log_marginal_final'], q['log_marginal_final'])
    # key: reproducible, and another key gives other samples
    r2 = m.sample_latent_segments(y, seg, n_samples=n, key=5, **common)
    r3 = m.sample_latent_segments(y, seg, n_samples=n, key=6, **common)
    for k in r:
        assert np.array_equal(r[k], r2[k]), k
    assert not np.array_equal(r['sample_latent'], r3['sample_latent'])
    # explicit uniforms (array or device tensor) reproduce the engine-level result
    u = SR.uniforms(n, Ttot, 21)
    ru = m.sample_latent_segments(y, seg, n_samples=n, uniforms=u, **common)
    rt = m.sample_latent_segments(y, seg, n_samples=n, uniforms=torch.tensor(u, device='cuda'), **common)
    yc, off2, ma = gather_segments(y, seg, mn)
    eng = m._decode_engine(yc, tun, m._decode_hp({}), ma, ml, exact=False)
    eng.emission(1.0)
    eng.segment_smoother(1.0, _dev_i64(off2))
    ed, el = eng.segment_sampler(_dev_i64(off2), torch.tensor(u, device='cuda'))
    for res in (ru, rt):
        assert np.array_equal(res['sample_dynamics'], ed.cpu().numpy())
        assert np.array_equal(res['sample_latent'], el.cpu().numpy())
    # list input equals interval input
    rl = m.sample_latent_segments([y[a:b] for a, b in seg], n_samples=n, uniforms=u, **common)
    for k in ru:
        assert np.array_equal(ru[k], rl[k]), k


def test_long_events_take_the_chunk_parallel_forward(monkeypatch):
    """segment_wave_max = 16 on lengths [5, 40, 300, 9]: the two long events are filtered by the
    chunk-parallel forward and spliced in; every step passes the check against that call's
    alpha, and the short events equal the all-short call exactly."""
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
    u = SR.uniforms(32, int(off[-1]), 22)
    spy = _Spy(monkeypatch)
    r = routed.sample_latent_segments(d['y'], seg, n_samples=32, uniforms=u, tuning=d['tuning'])
    c = spy.calls[-1]
    q = plain.sample_latent_segments(d['y'], seg, n_samples=32, uniforms=u, tuning=d['tuning'])
    assert SR.check_paths(c['alpha'], c['tr'], off, u, r['sample_dynamics'], r['sample_latent']) == 0
    lz = routed.decode_latent_segments(d['y'], seg, tuning=d['tuning'])['log_marginal_final']
    np.testing.assert_allclose(r['log_marginal_final'], lz, rtol=1e-7)
    for s in range(len(lens)):
        if lens[s] <= 16:
            sl = slice(int(off[s]), int(off[s + 1]))
            assert np.array_equal(r['sample_latent'][:, sl], q['sample_latent'][:, sl]), s
            assert np.array_equal(r['sample_dynamics'][:, sl], q['sample_dynamics'][:, sl]), s
            assert r['log_marginal_final'][s] == q['log_marginal_final'][s]


def test_sample_latent_posterior_is_the_one_segment_call():
    cls, args, kw, y, tun, ml, mn = _api_model('poisson')
    m = cls(*args, **kw)
    y = y[:150]
    common = dict(n_samples=16, key=3, tuning=tun, ma_neuron=mn, ma_latent=ml)
    p = m.sample_latent_posterior(y, **common)
    s = m.sample_latent_segments(y, [[0, 150]], **common)
    assert list(p) == ['sample_dynamics', 'sample_latent', 'log_marginal_final']
    assert p['sample_latent'].shape == (16, 150) and isinstance(p['log_marginal_final'], float)
    assert np.array_equal(p['sample_dynamics'], s['sample_dynamics'])
    assert np.array_equal(p['sample_latent'], s['sample_latent'])
    assert p['log_marginal_final'] == float(s['log_marginal_final'][0])
    u = SR.uniforms(16, 150, 23)
    pu = m.sample_latent_posterior(y, n_samples=16, uniforms=u, tuning=tun, ma_neuron=mn, ma_latent=ml)
    su = m.sample_latent_segments(y, [[0, 150]], n_samples=16, uniforms=u, tuning=tun, ma_neuron=mn, ma_latent=ml)
    assert np.array_equal(pu['sample_latent'], su['sample_latent'])
