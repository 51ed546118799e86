"""The int8-digit Poisson emission pinned to the integer reference of tests/emission_ref.py
at its operand extremes: digits at -128 / 127, single digit planes at the kernels'
fragment, chunk and ring-slot edges, counts of 126 / 127, tuning = 0 columns and
|ll| >= 2^21.  Every bar is bit-identity or a formula evaluated from the reference
(emission_ref's head comment derives them; tests/test_emission_ref_host.py checks on the
CPU that they are tight enough to catch one digit unit):

  D      |D_gpu - D_int| <= bound_D = 8 u M + 4 u |Q|[|S| >= 2^53], the double difference
         against an all-zero time row and a reference latent, device lgamma / lamsum cancel;
  ll64   |ll64 - ll_ref| <= bound_ll = bound_D + N u (lamsum + |gconst|);
  rblk   == float64(float32(max over the block's valid latents of ll64)), masked latents
         being -1e20 in ll64 (a fully masked block: float32(-1e20));
  delta  == float32(ll64 - rblk), rblk repeated over its 32 latents;
  the four kernel variants (PMG_EMISSION_PIPE / PMG_EMISSION_MT = 0/1, 0/2, 1/1, auto/1)
  bit-identical in delta, rblk and ll64.
"""
import numpy as np
import pytest
import torch

from tests import emission_ref as E

pytestmark = pytest.mark.gpu
LD = np.longdouble
VARIANTS = (("0", "1"), ("0", "2"), ("1", "1"), ("auto", "1"))


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _run(monkeypatch, y, tuning, dt=1.0, ma=None, ml=None, variants=VARIANTS, with_ll=True):
    """{variant: (delta, rblk, ll64, int_path)} of one emission per kernel variant,
    emission_status() clean for each."""
    from poor_man_gplvm_amd.engine import DeviceEM, SpikeData
    T, L = y.shape[0], tuning.shape[0]
    out = {}
    for pipe, mt in variants:
        monkeypatch.setenv("PMG_EMISSION_MT", mt)
        monkeypatch.setenv("PMG_EMISSION_PIPE", pipe)
        sp = SpikeData(np.asarray(y, np.float32), ma)
        eng = DeviceEM(sp, L)
        eng.set_ma_latent(ml)
        if with_ll:
            eng.ll64 = torch.empty((T, L), dtype=torch.float64, device='cuda')
        eng.set_tuning(np.array(tuning, np.float64))       # a copy: the cases' arrays are read-only
        eng.emission(1.0, dt)
        eng.emission_status()
        out[pipe + mt] = (eng.delta.cpu().numpy(), eng.rblk.cpu().numpy(), eng.ll64.cpu().numpy(), sp, eng)
    return out


def _identities(delta, rblk, ll64, L):
    """rblk and delta from ll64, bit for bit (the int8 kernels' output format)."""
    T = ll64.shape[0]
    nblk = (L + 31) // 32
    pad = np.full((T, nblk * 32), -np.inf)
    pad[:, :L] = ll64
    want_r = pad.reshape(T, nblk, 32).max(2).astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(rblk, want_r)
    want_d = (ll64 - np.repeat(rblk, 32, axis=1)[:, :L]).astype(np.float32)
    np.testing.assert_array_equal(delta, want_d)


def _assert_same(out):
    base = out["01"]
    for key in ("02", "11", "auto1"):
        for a, b in zip(base[:3], out[key][:3]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("c", E.CASES, ids=[E.case_id(c) for c in E.CASES])
def test_emission_exact(c, monkeypatch):
    case = E.make_case(*c)
    r = case.ref
    L = case.L
    out = _run(monkeypatch, case.y, case.tuning, case.dt, case.ma, case.ml)
    keep = np.ones(L, bool) if case.ml is None else case.ml != 0
    for key, (delta, rblk, ll64, sp, _) in out.items():
        assert sp.int_path and sp.ybt is not None, key
        assert np.all(ll64[:, ~keep] == -1e20), key
        D = E.double_difference(ll64, r.t0, r.l0)
        eD = np.abs((D - r.D).astype(np.float64))[:, keep]
        ell = np.abs((ll64.astype(LD) - r.ll).astype(np.float64))[:, keep]
        print(f"{key}: max |D - D_int| / bound {np.max(eD / r.bound_D[:, keep]):.3f} (max {eD.max():.3e}), "
              f"max |ll - ref| / bound {np.max(ell / r.bound_ll[:, keep]):.3f} (max {ell.max():.3e})")
        assert np.all(eD <= r.bound_D[:, keep]), key
        assert np.all(ell <= r.bound_ll[:, keep]), key
        _identities(delta, rblk, ll64, L)
    _assert_same(out)


def _raised(case, new):
    """The case's counts with one entry of the largest count changed to new, away from the
    all-zero row; (y float32, t, n)."""
    y = case.y.astype(np.float32)
    big = E.COUNTS[case.family][-1]
    t = int(np.flatnonzero((case.y == big).any(1) & (np.count_nonzero(case.y, axis=1) > 1))[3])
    n = int(np.flatnonzero(case.y[t] == big)[5])
    y[t, n] = new
    return y, t, n


@pytest.mark.parametrize("new", [128.0, 2.5])
def test_path_boundary(new, monkeypatch):
    """Counts up to 127 take the int8 path; 128 (or 2.5) anywhere sends the whole matrix
    through k_emission_f64.  That kernel against the longdouble reference of true logs:
    |ll64 - ref| <= (N + 16) u (A1 + A2 + G) + 4 u sum_n y m  (emission_ref.f64_reference
    derives it from the kernel's loop; <= c u N max|term| with c = 3 (N + 16)); on the rows
    that do not hold the changed count the two paths differ by what their references
    differ (the 2^-32 quantisation of log lam), within the sum of the two bounds."""
    c = ('B', 516, 257, 96, 0.02, 'none')
    case = E.make_case(*c)
    r = case.ref
    from poor_man_gplvm_amd.engine import SpikeData
    y, t, n = _raised(case, new)
    y_int = case.y.astype(np.float32)
    y_int[t, n] = np.floor(new) - (new == 128.0)         # 127 or 2.0: still the int8 path
    sp_int = SpikeData(y_int)
    assert sp_int.int_path and sp_int.ybt is not None
    run = _run(monkeypatch, y, case.tuning, case.dt, variants=(("auto", "1"),))["auto1"]
    delta, rblk, ll64, sp, eng = run
    assert not sp.int_path and sp.ybt is None
    ref, bound = E.f64_reference(y, case.tuning, case.dt)
    err = np.abs((ll64.astype(LD) - ref).astype(np.float64))
    print(f"f64 path: max |ll64 - ref| / bound {np.max(err / bound):.4f} (max {err.max():.3e})")
    assert np.all(err <= bound)
    # loglik() is float32(delta + rblk) of this kernel's float32(ll - block max): two f32 roundings
    ll32 = eng.loglik().cpu().numpy()
    np.testing.assert_array_equal(ll32, (delta.astype(np.float64) + np.repeat(rblk, 32, 1)[:, :case.L])
                                  .astype(np.float32))
    slack = 2.0 ** -24 * (np.abs(ll64 - np.repeat(rblk, 32, 1)[:, :case.L]) + np.abs(ll64)) * (1 + 2.0 ** -20)
    assert np.all(np.abs((ll32.astype(LD) - ref).astype(np.float64)) <= bound + slack)
    # against the int8 path on the untouched rows
    ll_int = _run(monkeypatch, case.y, case.tuning, case.dt, variants=(("auto", "1"),))["auto1"][2]
    rows = np.arange(case.T) != t
    ref_int = E.f64_reference(case.y, case.tuning, case.dt)[0]
    assert np.all(ref_int[rows] == ref[rows])
    gap = np.abs(((ll64.astype(LD) - ll_int.astype(LD)) - (ref - r.ll)).astype(np.float64))
    print(f"f64 vs int8 path: max gap / (sum of bounds) {np.max(gap[rows] / (bound + r.bound_ll)[rows]):.4f}")
    assert np.all(gap[rows] <= (bound + r.bound_ll)[rows])


def test_range_edge(monkeypatch):
    """log(lam) = 59.9 (top digit 60) and log(lam) = -46.05 (tuning = 0) are inside the
    digit range: emission_status() stays clean (|log lam| >= 60 raises:
    test_gpu_parity.test_emission_range_flag_raises) and the four variants agree bit for
    bit.  Nothing is asserted on ll here: lamsum ~ 1e26 makes any bar on it vacuous."""
    c = ('B', 516, 257, 96, 1.0, 'none')
    case = E.make_case(*c)
    tun = np.array(case.tuning, copy=True)
    hot = np.float64(np.exp(LD(59.9)))
    for l, n in ((0, 0), (5, 515), (40, 64), (95, 127), (95, 128)):
        tun[l, n] = hot
    assert np.all(np.abs(np.log(tun + 1e-20)) < 60.0) and np.log(hot) > 59.89
    q, margin = E.recover_q(tun, 1.0)
    assert E.split_kernel(q)[4].max() == 60 and E.split_kernel(q)[4].min() == -46 and margin.min() > 1e-3
    out = _run(monkeypatch, case.y, tun, 1.0)
    _assert_same(out)
    for delta, rblk, ll64, _, _ in out.values():
        assert np.all(np.isfinite(ll64)) and np.all(np.isfinite(rblk))
        _identities(delta, rblk, ll64, case.L)
