"""Host checks of tests/emission_ref.py (no GPU):

  1. the designed digits survive the longdouble recovery, every entry > 1e-3 away from a
     rounding tie (the measured f64 detour is printed: ~1e-6 units of q);
  2. the Python split reproduces the designed digits and the kernel's recurrence, the
     127 -> -128 carry included, and the tuning = 0 entries sit 0.17 from a tie;
  3. Q - lamsum - gconst agrees with oracle.gplvm_oracle.loglikelihood_poisson_all within
     that oracle's own f64 rounding plus the 2^-33 quantisation of each log(lam);
  4. both family conditions on the bound hold, and every named pattern is reached;
  5. a deliberately corrupted reference (one unit in digit 0 under the family's smallest
     non-zero count; one unit under its second-largest count; the lowest plane zeroed)
     leaves the bound: the GPU test would fail for the errors it is meant to catch.
"""
import numpy as np
import pytest

from oracle import gplvm_oracle as O
from tests import emission_ref as E

LD = np.longdouble
IDS = [E.case_id(c) for c in E.CASES]


@pytest.mark.parametrize("c", E.CASES, ids=IDS)
def test_designed_digits_survive_recovery(c):
    case = E.make_case(*c)
    q, margin = E.recover_q(case.tuning, case.dt)
    assert np.array_equal(q, E.compose(case.digits))
    print(f"tie margin min {margin.min():.6f}; designed entries: max distance from the integer "
          f"{(0.5 - margin[~case.zero]).max():.3e}")
    assert margin.min() > 1e-3
    # designed entries: the f64 detour stays within 1e-5 units (documented in emission_ref)
    assert (0.5 - margin[~case.zero]).max() < 1e-5
    assert np.all(case.tuning[case.zero] == 0.0) and np.all(case.tuning[~case.zero] > 0.0)
    # the f64 recovery (what the kernel computes, up to its log's last bits) agrees as well
    lam = case.tuning * np.float64(case.dt) + 1e-20
    x64 = np.log(lam) * 4294967296.0
    assert np.array_equal(np.rint(x64).astype(np.int64), q)
    assert np.abs(x64 - q)[~case.zero].max() < 1e-4
    assert np.all(np.abs(np.log(lam)) < 60.0)


def test_split_matches_design_and_kernel_recurrence():
    # the carry: an unsigned low byte of 128..255 becomes -128..-1 and adds one to the next digit
    assert E.split_python(127) == [127, 0, 0, 0, 0]
    assert E.split_python(128) == [-128, 1, 0, 0, 0]
    assert E.split_python(-128) == [-128, 0, 0, 0, 0]
    assert E.split_python(-129) == [127, -1, 0, 0, 0]
    assert E.split_python(128 + 127 * 256) == [-128, -128, 1, 0, 0]         # a carry that carries on
    assert E.split_python((1 << 32) - 1) == [-1, 0, 0, 0, 1]
    rng = np.random.default_rng(0)
    q = np.concatenate([rng.integers(-61 << 32, 61 << 32, size=2000),
                        np.array([0, 127, 128, -128, -129, 32767, 32768, -(60 << 32), 60 << 32])])
    dk = E.split_kernel(q)
    assert np.array_equal(E.compose(dk), q)
    assert dk[:4].min() >= -128 and dk[:4].max() <= 127 and np.abs(dk[4]).max() <= 61
    assert np.array_equal(dk, np.array([E.split_python(v) for v in q]).T)
    for c in E.CASES[:1] + E.CASES[6:7]:
        case = E.make_case(*c)
        qd = E.compose(case.digits)
        assert np.array_equal(E.split_kernel(qd), case.digits)
        flat = np.array([E.split_python(v) for v in qd.ravel()]).T.reshape(case.digits.shape)
        assert np.array_equal(flat, case.digits)


def test_zero_rate_digits():
    q0, x = E.zero_rate_q()
    frac = float(x - np.floor(x))
    print(f"log(1e-20) 2^32 = {x!r}, fraction {frac:.4f}")
    assert abs(frac - 0.669) < 1e-3 and abs(frac - 0.5) > 0.16
    assert q0 == int(np.rint(np.log(1e-20) * 4294967296.0))                 # the f64 route agrees
    d = E.split_python(q0)
    assert sum(v * 256 ** k for k, v in enumerate(d)) == q0
    assert d[4] == -46 and all(-128 <= v <= 127 for v in d[:4])
    assert np.array_equal(E.split_kernel(np.array([q0]))[:, 0], d)
    case = E.make_case(*E.CASES[6])
    assert case.zero.any()
    assert np.all(case.digits[:, case.zero] == np.array(d)[:, None])


@pytest.mark.parametrize("c", E.CASES, ids=IDS)
def test_reference_matches_oracle(c):
    case = E.make_case(*c)
    r = case.ref
    N = case.N
    ref = O.loglikelihood_poisson_all(case.y, case.tuning, case.ma, None, dt=case.dt)
    m = np.ones(N) if case.ma is None else case.ma.astype(np.float64)
    lam = case.tuning * case.dt + 1e-20
    ym = case.y * m[None, :]
    A1 = ym @ np.abs(np.log(lam)).T
    A2 = (lam * m[None, :]).sum(1)
    G = np.abs(r.gconst).astype(np.float64)
    # the oracle: three f64 sums of N terms (each term and partial within u, log / gammaln
    # within a few ulp), two subtractions; the reference: each log(lam) quantised to 2^-32
    tol = (N + 8) * E.U * (A1 + A2[None, :] + G[:, None]) + ym.sum(1)[:, None] * 2.0 ** -33
    err = np.abs((r.ll - ref.astype(LD)).astype(np.float64))
    print(f"max err {err.max():.3e}, max err / tol {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol)


@pytest.mark.parametrize("c", E.CASES, ids=IDS)
def test_family_condition_and_patterns(c):
    case = E.make_case(*c)
    r = case.ref
    fam, N, T, L = case.family, case.N, case.T, case.L
    bmax = float(r.bound_D.max())
    mag = float((np.abs(r.Q) + np.abs(r.lamsum)[None, :] + np.abs(r.gconst)[:, None]).max())
    print(f"{E.case_id(c)}: bound_D max {bmax:.3e} (condition {E.COND[fam]:.3e}), M {mag:.3e}, "
          f"max |Q| {float(np.abs(r.Q).max()):.3e}, bound_ll max {float(r.bound_ll.max()):.3e}")
    assert bmax < E.COND[fam]
    assert set(np.unique(case.y)) <= set(E.COUNTS[fam])
    top = case.digits[4][~case.zero]
    assert top.min() >= E.TOP_RANGE[0] and top.max() <= E.TOP_RANGE[1]
    if T > 1:
        assert not case.y[r.t0].any() and np.all(r.S[r.t0] == 0)
        assert np.array_equal(r.D, (r.S - r.S[:, r.l0][:, None]).astype(LD) / LD(2 ** 32))
        assert case.y.max() == E.COUNTS[fam][-1]
    if fam == 'A':
        assert not case.zero.any()
    else:
        if L >= 5 and case.ma is None:      # (the neuron mask drops a third of the zero columns)
            # the inexact-Horner regime: |ll| >= 2^21, i.e. |S| >= 2^53, on some rows
            assert case.zero.any() and float(np.abs(r.Q).max()) >= 2.0 ** 21 and np.abs(r.S).max() >= 2 ** 53
    # patterns by name
    if L >= E.bank_size(fam, N):
        low = case.digits[:4]
        i = case.names.index
        assert np.all(low[:, i('low_min')] == -128) and np.all(low[:, i('low_max')] == 127)
        if N > 1:
            a = low[:, i('alt')]
            assert set(np.unique(a)) == {-128, 127} and np.all(a[:, 1:] != a[:, :-1])
            assert np.all(low[:, i('alt_flip')] == -1 - a)                  # -128 <-> 127
        for ne in E.edge_neurons(N):
            for p in range(5):
                d = case.digits[:, i(f'one_p{p}_n{ne}')]
                assert np.count_nonzero(d) == 1 and d[p, ne] != 0
        if fam == 'B':
            for nm in ('zero_head', 'zero_tail', 'zero_alt'):
                assert case.zero[i(nm)].any()


def test_every_shape_and_full_bank_covered():
    for fam, Ns in (('A', {1, 63, 64, 130}), ('B', {516})):
        cs = [c for c in E.CASES if c[0] == fam]
        assert Ns <= {c[1] for c in cs}
        assert {1, 257, 300} <= {c[2] for c in cs} and {1, 37, 96, 100} <= {c[3] for c in cs}
        for N in Ns:      # the whole pattern bank at every N, without a mask
            assert any(c[1] == N and c[3] >= E.bank_size(fam, N) and c[2] > 1 and c[5] == 'none' for c in cs)
    assert {c[5] for c in E.CASES} == {'none', 'neuron', 'latent'}


def _corrupt(case, q2):
    """Largest excess of |D' - D| over the bound for the reference built on q2."""
    r = case.ref
    r2 = E.integer_reference(case.y, q2, case.tuning, case.dt, r.t0, r.l0, case.ma)
    diff = np.abs((r2.D - r.D).astype(np.float64))
    return diff, diff - r.bound_D


@pytest.mark.parametrize("c", [E.CASES[0], E.CASES[1], E.CASES[6], E.CASES[10], E.CASES[12]],
                         ids=lambda c: E.case_id(c))
def test_corrupted_reference_exceeds_bound(c):
    case = E.make_case(*c)
    r = case.ref
    q = E.compose(case.digits)
    m = np.ones(case.N) if case.ma is None else case.ma
    vals = E.COUNTS[case.family]
    # one unit in digit 0 of one neuron, seen through a row whose only spike is that neuron
    # (design_counts: A's one-spike rows carry 1 and 3, B's 127 and 126)
    for count in ((1, vals[-1]) if case.family == 'A' else (vals[-2], vals[-1])):
        rows = np.flatnonzero((np.count_nonzero(case.y, axis=1) == 1) & (case.y.max(1) == count))
        rows = [t for t in rows if m[np.argmax(case.y[t])] == 1]
        t = rows[len(rows) // 2]
        n = int(np.argmax(case.y[t]))
        l = 1 if r.l0 != 1 else 2
        q2 = q.copy()
        q2[l, n] += 1
        diff, excess = _corrupt(case, q2)
        assert diff[t, l] == count * 2.0 ** -32
        print(f"unit under count {count}: moves D by {diff[t, l]:.3e}, bound there {r.bound_D[t, l]:.3e}")
        assert excess[t, l] > 0
        if case.family == 'A':      # a quarter of a unit: the condition of the family
            assert diff[t, l] > 4 * r.bound_D[t, l]
    # the lowest digit plane dropped
    d2 = case.digits.copy()
    d2[0] = 0
    diff, excess = _corrupt(case, E.compose(d2))
    print(f"lowest plane zeroed: max move {diff.max():.3e}, entries outside the bound {np.mean(excess > 0):.2%}")
    assert excess.max() > 0 and np.mean(excess > 0) > 0.25
