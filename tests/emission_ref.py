"""Exact reference of the int8-digit Poisson emission at its operand extremes (TEST
INFRASTRUCTURE ONLY).

The integer path of csrc/emission.hip claims exactness: counts y (0..127) as int8,
log(lam) as a 2^-32 fixed-point integer q split into five balanced base-256 int8 digits
(k_rates_prepare), five int8 GEMMs with exact int32 sums, recombined in f64.  This module
builds operands whose digits are KNOWN and a reference that never leaves integers:

  designed rates   the digits d0..d4 of every (l, n) are chosen, q = sum_k d_k 256^k and
                   tuning = float64(exp_longdouble(q / 2^32)) / dt.  recover_q() takes the
                   way back, rint(log_longdouble(tuning dt + 1e-20) 2^32), and reports how
                   far the unrounded value is from a rounding tie k + 1/2: the kernel
                   rounds to nearest, so its integer can differ from q only next to a tie.
                   The f64 roundings on the way (exp, / dt, * dt, + 1e-20, and one or two
                   roundings of tuning dt + 1e-20 depending on fma contraction) move the
                   value by < 1e-5 units of q, and a device log a few ulp off by 2^-20
                   units per ulp; tests assert a margin > 1e-3.  Entries with tuning = 0
                   exactly have lam = 1e-20; their digits are not designed but taken from
                   the host split of rint(log(1e-20) 2^32) (fraction 0.669, 0.17 from a tie).
  integer reference  S[t, l] = sum_n (y m)[t, n] q[l, n] in int64, Q = S / 2^32, and
                   lamsum[l] = sum_n m_n lam[l, n], gconst[t] = sum_n m_n lgamma(y + 1)
                   in longdouble; ll = Q - lamsum - gconst.

The pinned quantity is a double difference, so the device's lamsum and lgamma values
cancel whatever their last bits are: with an all-zero time row t0 and a reference latent l0,

    D[t, l] = ll[t, l] - ll[t0, l] - ll[t, l0] + ll[t0, l0]  ==  (S[t, l] - S[t, l0]) / 2^32.

Bound (Reference.bound_D, from the reference alone).  The epilogue computes
v = fl(fl(Q - lsum) - gc) with Q = q 2^-32 exact: two roundings of relative size
u = 2^-53, |v - exact| <= 2 u (|Q| + |lsum| + |gc|).  Over the four entries of D:
|D_gpu - D_int| <= 8 u M, M = max over the four of |Q| + |lsum| + |gc|.  The Horner
recombination q = fma(fma(fma(fma(a4, 256, a3), 256, a2), 256, a1), 256, a0) works on
integers; every partial but the last is below |S| / 256 + 2^24, so only the last step can
round, and only where |S| >= 2^53 (|ll| >= 2^21): there it adds u |Q| per entry, 4 u |Q|
(largest such |Q| of the four) to the bound.

ll itself (Reference.bound_ll) additionally sees the device's own lamsum and gconst: N
terms each, every term and every partial sum within u relative (lgamma table and lam
within an ulp or two), so bound_ll = bound_D + N u (lamsum + |gconst|).

Two operand families, each with a condition on bound_D that tests/test_emission_ref_host.py
asserts:
  A  counts 0..3, N in {1, 63, 64, 130}, top digit in [-7, 3]: bound_D < 2^-34, a quarter
     of one unit of the lowest digit under a count of 1 (2^-32).
  B  counts from {0, 1, 126, 127}, N = 516 (ring kernel) and, beyond the issue's list,
     N = 512 (the register-resident kernel's int32 digit-pair sums at their largest),
     columns with tuning = 0 so that |Q| passes 2^21: bound_D < 2^-27, a quarter of one
     unit under a count of 126 (~2^-25).
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
QBITS = 32
QSCALE = 1 << QBITS
NDIG = 5
RATE_EPS = 1e-20
TOP_RANGE = (-7, 3)                      # top digit of the designed rates (lam <= e^3.5)
EXTREME_DIGITS = (-128, 127, 0, 1, -1, -127, 126)
COND = {'A': 2.0 ** -34, 'B': 2.0 ** -27}
COUNTS = {'A': (0, 1, 2, 3), 'B': (0, 1, 126, 127)}


def _need_extended():
    if np.finfo(LD).nmant < 63:
        raise RuntimeError("tests/emission_ref.py needs an extended-precision numpy longdouble")


# ----------------------------------------------------------------------------- digits
def edge_neurons(N):
    """Fragment (16, 32), chunk (64, 128) and ring-slot edges of the three kernels."""
    return sorted({n for n in (0, 15, 16, 31, 32, 63, 64, 127, 128, N - 1) if 0 <= n < N})


def compose(digits):
    """q = sum_k d_k 256^k (int64) of a (5, ...) digit array."""
    d = np.asarray(digits, np.int64)
    q = np.zeros(d.shape[1:], np.int64)
    for k in reversed(range(NDIG)):
        q = q * 256 + d[k]
    return q


def split_kernel(q):
    """k_rates_prepare's recurrence, as written there: rr = ((q + 128) & 255) - 128,
    q = (q - rr) >> 8, the last digit what is left."""
    q = np.array(q, np.int64, copy=True)
    out = []
    for _ in range(NDIG - 1):
        rr = ((q + 128) & 255) - 128
        out.append(rr)
        q = (q - rr) >> 8
    out.append(q)
    return np.stack(out)


def split_python(q):
    """The balanced base-256 digits of one Python int, written without the kernel's bit
    tricks: the residue nearest zero (ties to -128), exact division."""
    q = int(q)
    out = []
    for _ in range(NDIG - 1):
        r = q % 256                      # 0 .. 255, Python's floor modulus
        if r >= 128:
            r -= 256                     # 128 .. 255 -> -128 .. -1: the carry into the next digit
        out.append(r)
        q = (q - r) // 256
    out.append(q)
    return out


def zero_rate_q():
    """q of tuning = 0 (lam = 1e-20) and the unrounded scaled log."""
    _need_extended()
    x = np.log(LD(RATE_EPS)) * LD(QSCALE)
    return int(np.rint(x)), x


def design_digits(N, L, family, seed):
    """(digits (5, L, N) int64, zero (L, N) bool, names [L]): the pattern rows in a fixed
    order, then random rows up to L (L below the bank: its first L rows).  zero marks the
    tuning = 0 entries (family B only); their digits are those of zero_rate_q()."""
    rng = np.random.default_rng(seed)
    lo, hi = TOP_RANGE
    n = np.arange(N)
    rows, names = [], []

    def top():
        return rng.integers(lo, hi + 1, size=N)

    def add(name, low, t=None, zero=None):
        d = np.zeros((NDIG, N), np.int64)
        d[:NDIG - 1] = low
        d[NDIG - 1] = top() if t is None else t
        rows.append((d, np.zeros(N, bool) if zero is None else zero))
        names.append(name)

    def random_low():
        full = rng.integers(-128, 128, size=(NDIG - 1, N))
        ext = rng.choice(EXTREME_DIGITS, size=(NDIG - 1, N))
        return np.where(rng.random((NDIG - 1, N)) < 0.5, ext, full)

    add('low_min', -128)
    add('low_max', 127)
    k = np.arange(NDIG - 1)[:, None]
    add('alt', np.where((n[None, :] + k) % 2 == 0, -128, 127))
    add('alt_flip', np.where((n[None, :] + k) % 2 == 0, 127, -128))
    if family == 'B':
        # columns with tuning = 0: most of the row (|Q| past 2^21 under counts of 127), the
        # upper part, every other column
        for name, z in (('zero_head', n < (4 * N) // 5), ('zero_tail', n >= N // 5), ('zero_alt', n % 2 == 1)):
            add(name, random_low(), zero=z)
    low_vals, top_vals = (1, -128, 127), (1, lo, hi)
    for i, ne in enumerate(edge_neurons(N)):
        for p in range(NDIG):
            d = np.zeros((NDIG, N), np.int64)
            d[p, ne] = top_vals[i % 3] if p == NDIG - 1 else low_vals[(i + p) % 3]
            rows.append((d, np.zeros(N, bool)))
            names.append(f'one_p{p}_n{ne}')
    while len(rows) < L:
        add(f'random{len(rows)}', random_low())
    rows, names = rows[:L], names[:L]
    digits = np.stack([r[0] for r in rows], axis=1)
    zero = np.stack([r[1] for r in rows])
    qz = np.array(split_python(zero_rate_q()[0]), np.int64)
    digits = np.where(zero[None], qz[:, None, None], digits)
    return digits, zero, names


def design_tuning(digits, zero, dt):
    """tuning (L, N) float64 = float64(exp_longdouble(q / 2^32)) / dt, 0 where zero."""
    _need_extended()
    x = compose(digits).astype(LD) / LD(QSCALE)
    tun = np.exp(x).astype(np.float64) / np.float64(dt)
    return np.where(zero, 0.0, tun)


def recover_q(tuning, dt):
    """(q int64, margin): q = rint(log_longdouble(tuning dt + 1e-20) 2^32) and the distance
    of the unrounded value from the nearest rounding tie."""
    _need_extended()
    lam = np.asarray(tuning, np.float64).astype(LD) * LD(np.float64(dt)) + LD(RATE_EPS)
    x = np.log(lam) * LD(QSCALE)
    q = np.rint(x)
    margin = (LD(0.5) - np.abs(x - q)).astype(np.float64)
    return q.astype(np.int64), margin


# ----------------------------------------------------------------------------- counts
def design_counts(N, T, family, seed):
    """(y (T, N) int64, t0): an all-zero row t0 = T // 2 (T = 1: the single row is not
    zero and D is trivially 0), one-spike rows at the edge neurons (largest and
    second-largest count of the family), full rows of the largest count (the last row
    too: the ragged time tile), the two largest counts alternating along n, the rest
    drawn from the family's counts."""
    rng = np.random.default_rng(seed)
    vals = np.array(COUNTS[family])
    p = (0.55, 0.25, 0.12, 0.08) if family == 'A' else (0.3, 0.2, 0.2, 0.3)
    y = rng.choice(vals, size=(T, N), p=p).astype(np.int64)
    t0 = T // 2
    t = 0
    for c in ((1, vals[-1]) if family == 'A' else (vals[-1], vals[-2])):
        for ne in edge_neurons(N):
            if t < T:
                y[t] = 0
                y[t, ne] = c
                t += 1
    n = np.arange(N)
    for row in (np.full(N, vals[-1]), np.where(n % 2 == 0, vals[-2], vals[-1])):
        if t < T:
            y[t] = row
            t += 1
    y[T - 1] = vals[-1]
    if T > 1:
        y[t0] = 0
    return y, t0


# ----------------------------------------------------------------------------- reference
_LGAMMA = None


def _lgamma_table():
    global _LGAMMA
    if _LGAMMA is None:
        _LGAMMA = np.array([math.lgamma(k + 1.0) for k in range(256)], np.float64).astype(LD)
    return _LGAMMA


@dataclass(frozen=True)
class Reference:
    q: np.ndarray          # (L, N) int64
    S: np.ndarray          # (T, L) int64
    Q: np.ndarray          # (T, L) longdouble
    lamsum: np.ndarray     # (L,) longdouble
    gconst: np.ndarray     # (T,) longdouble
    ll: np.ndarray         # (T, L) longdouble, unmasked latents only meaningful
    t0: int
    l0: int
    D: np.ndarray          # (T, L) longdouble, exact
    bound_D: np.ndarray    # (T, L) float64
    bound_ll: np.ndarray   # (T, L) float64


def double_difference(ll, t0, l0):
    """D[t, l] = ll[t, l] - ll[t0, l] - ll[t, l0] + ll[t0, l0] in longdouble."""
    a = np.asarray(ll).astype(LD)
    return a - a[t0][None, :] - a[:, l0][:, None] + a[t0, l0]


def integer_reference(y, q, tuning, dt, t0, l0, ma=None):
    """The integer reference of integer counts y (T, N) under the 0/1 neuron mask ma,
    for rates given by their fixed-point integers q (L, N) and tuning (lamsum only)."""
    _need_extended()
    y = np.asarray(y, np.int64)
    q = np.asarray(q, np.int64)
    T, N = y.shape
    m = np.ones(N, np.int64) if ma is None else np.asarray(ma).astype(np.int64)
    assert set(np.unique(m)) <= {0, 1}
    ym = y * m[None, :]
    assert int(np.abs(ym).sum(1).max()) * int(np.abs(q).max()) < 2 ** 62     # int64 cannot overflow
    S = ym @ q.T
    Q = S.astype(LD) / LD(QSCALE)
    lam = np.asarray(tuning, np.float64) * np.float64(dt) + np.float64(RATE_EPS)
    lamsum = (lam.astype(LD) * m[None, :].astype(LD)).sum(1)
    gconst = (_lgamma_table()[y] * m[None, :].astype(LD)).sum(1)
    ll = Q - lamsum[None, :] - gconst[:, None]
    # exact double difference of the integers (|.| < 2^63: exact in longdouble)
    Dint = S - S[t0][None, :] - S[:, l0][:, None] + S[t0, l0]
    D = Dint.astype(LD) / LD(QSCALE)
    mag = (np.abs(Q) + np.abs(lamsum)[None, :] + np.abs(gconst)[:, None]).astype(np.float64)
    big = np.where(np.abs(S) >= 2 ** 53, np.abs(Q).astype(np.float64), 0.0)

    def four(a):
        return np.maximum(np.maximum(a, a[t0][None, :]), np.maximum(a[:, l0][:, None], a[t0, l0]))

    bound_D = 8.0 * U * four(mag) + 4.0 * U * four(big)
    bound_ll = bound_D + N * U * (np.abs(lamsum)[None, :] + np.abs(gconst)[:, None]).astype(np.float64)
    return Reference(q, S, Q, lamsum, gconst, ll, int(t0), int(l0), D, bound_D, bound_ll)


def f64_reference(y, tuning, dt, ma=None):
    """longdouble ll of arbitrary counts (the f64 kernel's operation, true logs) and the
    bound of k_emission_f64 against it.  With A1 = sum_n |y m log lam|, A2 = sum_n m lam,
    G = sum_n m lgamma(y + 1), that kernel's loop gives, per (t, l):
      - a1 and a2: N terms each, one fma per term, so one rounding per step:
        <= (N - 1) u (A1 + A2);
      - its operands: lam = tuning dt + 1e-20 within one ulp of the host's (one rounding
        or two, by fma contraction; 2 u relative) and a device log within 2 ulp (4 u
        relative): <= 4 u A1 + 2 u A2, and lam's ulp through the log moves every term by
        2 u y m: <= 2 u sum_n y m;
      - gconst: N lgamma values taken within 4 ulp (8 u relative), added by a wave
        reduction ((N - 1) u): <= (N + 7) u G;
      - v = fl(fl(a1 - a2) - gc): <= 2 u (A1 + A2 + G).
    Altogether |ll_gpu - ll| <= (N + 16) u (A1 + A2 + G) + 4 u sum_n y m (rounded up).
    With tmax the largest single term, A1 + A2 + G <= 3 N tmax, so the first part is
    within c u N tmax for c = 3 (N + 16); the sums themselves are the tighter bar."""
    _need_extended()
    y = np.asarray(y, np.float64)
    T, N = y.shape
    m = (np.ones(N) if ma is None else np.asarray(ma, np.float64)).astype(LD)
    lam = (np.asarray(tuning, np.float64) * np.float64(dt) + np.float64(RATE_EPS)).astype(LD)
    ym = y.astype(LD) * m[None, :]
    lg = np.log(lam)
    a1 = ym @ lg.T
    A1 = np.abs(ym) @ np.abs(lg).T
    a2 = (lam * m[None, :]).sum(1)
    g = np.array([[math.lgamma(v + 1.0) for v in row] for row in y], np.float64).astype(LD)
    G = (g * m[None, :]).sum(1)
    ll = a1 - a2[None, :] - G[:, None]
    bound = (N + 16) * U * (A1 + np.abs(a2)[None, :] + np.abs(G)[:, None]) + 4 * U * ym.sum(1)[:, None]
    return ll, bound.astype(np.float64)


# ----------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    family: str
    N: int
    T: int
    L: int
    dt: float
    mask: str               # 'none' | 'neuron' | 'latent'
    digits: np.ndarray
    zero: np.ndarray
    names: tuple
    tuning: np.ndarray
    y: np.ndarray
    ma: object               # (N,) float32 0/1 or None
    ml: object               # (L,) uint8 or None
    ref: Reference


# family, N, T, L, dt, mask: every N of a family with L at or above its pattern bank
# (A: 4 + 5 edges(N) rows; B: 7 + 50) at least once; every T and L once per family
CASES = (
    ('A', 130, 300, 100, 1.0, 'none'),
    ('A', 64, 257, 96, 0.02, 'none'),
    ('A', 63, 257, 37, 1.0, 'none'),
    ('A', 1, 300, 37, 0.02, 'none'),
    ('A', 130, 1, 1, 1.0, 'none'),
    ('A', 130, 257, 100, 0.02, 'latent'),
    ('B', 516, 300, 100, 1.0, 'none'),
    ('B', 516, 257, 96, 0.02, 'none'),
    ('B', 516, 1, 37, 1.0, 'none'),
    ('B', 516, 257, 1, 1.0, 'none'),
    ('B', 516, 257, 100, 1.0, 'neuron'),
    ('B', 516, 300, 96, 0.02, 'latent'),
    ('B', 512, 257, 96, 1.0, 'none'),
)


def case_id(c):
    return f"{c[0]}-N{c[1]}-T{c[2]}-L{c[3]}-dt{c[4]}-{c[5]}"


def bank_size(family, N):
    return 4 + (3 if family == 'B' else 0) + NDIG * len(edge_neurons(N))


@functools.lru_cache(maxsize=None)
def make_case(family, N, T, L, dt, mask):
    """Operands and reference of one case (cached: the host and the GPU tests share them;
    treat the arrays as read-only)."""
    seed = 1000 * N + 10 * L + T
    digits, zero, names = design_digits(N, L, family, seed)
    tuning = design_tuning(digits, zero, dt)
    y, t0 = design_counts(N, T, family, seed + 1)
    ma = ml = None
    l0 = L - 1
    if mask == 'neuron':
        # drops every third neuron, among them neurons that carry the largest count
        ma = (np.arange(N) % 3 != 1).astype(np.float32)
        assert np.any((y == COUNTS[family][-1]) & (ma == 0)[None, :])
    if mask == 'latent':
        # block 1 (latents 32..63) fully masked, block 2 partly; l0 stays unmasked
        ml = np.ones(L, np.uint8)
        ml[32:64] = 0
        ml[64:L - 1:3] = 0
        assert ml[l0] == 1
    ref = integer_reference(y, compose(digits), tuning, dt, t0, l0, ma)
    for a in (digits, zero, tuning, y, ref.S, ref.ll, ref.D, ref.bound_D, ref.bound_ll):
        a.setflags(write=False)
    return Case(family, N, T, L, dt, mask, digits, zero, tuple(names), tuning, y, ma, ml, ref)


def masked_view(case, a, fill):
    """a (T, L) with the case's masked latents replaced by fill."""
    if case.ml is None:
        return a
    return np.where(case.ml[None, :] != 0, a, fill)
