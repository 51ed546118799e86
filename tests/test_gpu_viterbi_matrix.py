"""Every (J latents per lane, WP band taps) instantiation of the Viterbi forward kernel
(csrc/viterbi.hip: J in {1, 2, 4, 8, 16} x WP in {5, 9, 17, 32}) against the float64
reference, with conditions (a)-(d) of tests/test_gpu_viterbi.py (_check, unchanged).

The transition is the flat band of tests/scan_ref.py at band = WP - 2, so the kernels'
back-pointer code carries a non-zero shift (WP - band = 2), and the data's latent uses the
whole band: the reference MAP path takes steps of exactly +-band and jumps, and a
kernel that lost its outermost tap would lower the optimum by far more than the rounding
bound B (tests/test_scan_ref_host.py checks both for every case here).  The lines are
ragged (L = 61 .. 1000); T = 400 (300 at J = 16) lets the 0.5 % agreement cap admit 2 (1)
bins.  A has p = (0.05, 0.02); the cases whose band spans half the line or more take a
faster-switching A, without which no MAP path both steps by +-band and jumps
(scan_ref.VIT_INPUT).  The engine is driven directly (set_transition accepts any BandedTransition); the
log marginal of condition (d) is the float64 reference's.
"""
import numpy as np
import pytest
import torch

from tests import scan_ref as S
from tests import viterbi_ref as V
from tests.test_gpu_viterbi import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _decode(y, basis, tuning, tr, n_seq=1):
    """emission + viterbi of one engine: list of n_seq result dicts (decode_latent_viterbi's keys)."""
    from poor_man_gplvm_amd.engine import DeviceEM, SpikeData
    eng = DeviceEM(SpikeData(y), tr.L, basis=basis)
    eng.set_transition(tr)
    eng.set_ma_latent(None)
    eng.set_tuning(tuning)
    eng.emission(1.0)
    pd, pl, lj = eng.viterbi(1.0, n_seq)
    eng.emission_status()
    pd, pl, lj = pd.cpu().numpy(), pl.cpu().numpy(), lj.cpu().numpy()
    assert pd.shape == pl.shape == (n_seq, y.shape[0] // n_seq) and lj.shape == (n_seq,)
    return [dict(map_dynamics=pd[r], map_latent=pl[r], log_joint_map=float(lj[r])) for r in range(n_seq)]


def _logz(tr, u):
    return S.forward_backward(u, S.dense_K(tr), S.device_A(tr))[1]


def _case(run):
    d, tr, u = S.vit_inputs(run['L'], run['band'], run['T'], run['seed'], run['p'])
    res = _decode(d['y'], d['B'], d['tuning'], tr)[0]
    return _check(res, u, tr, _logz(tr, u))


@pytest.mark.parametrize("J,WP", S.VIT_PAIRS)
def test_viterbi_pair(J, WP):
    _case(S.vit_run(J, WP))


@pytest.mark.parametrize("L", S.VIT_TINY_L)
def test_viterbi_tiny_line(L):
    _case(S.vit_tiny_run(L))


def test_viterbi_single_latent():
    """L = 1 (band 0): both kernels are exactly 1, no datum separates the dynamics, so the
    path is held to feasibility (a), optimality (b) and its score (d), not to agreement
    with the reference's tie-breaks (c)."""
    T = 400
    d, tr, u = S.vit_inputs(1, 0, T, 0)
    res = _decode(d['y'], d['B'], d['tuning'], tr)[0]
    l, dyn = res['map_latent'], res['map_dynamics']
    assert l.shape == dyn.shape == (T,) and l.dtype == dyn.dtype == np.int32
    # (a)
    assert np.all(l == 0) and dyn.min() >= 0 and dyn.max() <= 1
    # (b)
    logK0, logA = V.banded_logK(tr), V.device_logA(tr)
    lp0 = V.log_pi0(logK0, logA)
    ref_path, ref_score = V.viterbi(u, logK0, logA, lp0)
    s_dev, M_dev = V.path_score(np.stack([dyn, l], axis=1), u, logK0, logA, lp0)
    s_ref, M_ref = V.path_score(ref_path, u, logK0, logA, lp0)
    assert abs(s_ref - ref_score) <= 1e-9 * abs(ref_score)
    B = 16.0 * T * 2.0 ** -24 * max(M_dev, M_ref)
    lj, logz = res['log_joint_map'], _logz(tr, u)
    print(f"L=1 score_ref={s_ref:.6f} gap={s_ref - s_dev:.3e} B={B:.3e} lj-score={lj - s_dev:.3e}")
    assert np.isfinite(s_dev) and s_ref - s_dev <= B
    # (d)
    assert abs(lj - s_dev) <= B
    assert lj <= logz + 1e-6 * abs(logz)


def test_batched_sequences_wide_lanes_bit_for_bit():
    """viterbi(n_seq=2) at L = 1000 (J = 16), flat band 30: two sequences stacked in time in
    one engine, each equal to its own single-sequence call bit for bit."""
    L, band, T = 1000, 30, 300
    ds = [S.wide_step_data(S.N_NEURON, L, T, band, seed) for seed in (0, 10)]
    tr = S.flat_transition(L, band)
    B, tun = ds[0]['B'], ds[0]['tuning']
    both = _decode(np.concatenate([d['y'] for d in ds]), B, tun, tr, n_seq=2)
    for r in range(2):
        one = _decode(ds[r]['y'], B, tun, tr)[0]
        assert np.array_equal(one['map_dynamics'], both[r]['map_dynamics'])
        assert np.array_equal(one['map_latent'], both[r]['map_latent'])
        assert one['log_joint_map'] == both[r]['log_joint_map']
    assert both[0]['log_joint_map'] != both[1]['log_joint_map']
    assert not np.array_equal(both[0]['map_latent'], both[1]['map_latent'])
