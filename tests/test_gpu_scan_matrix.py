"""Every (J latents per lane, WP band taps) instantiation of the banded forward filter,
smoother and relaxation kernels (csrc/fb_inst_j*_w*.hip: J in {1, 2, 4, 8, 16} x WP in
{5, 9, 13, 17, 25, 32}) against the float64 reference of tests/scan_ref.py, on a flat-band
transition whose outermost tap carries half the weight of its centre and data whose
latent uses the whole band (tests/test_scan_ref_host.py shows that a lost outer tap would
miss these bars by a factor >= 100 in every case).

Each pair makes two runs:
  ragged  L = 61 .. 1000 (partial last lane and 32-block), band = WP - 2 (< WP: g is
          zero-padded), chunk 16 without warm-up: every chunk boundary is verified and
          repaired by the relaxation kernel, and the last chunk is ragged;
  full    L = 64 J, band = WP, chunk 24 with an 8-step warm-up: the chunk-parallel main
          pass.
Bars: those of test_forward_backward_vs_oracle (tests/test_gpu_parity.py).

Tiny lines (L = 1, 2, 3, 8, 33 with band L - 1; band 0, mostly empty lanes, a last
32-block holding one latent) and the RBF transition at L = 8 (its band clamped to L - 1)
take the same checks at T = 40, chunk 16, no warm-up (repairs() is read, so a relaxation
time-out raises, but its counts are asserted in the ragged runs only).

Batched restarts at J >= 4 (blockIdx.y selects the restart, rows ldd = R L apart): each
restart bit-identical to its own single fit, as tests/test_gpu_restarts.py has it at J <= 2.
"""
import numpy as np
import pytest
import torch

from tests import scan_ref as S
from tests.test_gpu_parity import argmax_match, close_prob
from tests.test_gpu_restarts import _inits, _same
from tests.synth import make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def _run(run, rbf_mv=None):
    """One E-step through DeviceEM against scan_ref; returns repairs()."""
    from poor_man_gplvm_amd.engine import DeviceEM, ScanConfig, SpikeData
    L, T = run['L'], run['T']
    d, tr, (ref_gamma, ref_logz, ref_alpha, ref_logc) = S.scan_reference(L, run['band'], T, run['seed'],
                                                                         rbf_mv=rbf_mv)
    eng = DeviceEM(SpikeData(d['y']), L, basis=d['B'], scan=ScanConfig(chunk=run['chunk'], warmup=run['warmup']))
    eng.set_transition(tr)
    eng.set_ma_latent(None)
    eng.set_tuning(d['tuning'])
    logz = torch.zeros(1, dtype=torch.float64, device='cuda')
    gamma = torch.empty((T, 2, L), dtype=torch.float32, device='cuda')
    eng.e_step(1.0, logz, gamma=gamma)
    rep = eng.repairs()
    eng.scan_status()
    eng.emission_status()
    g = gamma.cpu().numpy()
    P = eng.P.cpu().numpy()
    alpha = eng.alpha.cpu().numpy()
    err = np.abs(g - ref_gamma) / (1e-5 * np.abs(ref_gamma) + 1e-12)
    print(f"L={L} band={tr.band} chunk={run['chunk']} warmup={run['warmup']} repairs={rep} "
          f"gamma err / bar {err.max():.3f} logZ rel {abs(logz.item() - ref_logz) / abs(ref_logz):.2e}")
    close_prob(g, ref_gamma)
    close_prob(g.sum(1), ref_gamma.sum(1))
    close_prob(P, ref_gamma.sum(1))
    if L > 1:                         # (a single latent has no runner-up to be clear of)
        argmax_match(g.sum(1), ref_gamma.sum(1))
    close_prob(alpha, ref_alpha)
    assert abs(logz.item() - ref_logz) <= 1e-7 * abs(ref_logz)
    np.testing.assert_allclose(eng.logc.cpu().numpy(), ref_logc, rtol=1e-6, atol=1e-5)
    return rep


@pytest.mark.parametrize("J,WP", S.SCAN_PAIRS)
def test_scan_pair(J, WP):
    runs = S.scan_runs(J, WP)
    f, b = _run(runs['ragged'])
    assert f > 0 and b > 0            # no warm-up: the relaxation kernel of this pair ran
    _run(runs['full'])


@pytest.mark.parametrize("L", S.TINY_L)
def test_tiny_line(L):
    _run(S.tiny_run(L))


def test_tiny_line_rbf_band_clamped_to_line():
    _run(dict(S.tiny_run(8), band=7), rbf_mv=1.0)


@pytest.mark.parametrize("L,mv", [(256, 2.0), (512, 3.0), (1024, 1.0)])
def test_batched_restarts_match_single_wide_lanes(L, mv):
    """run_em_restarts at J = 4, 8, 16: each restart equals run_em on the same segment grid
    (relax_segments = CUs // R) bit for bit."""
    from poor_man_gplvm_amd import AdamConfig, ScanConfig, banded_transition, run_em, run_em_restarts
    N, T, R = 16, 300, 2
    d = make(N, L, T, mv=mv)
    lps = _inits(T, L, R)
    kw = dict(n_iter=1, transition=banded_transition(L, mv), adam=AdamConfig(maxiter=20, tol=0.0))
    outs = run_em_restarts(d['y'], d['W0'], d['B'], lps, scan=ScanConfig(chunk=40, chunk_bwd=80), **kw)
    assert len(outs) == R
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sc1 = ScanConfig(chunk=40, chunk_bwd=80, relax_segments=max(1, cus // R))
    for r in range(R):
        ref, _ = run_em(d['y'], d['W0'], d['B'], lps[r], scan=sc1, **kw)
        _same(outs[r][0], ref)
        assert outs[r][1]['batched_restarts'] == R
    assert np.abs(outs[0][0]['tuning'] - outs[1][0]['tuning']).max() > 0
