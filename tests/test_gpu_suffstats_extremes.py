"""The suff-stats GEMMs y_w = P^T y, t_w = sum_t P at the count extreme of the integer
paths and on a posterior with dynamic range: counts from {0, 1, 126, 127} (127 is the
largest count the bf16 eligibility flag lets through), P rows peaked as a decode
produces them -- one entry near 1, a geometric tail down to 1e-30, exact zeros beyond it,
and one latent column that is zero at every t.  The three device paths and the bars of
test_gpu_parity.test_suffstats_vs_numpy (rtol 1e-6, atol 1e-9 on y_w; rtol 1e-6 on t_w,
against f64 numpy; `planes` bit-identical to `bf16x3`); the all-zero column exactly 0.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_parity import split_planes

pytestmark = pytest.mark.gpu
ZERO_COL = 7


@pytest.fixture(scope="module", autouse=True)
def _dev():
    torch.cuda.set_device(0)


def peaked_posterior(T, L, seed):
    """(T, L) float32: row t peaks at a random latent with weight near 1 and falls by a
    constant ratio per step on both sides, reaching 1e-30 after K_t steps (K_t from
    {5, 10, 20, 30}), exactly 0 beyond; column ZERO_COL is 0 everywhere."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, L, size=T)
    K = rng.choice([5, 10, 20, 30], size=T)
    rho = 1e-30 ** (1.0 / K)
    k = np.abs(np.arange(L)[None, :] - c[:, None])
    P = np.where(k <= K[:, None], rho[:, None] ** k, 0.0)
    P /= P.sum(1, keepdims=True)
    P = P.astype(np.float32)
    P[:, ZERO_COL] = 0.0
    return P


@pytest.mark.parametrize("path", ["f32", "bf16x3", "planes"])
@pytest.mark.parametrize("N,L,T", [(70, 96, 3000), (5, 40, 65)])
def test_suffstats_count_extreme_peaked_posterior(path, N, L, T):
    from poor_man_gplvm_amd import _native as nat
    from poor_man_gplvm_amd.engine import DeviceEM, SpikeData
    rng = np.random.default_rng(11)
    y = rng.choice([0, 1, 126, 127], size=(T, N), p=(0.4, 0.2, 0.2, 0.2)).astype(np.float32)
    y[0] = 127
    P = peaked_posterior(T, L, 12)
    pos = P[P > 0]
    assert P.max() > 0.9 and pos.min() < 1e-29 and pos.min() > 1e-37 and np.mean(P == 0) > 0.2
    sp = SpikeData(y)
    assert sp.int_path and sp.ybt is not None
    eng = DeviceEM(sp, L)
    eng.P.copy_(torch.as_tensor(P, device='cuda'))
    eng.yw.fill_(float('nan'))
    eng.tw.fill_(float('nan'))
    if path == "f32":
        ws = torch.empty(int(eng.lib.pmg_suffstats_workspace_size(T, L, sp.Np)), dtype=torch.uint8, device='cuda')
        rc = eng.lib.pmg_suffstats(nat.ptr(eng.P), nat.ptr(sp.yext), T, L, N, sp.Np, nat.ptr(eng.yw),
                                   nat.ptr(eng.tw), nat.ptr(ws), ws.numel(), nat.stream_handle())
    else:
        ws = torch.empty(int(eng.lib.pmg_suffstats_bf16_workspace_size(T, L, N)), dtype=torch.uint8, device='cuda')
        rc = eng.lib.pmg_suffstats_bf16(nat.ptr(eng.P), nat.ptr(sp.ybt), T, sp.Tp, L, N, sp.Np, nat.ptr(eng.yw),
                                        nat.ptr(eng.tw), nat.ptr(ws), ws.numel(), nat.stream_handle())
    nat.check(rc, "suffstats")
    if path == "planes":
        yw_split = eng.yw.cpu().numpy().copy()
        Pq = torch.as_tensor(split_planes(P), device='cuda')
        ws = torch.empty(int(eng.lib.pmg_suffstats_bf16x3_workspace_size(T, L, N)), dtype=torch.uint8,
                         device='cuda')
        eng.yw.fill_(float('nan'))
        eng.tw.fill_(float('nan'))
        nat.check(eng.lib.pmg_suffstats_bf16x3(nat.ptr(Pq), L, nat.ptr(sp.ybt), T, sp.Tp, L, N, sp.Np,
                                               nat.ptr(eng.yw), nat.ptr(eng.tw), nat.ptr(ws), ws.numel(),
                                               nat.stream_handle()), "suffstats_bf16x3")
        np.testing.assert_array_equal(eng.yw.cpu().numpy(), yw_split)
    P64 = P.astype(np.float64)
    yw, tw = P64.T @ y.astype(np.float64), P64.sum(0)
    got_yw, got_tw = eng.yw.cpu().numpy(), eng.tw.cpu().numpy()
    print(f"y_w max rel err {np.max(np.abs(got_yw - yw) / np.maximum(yw, 1e-300)):.3e}, "
          f"t_w max rel err {np.max(np.abs(got_tw - tw) / np.maximum(tw, 1e-300)):.3e}")
    np.testing.assert_allclose(got_yw, yw, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got_tw, tw, rtol=1e-6)
    assert np.all(got_yw[ZERO_COL] == 0.0) and got_tw[ZERO_COL] == 0.0
