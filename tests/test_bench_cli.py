"""bench.py's command line: a plain run prints the headline line only and --full adds the
rest; --dump-outputs writes the last timed iteration's arrays.  The argument checks run on
the CPU, the two bench runs at the smallest configuration (C1) on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "rooflines", "kernels_ms", "kernel_calls", "ms_per_step_instrumented", "fit_em_api",
             "cpu_baseline", "decode_latent")


def _bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=180, env=env, cwd=ROOT)


def _line(out):
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("args", [("--steps", "0"), ("--decode",),
                                  ("--dump-outputs", "x", "--restarts", "8"),
                                  ("--dump-outputs", "x", "--shard", "time")])
def test_rejected_arguments(args):
    out = _bench("--gpus", "1", *args)
    assert out.returncode == 2 and "error" in out.stderr     # argparse, before any GPU work


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    d = tmp_path / "dump"
    r = _line(_bench("--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d)))
    for k in HEADLINE:
        assert k in r, k
    for k in FULL_ONLY:
        assert k not in r, k
    assert r["steps"] == 3 and r["warmup"] == 2 and r["fresh_fit"]["iterations"] == 5
    assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] / 1e3 - 1.0) < 1e-9
    N, T, L = 30, 1000, 100
    a = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    nb = a["params"].shape[0]
    assert a["params"].shape == (nb, N) and a["tuning"].shape == (L, N)
    assert a["suffstats_yw"].shape == (L, N) and a["suffstats_tw"].shape == (L,)
    assert a["posterior_latent_marg"].shape == (T, L)
    assert np.array_equal(a["posterior_latent_marg_rows"], np.arange(T))
    assert a["log_marginal"].shape == (5,) and a["log_marginal"][-1] == r["log_marginal_last"]
    assert all(np.isfinite(v).all() for v in a.values())
    # a posterior marginal per time step, and the last M-step's statistics of the one before
    assert np.abs(a["posterior_latent_marg"].sum(1) - 1.0).max() < 1e-4
    assert abs(a["suffstats_tw"].sum() - T) < 1e-3 * T
    assert a["adam_stats"][0] == np.count_nonzero(a["adam_loss_history"])


@pytest.mark.gpu
def test_full_run_keeps_the_other_legs():
    r = _line(_bench("--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", "2", "--full"))
    for k in HEADLINE + FULL_ONLY[:5] + ("fit_em_api", "cpu_baseline"):
        assert k in r, k
    assert r["steps"] == 3 and r["kernel_calls"]["forward_filter"] == 3
