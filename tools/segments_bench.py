"""Time of decode_latent_segments on many short events at the C3 shape (N = 512, L = 512),
against the route available without it: one decode_marginals call per event.

S events (--events, default 2000) with geometric lengths of mean 25 clipped to [3, 200]
(fixed seed) are cut from bench.synth's seeded recording.  Reported: the wall time of one
decode_latent_segments call (best of --calls after --warmup), its device time by section
(KernelTimer), the wall time of a loop of decode_marginals calls over the first 50 events
scaled to S, and the ratio of the two.  Prints one JSON line and writes it to
profiles/segments_bench_c3.json (--json).

--crossover: one segment of 256, 1024, 4096, 16384 and 65536 rows through both routes of
decode_latent_segments -- one wave (ScanConfig.segment_wave_max above the length) and the
chunk-parallel scans (segment_wave_max = 1) -- and the largest power of two at which the
one-wave route is not slower (wall time, best of --calls); written to
profiles/segments_crossover_c3.json.  ScanConfig.segment_wave_max's default cites it.

--viterbi: the same event set through decode_latent_segments_viterbi (one call; wall time,
device time by section) against a loop of decode_latent_viterbi calls over the first 50
events scaled to S; written to profiles/segments_viterbi_bench_c3.json.  The loop is the
baseline: no ratio is fixed.

--sample R: the same event set through sample_latent_segments with R samples per event (one
call; wall time, device time by section, the sampler kernel's share) next to
decode_latent_segments on the same events in the same process, the yardstick: the smoother
pays a backward pass and 2 L floats per row, the sampler R backward draws.  --parent-json: a
record that the parent commit's tools/segments_bench.py wrote on the same machine, kept
under "parent_commit".  Written to profiles/segments_sample_bench_c3.json.  No time is
fixed: the ratio is reported as found.

--shuffle R [--shuffle-kind time_bin|column_cycle|both]: the same event set through
shuffle_test_segments with R shuffles per event (wall time of every timed call, device time by
section, the kernel's ns per filter step), next to a loop over the calls the project already
has: per shuffle a row gather of delta / phi / m with torch, then segment_smoother forward only.
The loop runs --loop-shuffles shuffles (default 50; fewer than R means a subset, scaled to R and
flagged in the record), on the same shuffles as one segment_shuffle_logz call, and the largest
difference between the two is recorded (0 for time_bin; a rotation's loop has to fold the block
references into delta, so it differs by float32 rounding).  Written to
profiles/segments_shuffle_bench_c3.json.  No ratio is fixed.

--shuffle R --shuffle-kind neuron_circular: the per-neuron circular spike shuffle, which needs a
new emission per shuffle.  Recorded: the one call (every timed call's wall time with min,
median and max, device time by section); the only route without it, a loop of a host roll plus
decode_latent_segments per shuffle, timed on --loop-shuffles shuffles (20 here) and scaled;
and, for the roll kernel alone, the route it replaces on the same rows -- a segment-aware torch
gather of f32 y into the stacked tensor, then SpikeData.refresh() -- with the two routes' yq and
gconst compared bit for bit.  Device time per kernel comes from running this tool under
rocprofv3 --kernel-trace --stats (--no-loop skips everything but the one call).  Written to
profiles/segments_shuffle_bench_c3_neuron_circular.json.  No ratio is fixed.

--exact: the same event set through decode_latent_segments(exact=True) (the dense log-domain
scans, one workgroup per event): every timed call's wall time, device time by section (the
kernel is the segment_smoother_dense section), next to the only route without it, a loop of
decode_latent calls over the first --loop-events events (default 30) scaled to S; the largest
difference between the two, and whether the events of up to 64 rows (which the public loop runs
as a single chunk too) are equal bit for bit.  Written to profiles/segments_exact_bench_c3.json.
No ratio is fixed.

--exact --crossover: one event of 16 .. 2048 rows through both routes of
decode_latent_segments(exact=True) -- one workgroup and the chunk-parallel dense scans -- and
the largest power of two at which one workgroup is not slower; written to
profiles/segments_exact_crossover_c3.json.  ScanConfig.segment_dense_max cites it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import poor_man_gplvm_amd as P  # noqa: E402
from poor_man_gplvm_amd.engine import KernelTimer, ScanConfig  # noqa: E402

N, L = 512, 512
CROSSOVER_LENGTHS = (256, 1024, 4096, 16384, 65536)


def event_intervals(S, T, seed=0):
    """(S, 2) [start, stop) rows: geometric lengths (mean 25) clipped to [3, 200], uniform starts."""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.geometric(1.0 / 25.0, size=S), 3, 200)
    start = rng.integers(0, T - lens + 1)
    return np.stack([start, start + lens], 1).astype(np.int64)


def model(timer=None, **scan):
    m = P.PoissonGPLVMJump1D(N, n_latent_bin=L, tuning_lengthscale=10., movement_variance=1.,
                             scan_config=ScanConfig(**scan))
    if timer is not None:       # every engine the decode builds reports to the timer
        make = m._engine_on

        def with_timer(*a, **k):
            eng = make(*a, **k)
            eng.timer = timer
            return eng
        m._engine_on = with_timer
    return m


def wall_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    best = float('inf')
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, 1e3 * (time.perf_counter() - t0))
    return best


def sections_ms(timer):
    return {k: round(n * ms, 4) for k, (n, ms) in sorted(timer.summary().items())}


def save(path, rec):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def run_events(args, y, tun):
    seg = event_intervals(args.events, y.shape[0])
    m = model()
    one = wall_ms(lambda: m.decode_latent_segments(y, seg, tuning=tun), args.calls, args.warmup)
    timer = KernelTimer()
    mt = model(timer)
    mt.decode_latent_segments(y, seg, tuning=tun)
    kern = sections_ms(timer)
    n_loop = min(50, len(seg))

    def loop():
        for a, b in seg[:n_loop]:
            m.decode_marginals(y[a:b], tuning=tun)
    per_event = wall_ms(loop, max(1, args.calls // 2), 1) / n_loop
    loop_ms = per_event * len(seg)
    return {"shape": "c3", "N": N, "L": L, "events": int(len(seg)), "rows": int((seg[:, 1] - seg[:, 0]).sum()),
            "mean_length": round(float((seg[:, 1] - seg[:, 0]).mean()), 2),
            "decode_latent_segments_wall_ms": round(one, 3), "decode_latent_segments_kernel_ms": kern,
            "decode_marginals_per_event_wall_ms": round(per_event, 3), "loop_events_timed": n_loop,
            "decode_marginals_loop_wall_ms_scaled": round(loop_ms, 1),
            "loop_over_one_call": round(loop_ms / one, 1)}


def run_viterbi(args, y, tun):
    seg = event_intervals(args.events, y.shape[0])
    m = model()
    one = wall_ms(lambda: m.decode_latent_segments_viterbi(y, seg, tuning=tun), args.calls, args.warmup)
    timer = KernelTimer()
    mt = model(timer)
    res = mt.decode_latent_segments_viterbi(y, seg, tuning=tun)
    kern = sections_ms(timer)
    n_loop = min(50, len(seg))
    singles = []

    def loop():
        singles[:] = [m.decode_latent_viterbi(y[a:b], tuning=tun) for a, b in seg[:n_loop]]
    per_event = wall_ms(loop, max(1, args.calls // 2), 1) / n_loop
    loop_ms = per_event * len(seg)
    off = res['segment_offsets']
    same = all(np.array_equal(r['map_latent'], res['map_latent'][off[s]:off[s + 1]]) and
               np.array_equal(r['map_dynamics'], res['map_dynamics'][off[s]:off[s + 1]]) and
               r['log_joint_map'] == res['log_joint_map'][s] for s, r in enumerate(singles))
    return {"shape": "c3", "N": N, "L": L, "events": int(len(seg)), "rows": int((seg[:, 1] - seg[:, 0]).sum()),
            "mean_length": round(float((seg[:, 1] - seg[:, 0]).mean()), 2),
            "decode_latent_segments_viterbi_wall_ms": round(one, 3),
            "decode_latent_segments_viterbi_kernel_ms": kern,
            "kernel_ms_total": round(sum(kern.values()), 4),
            "decode_latent_viterbi_per_event_wall_ms": round(per_event, 3), "loop_events_timed": n_loop,
            "decode_latent_viterbi_loop_wall_ms_scaled": round(loop_ms, 1),
            "loop_over_one_call": round(loop_ms / one, 1),
            "loop_events_equal_bit_for_bit": bool(same),
            "log_joint_map_sum": float(res['log_joint_map'].sum())}


def run_sample(args, y, tun):
    seg = event_intervals(args.events, y.shape[0])
    n = int(args.sample)
    m = model()
    one = wall_ms(lambda: m.sample_latent_segments(y, seg, n_samples=n, key=0, tuning=tun), args.calls, args.warmup)
    timer = KernelTimer()
    mt = model(timer)
    res = mt.sample_latent_segments(y, seg, n_samples=n, key=0, tuning=tun)
    kern = sections_ms(timer)
    smooth = wall_ms(lambda: m.decode_latent_segments(y, seg, tuning=tun), args.calls, args.warmup)
    timer.reset()
    mt.decode_latent_segments(y, seg, tuning=tun)
    kern_smooth = sections_ms(timer)
    rows = int((seg[:, 1] - seg[:, 0]).sum())
    pd, pl = res['sample_dynamics'], res['sample_latent']
    rec = {"shape": "c3", "N": N, "L": L, "events": int(len(seg)), "rows": rows, "n_samples": n,
           "mean_length": round(float((seg[:, 1] - seg[:, 0]).mean()), 2),
           "sample_latent_segments_wall_ms": round(one, 3), "sample_latent_segments_kernel_ms": kern,
           "kernel_ms_total": round(sum(kern.values()), 4),
           "segment_sampler_ns_per_drawn_state": round(1e6 * kern.get("segment_sampler", 0.0) / (rows * n), 4),
           "decode_latent_segments_wall_ms": round(smooth, 3), "decode_latent_segments_kernel_ms": kern_smooth,
           "decode_latent_segments_kernel_ms_total": round(sum(kern_smooth.values()), 4),
           "sample_over_decode_wall": round(one / smooth, 3),
           "sample_over_decode_kernel": round(sum(kern.values()) / sum(kern_smooth.values()), 3),
           "all_states_drawn": bool(pd.min() >= 0 and pl.min() >= 0),
           "mean_jump_fraction": round(float((pd == 1).mean()), 6)}
    if args.parent_json:
        with open(args.parent_json) as f:
            rec["parent_commit"] = json.load(f)
    return rec


def wall_all_ms(fn, calls, warmup):
    """Every timed call's wall time (ms), for the spread."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def run_shuffle(args, y, tun):
    from poor_man_gplvm_amd.core import gather_segments, segment_order, segment_permutations
    seg = event_intervals(args.events, y.shape[0])
    R, kind = int(args.shuffle), args.shuffle_kind
    m = model()
    walls = wall_all_ms(lambda: m.shuffle_test_segments(y, seg, n_shuffle=R, shuffle=kind, key=0, tuning=tun),
                        args.calls, args.warmup)
    timer = KernelTimer()
    mt = model(timer)
    res = mt.shuffle_test_segments(y, seg, n_shuffle=R, shuffle=kind, key=0, tuning=tun)
    kern = sections_ms(timer)
    # the loop the project's other calls allow, over the same shuffles: per shuffle a row gather
    # of delta / phi / m (a rotation needs the block references folded into delta first), then
    # segment_smoother forward only
    n_loop = min(R, int(args.loop_shuffles))
    yc, off, ma = gather_segments(y, seg, None)
    Ttot = int(off[-1])
    eng = m._decode_engine(yc, tun, m._decode_hp({}), ma, m.ma_latent_default, exact=False)
    dev = eng.dev
    eng.emission(1.0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    perm = segment_permutations(off, n_loop, gen, dev) if kind != 'column_cycle' else None
    rot = (torch.randint(0, L, (n_loop, Ttot), generator=gen, dtype=torch.int32, device=dev)
           if kind != 'time_bin' else None)
    off_d = torch.as_tensor(off, device=dev)
    order_d = torch.as_tensor(segment_order(off), device=dev)
    fused = eng.segment_shuffle_logz(1.0, off_d, order_d, perm=perm, rot=rot, n_shuffle=n_loop)
    d0, p0, m0 = eng.delta.clone(), eng.phi.clone(), eng.mref.clone()
    lat = torch.arange(L, device=dev)[None, :]
    looped = torch.empty_like(fused)

    def loop():
        for r in range(n_loop):
            idx = perm[r].long() if perm is not None else slice(None)
            if rot is None:
                eng.delta.copy_(d0[idx])
                eng.phi.copy_(p0[idx])
            else:
                full = d0[idx] + torch.repeat_interleave(p0[idx], 32, dim=1)[:, :L]
                eng.delta.copy_(torch.gather(full, 1, (lat + rot[r].long()[:, None]) % L))
                eng.phi.zero_()
            eng.mref.copy_(m0[idx])
            looped[r] = eng.segment_smoother(1.0, off_d, order_d)[2]
    loop_walls = wall_all_ms(loop, max(1, args.calls // 2), 1)
    per_shuffle = min(loop_walls) / n_loop
    diff = float((looped - fused).abs().max())
    rel = float(((looped - fused).abs() / fused.abs()).max())
    rows = int((seg[:, 1] - seg[:, 0]).sum())
    k_ms = kern.get("segment_shuffle_logz", 0.0)
    return {"shape": "c3", "N": N, "L": L, "events": int(len(seg)), "rows": rows, "n_shuffle": R,
            "shuffle": kind, "mean_length": round(float((seg[:, 1] - seg[:, 0]).mean()), 2),
            "shuffle_test_segments_wall_ms": round(min(walls), 3),
            "shuffle_test_segments_wall_ms_all": [round(w, 3) for w in walls],
            "shuffle_test_segments_kernel_ms": kern, "kernel_ms_total": round(sum(kern.values()), 4),
            "segment_shuffle_logz_ns_per_step": round(1e6 * k_ms / (rows * (R + 1)), 4),
            "loop_shuffles_timed": n_loop, "loop_is_a_subset_scaled_to_n_shuffle": bool(n_loop < R),
            "loop_per_shuffle_wall_ms": round(per_shuffle, 4),
            "loop_wall_ms_all": [round(w, 3) for w in loop_walls],
            "loop_wall_ms_scaled": round(per_shuffle * R, 1),
            "loop_over_one_call": round(per_shuffle * R / min(walls), 2),
            "loop_vs_kernel_max_abs_diff": diff, "loop_vs_kernel_max_rel_diff": rel,
            "p_value_min": float(res['p_value'].min()), "p_value_median": float(np.median(res['p_value']))}


def host_roll(yc, off, shift):
    """roll_segments of the whole compact array at once: row t of event s takes row
    a_s + (t - a_s - shift[s, n]) mod len_s of neuron n."""
    lens = np.diff(off)
    seg_of = np.repeat(np.arange(len(lens)), lens)
    a, ln = off[:-1][seg_of][:, None], lens[seg_of][:, None]
    rel = np.arange(int(off[-1]))[:, None] - a
    return np.take_along_axis(yc, a + (rel - shift[seg_of]) % ln, axis=0)


def run_neuron_shuffle(args, y, tun):
    from poor_man_gplvm_amd.core import gather_segments, segment_neuron_shifts
    from poor_man_gplvm_amd.engine import SpikeData
    seg = event_intervals(args.events, y.shape[0])
    R = int(args.shuffle)
    m = model()
    call = lambda: m.shuffle_test_segments(y, seg, n_shuffle=R, shuffle='neuron_circular', key=0, tuning=tun)  # noqa: E731
    walls = wall_all_ms(call, args.calls, args.warmup)
    rows = int((seg[:, 1] - seg[:, 0]).sum())
    yc, off, _ = gather_segments(y, seg, None)
    rec = {"shape": "c3", "N": N, "L": L, "events": int(len(seg)), "rows": rows, "n_shuffle": R,
           "shuffle": "neuron_circular", "mean_length": round(float((seg[:, 1] - seg[:, 0]).mean()), 2),
           "shuffles_per_launch": int(m._shuffle_neuron_batch(rows, len(seg), N, R, False)),
           "shuffle_test_segments_wall_ms_all": [round(w, 3) for w in walls],
           "shuffle_test_segments_wall_ms_min": round(min(walls), 3),
           "shuffle_test_segments_wall_ms_median": round(float(np.median(walls)), 3),
           "shuffle_test_segments_wall_ms_max": round(max(walls), 3),
           "estimate_in_the_issue_ms_per_1000_shuffles": 100.0}
    if args.no_loop:
        return rec
    timer = KernelTimer()
    res = model(timer).shuffle_test_segments(y, seg, n_shuffle=R, shuffle='neuron_circular', key=0, tuning=tun)
    kern = sections_ms(timer)
    rec.update({"shuffle_test_segments_section_ms": kern, "section_ms_total": round(sum(kern.values()), 4),
                "section_ms_per_shuffle": {k: round(v / (R + 1), 5) for k, v in kern.items()},
                "p_value_min": float(res['p_value'].min()), "p_value_median": float(np.median(res['p_value']))})
    # the only route without the kernel: per shuffle a host roll and a decode_latent_segments call
    n_loop = min(R, int(args.loop_shuffles))
    dev = torch.device('cuda', torch.cuda.current_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    shift_d = segment_neuron_shifts(off, n_loop, N, 0, gen, dev)
    shift = shift_d.cpu().numpy().astype(np.int64)
    looped = np.empty((n_loop, len(seg)))

    def loop():
        for r in range(n_loop):
            yr = host_roll(yc, off, shift[r])
            looped[r] = m.decode_latent_segments(yr, np.stack([off[:-1], off[1:]], 1), tuning=tun)['log_marginal_final']
    loop_walls = wall_all_ms(loop, 1, 0)
    own = m.shuffle_test_segments(y, seg, n_shuffle=n_loop, shift=shift_d, tuning=tun)['log_marginal_shuffle']
    per_shuffle = min(loop_walls) / n_loop
    rec.update({"loop_shuffles_timed": n_loop, "loop_is_a_subset_scaled_to_n_shuffle": bool(n_loop < R),
                "loop_per_shuffle_wall_ms": round(per_shuffle, 3), "loop_wall_ms_scaled": round(per_shuffle * R, 1),
                "loop_over_one_call_median": round(per_shuffle * R / float(np.median(walls)), 2),
                "loop_vs_one_call_bits_equal": bool(np.array_equal(looped, own))})
    # the roll kernel alone against the route it replaces on the same rows
    src = SpikeData(yc, None)
    nb = min(8, n_loop)
    off_d = torch.as_tensor(off, device=dev)
    sh = shift_d[:nb].contiguous()
    sp = SpikeData.rolled(src, off_d, sh)
    lens = torch.as_tensor(np.diff(off), device=dev)
    seg_of = torch.repeat_interleave(torch.arange(len(seg), device=dev), lens)
    a_t, ln_t = off_d[:-1][seg_of][:, None], lens[seg_of][:, None]
    rel = torch.arange(rows, device=dev)[:, None] - a_t
    stacked = SpikeData(torch.zeros((nb * rows, N), dtype=torch.float32, device=dev), None)

    def gather_refresh():
        for r in range(nb):
            idx = a_t + torch.remainder(rel - sh[r].long()[seg_of], ln_t)
            stacked.y[r * rows:(r + 1) * rows] = torch.gather(src.y, 0, idx)
        stacked.refresh()

    def event_ms(fn, n=5):
        out = []
        for _ in range(n + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out[1:]
    k_ms = event_ms(lambda: sp.roll(src, off_d, sh))
    g_ms = event_ms(gather_refresh)
    same = bool(torch.equal(sp.yq, stacked.yq) and torch.equal(sp.gconst.view(torch.int64),
                                                                stacked.gconst.view(torch.int64)))
    rec.update({"roll_kernel_copies": nb,
                "roll_kernel_ms_all": [round(v, 4) for v in k_ms], "roll_kernel_ms_median": round(float(np.median(k_ms)), 4),
                "roll_kernel_us_per_shuffle": round(1e3 * float(np.median(k_ms)) / nb, 2),
                "gather_refresh_ms_all": [round(v, 4) for v in g_ms],
                "gather_refresh_ms_median": round(float(np.median(g_ms)), 4),
                "gather_refresh_over_roll_kernel": round(float(np.median(g_ms) / np.median(k_ms)), 2),
                "roll_kernel_equals_gather_refresh_bits": same})
    return rec


EXACT_CROSSOVER_LENGTHS = (16, 32, 64, 128, 256, 512, 1024, 2048)
EXACT_KEYS = ('posterior_all', 'log_posterior_all', 'log_one_step_predictive_marginals_all')


def run_exact(args, y, tun):
    """decode_latent_segments(exact=True) against the only route without it: a loop of
    decode_latent calls, one per event (timed on the first --loop-events events, scaled)."""
    seg = event_intervals(args.events, y.shape[0])
    lens = seg[:, 1] - seg[:, 0]
    m = model()
    walls = wall_all_ms(lambda: m.decode_latent_segments(y, seg, tuning=tun, exact=True), args.calls, args.warmup)
    timer = KernelTimer()
    res = model(timer).decode_latent_segments(y, seg, tuning=tun, exact=True)
    kern = sections_ms(timer)
    # the same call with every event on one workgroup, whatever its length (the default sends
    # the events beyond ScanConfig.segment_dense_max rows to the chunk-parallel dense scans)
    big = 1 << 30
    m_all = model(segment_wave_max=big, segment_dense_max=big)
    walls_all = wall_all_ms(lambda: m_all.decode_latent_segments(y, seg, tuning=tun, exact=True), args.calls,
                            args.warmup)
    timer_all = KernelTimer()
    model(timer_all, segment_wave_max=big, segment_dense_max=big).decode_latent_segments(y, seg, tuning=tun, exact=True)
    kern_all = sections_ms(timer_all)
    n_loop = min(int(args.loop_events), len(seg))
    singles = []

    def loop():
        singles[:] = [m.decode_latent(y[a:b], tuning=tun) for a, b in seg[:n_loop]]
    loop_walls = wall_all_ms(loop, 1, 0)
    per_event = min(loop_walls) / n_loop
    off = res['segment_offsets']
    same, diff, lz_rel = [], 0.0, 0.0
    for s, r in enumerate(singles):
        sl = slice(int(off[s]), int(off[s + 1]))
        same.append(bool(all(np.array_equal(r[k], res[k][sl]) for k in EXACT_KEYS)
                         and r['log_marginal_final'] == res['log_marginal_final'][s]))
        diff = max(diff, float(np.abs(r['posterior_all'].astype(np.float64) - res['posterior_all'][sl]).max()))
        lz_rel = max(lz_rel, abs(r['log_marginal_final'] - res['log_marginal_final'][s]) / abs(r['log_marginal_final']))
    short = lens[:n_loop] <= 64      # the public loop runs these as a single chunk too
    k_ms = kern.get("segment_smoother_dense", 0.0)
    rows = int(lens.sum())
    return {"shape": "c3", "N": N, "L": L, "events": int(len(seg)), "rows": rows,
            "mean_length": round(float(lens.mean()), 2), "max_length": int(lens.max()),
            "decode_latent_segments_exact_wall_ms": round(min(walls), 3),
            "decode_latent_segments_exact_wall_ms_all": [round(w, 3) for w in walls],
            "decode_latent_segments_exact_kernel_ms": kern, "kernel_ms_total": round(sum(kern.values()), 4),
            "segment_smoother_dense_ms": round(k_ms, 4),
            "segment_smoother_dense_us_per_row": round(1e3 * k_ms / rows, 4),
            "segment_dense_max": int(m.scan_config.segment_dense_max),
            "events_beyond_segment_dense_max": int((lens > m.scan_config.segment_dense_max).sum()),
            "all_on_one_workgroup_wall_ms_all": [round(w, 3) for w in walls_all],
            "all_on_one_workgroup_kernel_ms": kern_all,
            "decode_latent_per_event_wall_ms": round(per_event, 3), "loop_events_timed": n_loop,
            "decode_latent_loop_wall_ms_scaled": round(per_event * len(seg), 1),
            "loop_over_one_call": round(per_event * len(seg) / min(walls), 1),
            "loop_vs_call_max_abs_posterior_diff": diff, "loop_vs_call_max_rel_logz_diff": lz_rel,
            "loop_events_up_to_64_rows": int(short.sum()),
            "loop_events_up_to_64_rows_equal_bit_for_bit": bool(np.all(np.asarray(same)[short])),
            "loop_events_equal_bit_for_bit": int(np.sum(same))}


def run_exact_crossover(args, y, tun):
    """One event of n rows through both routes of decode_latent_segments(exact=True): one
    workgroup (both segment limits above the length) and the chunk-parallel dense scans
    (segment_wave_max = 1)."""
    table, best = [], 0
    big = 1 << 30
    for n in EXACT_CROSSOVER_LENGTHS:
        seg = np.array([[0, n]])
        row = {"length": n}
        for name, scan in (("one_workgroup", dict(segment_wave_max=big, segment_dense_max=big)),
                           ("chunk_parallel", dict(segment_wave_max=1))):
            timer = KernelTimer()
            m = model(timer, **scan)
            row[name + "_wall_ms"] = round(wall_ms(lambda: m.decode_latent_segments(y, seg, tuning=tun, exact=True),
                                                   args.calls, args.warmup), 3)
            timer.reset()
            m.decode_latent_segments(y, seg, tuning=tun, exact=True)
            row[name + "_kernel_ms"] = sections_ms(timer)
        table.append(row)
    for row in table:           # the largest length up to which one workgroup was never slower
        if row["one_workgroup_wall_ms"] <= row["chunk_parallel_wall_ms"]:
            best = row["length"]
        else:
            break
    return {"shape": "c3", "N": N, "L": L, "table": table, "one_workgroup_not_slower_up_to": best,
            "rule": "wall time of one decode_latent_segments(exact=True) call, best of --calls; lengths are "
                    "powers of two"}


def run_crossover(args, y, tun):
    table, best = [], 0
    for n in CROSSOVER_LENGTHS:
        seg = np.array([[0, n]])
        row = {"length": n}
        for name, wave_max in (("one_wave", 1 << 30), ("chunk_parallel", 1)):
            timer = KernelTimer()
            m = model(timer, segment_wave_max=wave_max)
            row[name + "_wall_ms"] = round(wall_ms(lambda: m.decode_latent_segments(y, seg, tuning=tun), args.calls,
                                                   args.warmup), 3)
            timer.reset()
            m.decode_latent_segments(y, seg, tuning=tun)
            row[name + "_kernel_ms"] = sections_ms(timer)
        table.append(row)
    for row in table:           # the largest length up to which one wave was never slower
        if row["one_wave_wall_ms"] <= row["chunk_parallel_wall_ms"]:
            best = row["length"]
        else:
            break
    return {"shape": "c3", "N": N, "L": L, "table": table, "one_wave_not_slower_up_to": best,
            "rule": "wall time of one decode_latent_segments call, best of --calls; lengths are powers of two"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--viterbi", action="store_true")
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--loop-events", type=int, default=30)
    ap.add_argument("--sample", type=int, default=0, metavar="R")
    ap.add_argument("--shuffle", type=int, default=0, metavar="R")
    ap.add_argument("--shuffle-kind", default="time_bin", choices=("time_bin", "column_cycle", "both", "neuron_circular"))
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--loop-shuffles", type=int, default=50)
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    T = bench.CONFIGS["c3"][1]
    y, B, W0, _ = bench.synth(N, T, L)
    tun = np.logaddexp(B.astype(np.float64) @ W0.astype(np.float64), 0.0)
    if args.exact and args.crossover:
        rec = run_exact_crossover(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_exact_crossover_c3.json")
    elif args.exact:
        rec = run_exact(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_exact_bench_c3.json")
    elif args.crossover:
        rec = run_crossover(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_crossover_c3.json")
    elif args.shuffle and args.shuffle_kind == "neuron_circular":
        rec = run_neuron_shuffle(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_shuffle_bench_c3_neuron_circular.json")
    elif args.shuffle:
        rec = run_shuffle(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_shuffle_bench_c3.json")
    elif args.sample:
        rec = run_sample(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_sample_bench_c3.json")
    elif args.viterbi:
        rec = run_viterbi(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_viterbi_bench_c3.json")
    else:
        rec = run_events(args, y, tun)
        path = args.json or os.path.join(ROOT, "profiles", "segments_bench_c3.json")
    print(json.dumps(rec), flush=True)
    save(path, rec)


if __name__ == "__main__":
    main()
