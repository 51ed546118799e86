"""Summarise tools/gpu_bench_ab.sh outputs (bench.py --full lines): value and per-section
kernel ms per run.  usage: python tools/ab_summary.py TAG [OUTDIR]"""
import glob
import json
import sys

tag = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else "bench_out"
for f in sorted(glob.glob(f"{out}/{tag}_*.json")):
    try:
        d = json.loads(open(f).read().strip().splitlines()[-1])
    except Exception as e:  # noqa: BLE001
        print(f, "unreadable", e)
        continue
    k = d.get("kernels_ms", {})
    ks = " ".join(f"{n}={v:.4f}" for n, v in sorted(k.items()) if isinstance(v, (int, float)))
    print(f"{f.split('/')[-1]:28s} {d['value']:8.1f} frac={d['roofline']['frac']:.3f}  {ks}")
