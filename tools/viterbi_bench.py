"""Per-call time of the MAP (Viterbi) decode, pmg_viterbi_decode through DeviceEM.viterbi:
seeded synthetic spikes (bench.synth), the emission computed once, then HIP events around
`--calls` decodes after `--warmup` of them.  --batch R stacks R equal-length sequences (the
first is bench.synth's; sequence r is the same recording rolled by 997 r time bins) and
decodes them in one launch.  Prints one JSON line; --json PATH also stores it there under
the key "<config>_R<batch>".  For the split between the forward scan and the back-trace
run it once under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from poor_man_gplvm_amd import banded_transition  # noqa: E402
from poor_man_gplvm_amd.engine import DeviceEM, SpikeData  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=("c2", "c3", "c5"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    N, T, L = bench.CONFIGS[args.config]
    R = max(1, args.batch)
    y, B, W0, _ = bench.synth(N, T, L)
    tun = np.logaddexp(B.astype(np.float64) @ W0.astype(np.float64), 0.0)
    if R > 1:
        y = np.concatenate([np.roll(y, 997 * r, axis=0) for r in range(R)])
    eng = DeviceEM(SpikeData(y), L)
    eng.set_transition(banded_transition(L, 1.0, 0.01, 0.01))
    eng.set_tuning(tun)
    eng.emission(1.0)
    for _ in range(args.warmup):
        out = eng.viterbi(1.0, R)
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(args.calls):
        out = eng.viterbi(1.0, R)
    b.record(st)
    b.synchronize()
    ms = a.elapsed_time(b) / args.calls
    pd, pl, lj = (t.cpu().numpy() for t in out)
    rec = {"config": args.config, "N": N, "T": T, "L": L, "batch": R, "calls": args.calls,
           "ms_per_call": round(ms, 4), "ns_per_step": round(1e6 * ms / T, 2),
           "ns_per_step_per_sequence": round(1e6 * ms / (T * R), 2),
           "log_joint_map_0": float(lj[0]), "jump_fraction_0": float(pd[0].mean()),
           "path_checksum": int(pl.astype(np.int64).sum() + pd.astype(np.int64).sum())}
    print(json.dumps(rec), flush=True)
    if args.json:
        allrec = {}
        if os.path.exists(args.json):
            with open(args.json) as f:
                allrec = json.load(f)
        allrec[f"{args.config}_R{R}"] = rec
        with open(args.json, "w") as f:
            json.dump(allrec, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
