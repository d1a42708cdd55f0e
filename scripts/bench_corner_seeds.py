"""Corner-seed microbenchmark: the HIP op (csrc/corner_seeds.hip) against the torch reference on the
same device, and what corner seeds cost ``FlowInference``.

* the op alone at 440 x 1024 and 1080 x 1920, ``B = 2`` (the pair ``FlowInference`` hands it), for
  ``S`` = 8 and 32, on a frame of ``demo_sequence``: the op (event time) against
  ``corner_seeds_ref`` on the GPU (event time; the same arithmetic as ~150 torch ops).  The two
  alternate in rounds in one process; the median round of each;
* ``FlowInference.visualize_tracks`` pairs/s at 440 x 1024, 20 iterations, fp32, HIP graph,
  ``device_io`` on, ``track_seeds`` ``grid`` against ``corners`` (one more op on the uint8 pair that is
  already on the device, seeds into the tracker, a sixth array read back), two instances in
  alternating rounds of one process, host clock around calls that end in a device synchronise;
  the median round of each and their ratio.  The yardstick is the ``grid`` rate of the same process.

The log goes to ``--out`` (default profiles/corner_seeds_bench.log).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raft_ros_amd.data.synthetic import demo_sequence  # noqa: E402
from raft_ros_amd.ops.corners import corner_seeds, corner_seeds_ref  # noqa: E402
from raft_ros_amd.ros.node import FlowInference  # noqa: E402
from scripts.bench_warm_start import time_gpu  # noqa: E402


def bench_op(say, H, W, S, rounds, reps, ref_reps):
    dev = torch.device("cuda", 0)
    frames = torch.stack([f.permute(1, 2, 0) for f in demo_sequence(2, H, W)]).contiguous().to(dev)
    got, want = corner_seeds(frames, S), corner_seeds_ref(frames, S)
    host = corner_seeds_ref(frames.cpu(), S)
    equal = all(torch.equal(g, w) for g, w in zip(got, want)) and all(torch.equal(g.cpu(), w) for g, w in zip(got, host))
    ms = {"op": [], "ref": []}
    for _ in range(rounds):
        ms["op"].append(time_gpu(lambda: corner_seeds(frames, S), reps))
        ms["ref"].append(time_gpu(lambda: corner_seeds_ref(frames, S), ref_reps, warmup=2))
    med = {k: statistics.median(v) for k, v in ms.items()}
    N = got[1].shape[1]
    fallback = int((got[1] <= 0).sum())
    say(f"  {H:4d} x {W:4d}  S = {S:2d} (N = {N:5d})  corner_seeds {1e3 * med['op']:8.1f} us   torch reference on the "
        f"GPU {1e3 * med['ref']:9.1f} us ({med['ref'] / med['op']:6.1f}x)   results bitwise equal: {equal}   "
        f"cells at their centre: {fallback} of {2 * N}")
    say(f"      rounds (us): op {' '.join(f'{1e3 * x:.1f}' for x in ms['op'])} | ref "
        f"{' '.join(f'{1e3 * x:.0f}' for x in ms['ref'])}")


def bench_inference(say, rounds, pairs, cell, iters=20):
    H, W = 440, 1024
    say(f"FlowInference.visualize_tracks, RAFT-base fp32, {H} x {W}, {iters} iterations, HIP graph, device_io on, "
        f"track_cell {cell}; {rounds} alternating rounds of {pairs} pairs, host clock, median round")
    frames = [np.ascontiguousarray(f.permute(1, 2, 0).numpy()) for f in demo_sequence(4, H, W)]
    infs = {}
    for mode in ("grid", "corners"):
        torch.manual_seed(0)
        infs[mode] = FlowInference(None, small=False, device="cuda", iters=iters, device_io=True, track=True,
                                   track_cell=cell, track_seeds=mode)
    state = {"grid": 0, "corners": 0}

    def step(mode):
        k = state[mode]
        state[mode] += 1
        infs[mode].visualize_tracks(frames[k % 3], frames[k % 3 + 1], float(k), float(k + 1))

    ms = {"grid": [], "corners": []}
    for mode in ms:  # warm-up of both: graph capture, pinned buffers, code objects
        for _ in range(6):
            step(mode)
    for _ in range(rounds):
        for mode in ms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(pairs):
                step(mode)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) * 1e3 / pairs)
    med = {mode: statistics.median(v) for mode, v in ms.items()}
    for mode in ms:
        say(f"  track_seeds {mode:7s} {med[mode]:8.3f} ms/pair   {1e3 / med[mode]:7.1f} pairs/s   "
            f"(rounds: {' '.join(f'{x:.2f}' for x in ms[mode])})")
    say(f"  corners / grid = {med['corners'] / med['grid']:.3f}x the time per pair")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "corner_seeds_bench.log"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ref_reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--skip_inference", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_corner_seeds.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        say(f"corner_seeds, B = 2, default margin, min_score 0; {args.rounds} alternating rounds, median round, "
            "event time")
        for H, W in ((440, 1024), (1080, 1920)):
            for S in (8, 32):
                bench_op(say, H, W, S, args.rounds, args.reps, args.ref_reps)
        if not args.skip_inference:
            bench_inference(say, args.rounds, args.pairs, 32)


if __name__ == "__main__":
    main()
