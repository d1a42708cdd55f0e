"""Point-track microbenchmark: the HIP op (csrc/track_points.hip) against the torch reference on
the same device and against the host path it replaces, and what tracking costs ``FlowInference``.

* one step at 440 x 1024 with ``S = 32`` (N = 448) and ``S = 8`` (N = 7040), the state a few steps
  into a sequence: the op (event time), ``track_points_ref`` on the GPU (event time; the same
  arithmetic as ~100 torch ops) and the host path (host clock: both full-resolution flows copied to
  the host, then ``track_points_ref`` on the CPU).  The three alternate in rounds in one process;
  the median round of each;
* ``FlowInference`` pairs/s at 440 x 1024, 20 iterations, fp32, HIP graph, ``device_io`` on:
  ``visualize`` (track off) against ``visualize_tracks`` (the same run plus the tracker step and
  the five arrays read back under the one synchronisation), alternating rounds, host clock around
  calls that end in a device synchronise; the median round of each and their ratio.

The log goes to ``--out`` (default profiles/track_points_bench.log).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raft_ros_amd.data.synthetic import demo_sequence  # noqa: E402
from raft_ros_amd.ops.track import seed_points, track_points, track_points_ref  # noqa: E402
from raft_ros_amd.ros.node import FlowInference  # noqa: E402
from scripts.bench_warm_start import time_gpu  # noqa: E402

SHAPE = (440, 1024)


def smooth_flows(H, W, seed):
    """A smooth forward flow of a few pixels and bw = -fw plus noise (most points consistent)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(1, 2, H // 40 + 2, W // 40 + 2, generator=g) * 6
    fw = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=True)
    bw = -fw + torch.randn(1, 2, H, W, generator=g) * 0.3
    return fw.contiguous(), bw.contiguous()


def same(a, b):
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def bench_op(say, S, rounds, reps, ref_reps, host_reps):
    dev = torch.device("cuda", 0)
    H, W = SHAPE
    roi = (0, 0, W, H)
    flows = [tuple(t.to(dev) for t in smooth_flows(H, W, s)) for s in range(4)]
    state = [t.to(dev) for t in seed_points(1, roi, S, None)]
    for fw, bw in flows[:3]:  # a few steps in: ages differ, some slots re-seeded
        out = track_points(*state, fw, bw, roi, S)
        state = [out[0], out[2], out[3], out[4]]
    fw, bw = flows[3]
    got, want = track_points(*state, fw, bw, roi, S), track_points_ref(*state, fw, bw, roi, S)
    h_state = [t.cpu() for t in state]
    host = track_points_ref(*h_state, fw.cpu(), bw.cpu(), roi, S)
    equal = all(same(g, w) for g, w in zip(got, want)) and all(same(g.cpu(), w) for g, w in zip(got, host))

    def host_path():  # what a consumer does today: the flows to the host, the book-keeping there
        track_points_ref(*h_state, fw.cpu(), bw.cpu(), roi, S)

    ms = {"op": [], "ref": [], "host": []}
    for _ in range(rounds):
        ms["op"].append(time_gpu(lambda: track_points(*state, fw, bw, roi, S), reps))
        ms["ref"].append(time_gpu(lambda: track_points_ref(*state, fw, bw, roi, S), ref_reps, warmup=2))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(host_reps):
            host_path()
        ms["host"].append((time.perf_counter() - t0) * 1e3 / host_reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    N = state[1].shape[1]
    say(f"  S = {S:2d} (N = {N:4d})  track_points {1e3 * med['op']:8.1f} us   torch reference on the GPU "
        f"{1e3 * med['ref']:8.1f} us ({med['ref'] / med['op']:5.1f}x)   host path {1e3 * med['host']:8.1f} us "
        f"({med['host'] / med['op']:5.1f}x)   results bitwise equal: {equal}")
    say(f"      rounds (us): op {' '.join(f'{1e3 * x:.1f}' for x in ms['op'])} | ref "
        f"{' '.join(f'{1e3 * x:.0f}' for x in ms['ref'])} | host {' '.join(f'{1e3 * x:.0f}' for x in ms['host'])}")
    say(f"      slots per status (tracked, inconsistent, left, crowded out): {got[7][0].tolist()}")


def bench_inference(say, rounds, pairs, cell, iters=20):
    H, W = SHAPE
    say(f"FlowInference, RAFT-base fp32, {H} x {W}, {iters} iterations, HIP graph, device_io on, track_cell {cell}; "
        f"{rounds} alternating rounds of {pairs} pairs, host clock, median round")
    frames = [np.ascontiguousarray(f.permute(1, 2, 0).numpy()) for f in demo_sequence(4, H, W)]
    torch.manual_seed(0)
    inf = FlowInference(None, small=False, device="cuda", iters=iters, device_io=True, track=True, track_cell=cell)
    state = {"k": 0}

    def step(on):
        k = state["k"]
        state["k"] += 1
        (inf.visualize_tracks if on else inf.visualize)(frames[k % 3], frames[k % 3 + 1], float(k), float(k + 1))

    ms = {False: [], True: []}
    for on in (False, True):  # warm-up of both paths: graph capture, pinned buffers, code objects
        for _ in range(6):
            step(on)
    for _ in range(rounds):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(pairs):
                step(on)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) * 1e3 / pairs)
    med = {on: statistics.median(v) for on, v in ms.items()}
    for on in (False, True):
        say(f"  track {'on ' if on else 'off'} {med[on]:8.3f} ms/pair   {1e3 / med[on]:7.1f} pairs/s   "
            f"(rounds: {' '.join(f'{x:.2f}' for x in ms[on])})")
    say(f"  track on / off = {med[True] / med[False]:.3f}x the time per pair")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "track_points_bench.log"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ref_reps", type=int, default=10)
    ap.add_argument("--host_reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--skip_inference", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_points.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        H, W = SHAPE
        say(f"one step at {H} x {W}, B = 1, with flow_bw; {args.rounds} alternating rounds, median round "
            "(op and GPU reference: event time; host path: host clock, both flows copied to the host)")
        for S in (32, 8):
            bench_op(say, S, args.rounds, args.reps, args.ref_reps, args.host_reps)
        if not args.skip_inference:
            bench_inference(say, args.rounds, args.pairs, 32)


if __name__ == "__main__":
    main()
