"""Forward-backward consistency microbenchmark: the HIP op (csrc/fb_consistency.hip) against the
torch reference on the same device, and what the bidirectional mode costs ``FlowInference``.

* the op alone at 440 x 1024: us per call (event time) and the achieved GB/s over the bytes it has
  to move (fw and bw read once, the mask and the error written), beside ``fb_consistency_ref`` --
  the same arithmetic as ~60 torch ops -- on the same GPU;
* ``FlowInference`` pairs/s at 440 x 1024, 20 iterations, fp32, HIP graph, ``device_io`` on:
  ``visualize`` (one direction) against ``visualize_checked`` (the batch of two directions, the
  check, the mask read-back); the two alternate in rounds in the same process, host clock around
  calls that end in a device synchronise; the median round of each and their ratio.

The log goes to ``--out`` (default profiles/fb_consistency_bench.log).
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
from raft_ros_amd.ops.consistency import fb_consistency, fb_consistency_ref  # noqa: E402
from raft_ros_amd.ros.node import FlowInference  # noqa: E402
from scripts.bench_warm_start import time_gpu  # noqa: E402

SHAPE = (440, 1024)


def op_bytes(H, W):
    return H * W * (2 * 8 + 1 + 4)  # u, v of both flows read; one mask byte and one fp32 error written


def bench_op(say, reps, ref_reps):
    dev = torch.device("cuda", 0)
    H, W = SHAPE
    g = torch.Generator().manual_seed(0)
    fw = (torch.randn(1, 2, H, W, generator=g) * 4).to(dev)
    bw = (-fw.cpu() + torch.randn(1, 2, H, W, generator=g)).to(dev)
    got, want = fb_consistency(fw, bw), fb_consistency_ref(fw, bw)
    nan = want[1].isnan()
    equal = (torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[1].isnan(), nan)
             and torch.equal(got[1][~nan], want[1][~nan]))
    t_op = time_gpu(lambda: fb_consistency(fw, bw), reps)
    t_ref = time_gpu(lambda: fb_consistency_ref(fw, bw), ref_reps)
    say("op alone: HIP op vs the torch reference on the same GPU (event time; back-to-back calls on the same "
        "buffers, which can stay in the 256 MiB Infinity Cache)")
    say(f"  {H:4d} x {W:4d}  fb_consistency {1e3 * t_op:8.1f} us  {op_bytes(H, W) / t_op / 1e6:7.1f} GB/s   "
        f"torch reference {1e3 * t_ref:8.1f} us  ({t_ref / t_op:5.1f}x)   results bitwise equal: {equal}")
    say(f"  counts (class 1, class 2): {got[2][0].tolist()} of {H * W} pixels")


def bench_inference(say, rounds, pairs, iters=20):
    H, W = SHAPE
    say(f"FlowInference, RAFT-base fp32, {H} x {W}, {iters} iterations, HIP graph, device_io on; "
        f"{rounds} alternating rounds of {pairs} pairs, host clock, median round")
    frames = [np.ascontiguousarray(f.permute(1, 2, 0).numpy()) for f in demo_sequence(4, H, W)]
    torch.manual_seed(0)
    inf = FlowInference(None, small=False, device="cuda", iters=iters, device_io=True, consistency=True)
    state = {"k": 0}

    def step(checked):
        k = state["k"]
        state["k"] += 1
        (inf.visualize_checked if checked else inf.visualize)(frames[k % 3], frames[k % 3 + 1])

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
        say(f"  consistency {'on ' if on else 'off'} {med[on]:8.3f} ms/pair   {1e3 / med[on]:7.1f} pairs/s   "
            f"(rounds: {' '.join(f'{x:.2f}' for x in ms[on])})")
    say(f"  consistency on / off = {med[True] / med[False]:.2f}x the time per pair (two directions in one batch)")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "fb_consistency_bench.log"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ref_reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--skip_inference", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_fb_consistency.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        bench_op(say, args.reps, args.ref_reps)
        if not args.skip_inference:
            bench_inference(say, args.rounds, args.pairs)


if __name__ == "__main__":
    main()
