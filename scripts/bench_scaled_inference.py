"""Working-resolution inference benchmark: the two HIP ops (csrc/frame_scale.hip) against their
torch sequences on the same device, and what a working resolution buys ``FlowInference``.

* (a) ``ingest_frames_scaled`` and ``upscale_flow`` at 1080 x 1920 with D = 2, 3, 4 and at
  440 x 1024 with D = 2: us per call (event time) and the achieved GB/s over the bytes each has to
  move, beside ``ingest_frames_scaled_ref`` / ``upscale_flow_ref`` -- the same arithmetic as torch
  ops -- on the same GPU; op and sequence alternate in rounds in the same process, the median
  round of each is reported;
* (b) ``FlowInference.visualize`` pairs/s at 1080 x 1920, RAFT-base fp32, 20 iterations, random
  weights, HIP graph, ``device_io`` on, with ``scale`` 1, 2, 3, 4: the four alternate in rounds in
  the same process, host clock around calls that end in a device synchronise; the median round of
  each and its ratio to ``scale = 1``.

Random weights: the speed does not depend on them, the accuracy at a reduced resolution does and is
not measured here.  The log goes to ``--out`` (default profiles/scaled_inference_bench.log).
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
from raft_ros_amd.ops.frame_scale import (ingest_frames_scaled, ingest_frames_scaled_ref, scaled_shape,  # noqa: E402
                                          upscale_flow, upscale_flow_ref)
from raft_ros_amd.ros.node import FlowInference  # noqa: E402
from scripts.bench_warm_start import time_gpu  # noqa: E402

OP_CASES = (((1080, 1920), 2), ((1080, 1920), 3), ((1080, 1920), 4), ((440, 1024), 2))
FRAME = (1080, 1920)
SCALES = (1, 2, 3, 4)


def same(got, want):
    nan = want.isnan()
    return bool(torch.equal(got.isnan(), nan) and torch.equal(got[~nan], want[~nan]))


def alternate(fns, rounds, reps):
    """Median over alternating rounds of the event time per call (ms) of each function."""
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, (fn, n) in enumerate(zip(fns, reps)):
            ms[k].append(time_gpu(fn, n, warmup=3))
    return [statistics.median(v) for v in ms]


def bench_ops(say, rounds, reps, ref_reps):
    dev = torch.device("cuda", 0)
    say(f"(a) ops alone: HIP op vs its torch sequence on the same GPU (event time, median of {rounds} alternating "
        f"rounds of {reps} / {ref_reps} calls; back-to-back calls on the same buffers, which can stay in the 256 MiB "
        "Infinity Cache)")
    g = torch.Generator().manual_seed(0)
    for (H, W), D in OP_CASES:
        frames = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
        images, padder = ingest_frames_scaled(frames, D)
        pads = padder._pad
        want = ingest_frames_scaled_ref(frames, D, pads)
        equal = torch.equal(images, want)
        t_op, t_ref = alternate([lambda: ingest_frames_scaled(frames, D),
                                 lambda: ingest_frames_scaled_ref(frames, D, pads)], rounds, (reps, ref_reps))
        moved = frames.numel() + images.numel() * 4  # every byte read once, the padded fp32 pair written
        say(f"  {H:4d} x {W:4d} D={D}  ingest_frames_scaled (2 frames -> {tuple(images.shape[-2:])}) {1e3 * t_op:8.1f} us  "
            f"{moved / t_op / 1e6:7.1f} GB/s   torch sequence {1e3 * t_ref:8.1f} us  ({t_ref / t_op:5.1f}x)   "
            f"bitwise equal: {equal}")
        h, w = scaled_shape(H, W, D)
        l, r, t, b = pads
        flow = (torch.randn(1, 2, h + t + b, w + l + r, generator=g) * 8).to(dev)
        up = upscale_flow(flow, padder, D, (H, W))
        equal = same(up, upscale_flow_ref(flow, D, l, t, w, h, H, W))
        t_op, t_ref = alternate([lambda: upscale_flow(flow, padder, D, (H, W)),
                                 lambda: upscale_flow_ref(flow, D, l, t, w, h, H, W)], rounds, (reps, ref_reps))
        moved = (2 * h * w + up.numel()) * 4  # the unpadded low-resolution flow read once, the result written
        say(f"  {H:4d} x {W:4d} D={D}  upscale_flow ({tuple(flow.shape[-2:])} -> {H} x {W})          {1e3 * t_op:8.1f} us  "
            f"{moved / t_op / 1e6:7.1f} GB/s   torch sequence {1e3 * t_ref:8.1f} us  ({t_ref / t_op:5.1f}x)   "
            f"bitwise equal: {equal}")


def bench_inference(say, rounds, pairs, iters=20):
    H, W = FRAME
    say(f"(b) FlowInference.visualize, RAFT-base fp32, random weights, {H} x {W}, {iters} iterations, HIP graph, "
        f"device_io on; {rounds} alternating rounds of {pairs} pairs, host clock, median round")
    frames = [np.ascontiguousarray(f.permute(1, 2, 0).numpy()) for f in demo_sequence(4, H, W)]
    infs = {}
    for D in SCALES:
        torch.manual_seed(0)
        infs[D] = FlowInference(None, small=False, device="cuda", iters=iters, device_io=True, scale=D)
    state = {"k": 0}

    def step(D):
        k = state["k"]
        state["k"] += 1
        return infs[D].visualize(frames[k % 3], frames[k % 3 + 1])

    ms = {D: [] for D in SCALES}
    for D in SCALES:  # warm-up of every path: graph capture, pinned buffers, code objects
        for _ in range(4):
            img = step(D)
        assert img.shape == (H, W, 3), img.shape
    for _ in range(rounds):
        for D in SCALES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(pairs):
                step(D)
            torch.cuda.synchronize()
            ms[D].append((time.perf_counter() - t0) * 1e3 / pairs)
    med = {D: statistics.median(v) for D, v in ms.items()}
    for D in SCALES:
        h, w = scaled_shape(H, W, D)
        say(f"  scale {D} (model at {h:4d} x {w:4d}) {med[D]:8.3f} ms/pair   {1e3 / med[D]:7.1f} pairs/s   "
            f"{med[1] / med[D]:5.2f}x scale 1   (rounds: {' '.join(f'{x:.2f}' for x in ms[D])})")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "scaled_inference_bench.log"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--ref_reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--skip_inference", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scaled_inference.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        bench_ops(say, args.rounds, args.reps, args.ref_reps)
        if not args.skip_inference:
            bench_inference(say, args.rounds, args.pairs)


if __name__ == "__main__":
    main()
