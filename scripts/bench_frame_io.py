"""Frame-path microbenchmark: the HIP colour coding and frame ingest (csrc/flow_color.hip) against
the host code they replace, and what ``device_io`` does to the published image rate.

* the two ops alone at 440 x 1024, 1080 x 1920 and 135 x 240: us per call (event time) and the
  achieved GB/s over the bytes the op has to move (colour: the flow read by both passes + the
  image written; ingest: two uint8 frames read + their padded fp32 planes written), beside the
  host code on the same box (numpy ``flow_to_image`` incl. the copy of the flow to the host; the
  CPU ``permute().float()``, upload and replicate padding of two frames);
* ``FlowInference.visualize`` pairs/s at 440 x 1024, 20 iterations, fp32, HIP graph, with
  ``device_io`` off and on: the two alternate in rounds in the same process, host clock around
  calls that end in a device synchronise; the median round of each and their ratio.

The log goes to ``--out`` (default profiles/frame_io_bench.log).
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
from raft_ros_amd.ops.frame_io import flow_to_image, ingest_frames  # noqa: E402
from raft_ros_amd.ros.node import FlowInference  # noqa: E402
from raft_ros_amd.utils import flow_viz  # noqa: E402
from raft_ros_amd.utils.utils import InputPadder  # noqa: E402
from scripts.bench_warm_start import time_gpu, time_host  # noqa: E402

SHAPES = [(440, 1024), (1080, 1920), (135, 240)]


def color_bytes(H, W):
    return H * W * (2 * 8 + 3)  # u, v read by the maximum pass and again by the colour pass; 3 bytes written


def ingest_bytes(n, H, W, padder):
    l, r, t, b = padder._pad
    return n * (H * W * 3 + 3 * (H + t + b) * (W + l + r) * 4)


def host_color(flow):
    """What visualize does without the op: flow to the host, numpy colour coding, channel swap."""
    flo = flow[0].permute(1, 2, 0).float().cpu().numpy()
    return np.ascontiguousarray(flow_viz.flow_to_image(flo)[:, :, [2, 1, 0]]).astype(np.uint8)


def host_ingest(frames, device):
    """What flow() does without the op: CPU uint8 -> fp32 CHW, fp32 upload, replicate padding."""
    imgs = [torch.from_numpy(f).permute(2, 0, 1).float()[None].to(device) for f in frames]
    return InputPadder(imgs[0].shape).pad(*imgs)


def bench_ops(say, reps, host_reps):
    dev = torch.device("cuda", 0)
    say("ops alone: HIP op (event time, achieved GB/s) vs the host code it replaces (host time, copies included)")
    say("  (back-to-back calls on the same buffers: they can stay in the 256 MiB Infinity Cache, and the small "
        "shapes are launch-bound)")
    for H, W in SHAPES:
        g = torch.Generator().manual_seed(0)
        flow = (torch.randn(1, 2, H, W, generator=g) * 8).to(dev)
        frames = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=g)
        d_frames = frames.to(dev)
        padder = ingest_frames(d_frames)[1]
        t_col = time_gpu(lambda: flow_to_image(flow, convert_to_bgr=True), reps)
        t_ing = time_gpu(lambda: ingest_frames(d_frames), reps)
        h_col = time_host(lambda: host_color(flow), host_reps)
        np_frames = [f.numpy() for f in frames]
        h_ing = time_host(lambda: host_ingest(np_frames, dev), host_reps)
        say(f"  {H:4d} x {W:4d}  flow_to_image {1e3 * t_col:8.1f} us  {color_bytes(H, W) / t_col / 1e6:7.1f} GB/s"
            f"   numpy path {h_col:8.2f} ms  ({h_col / t_col:6.0f}x)")
        say(f"  {H:4d} x {W:4d}  ingest_frames {1e3 * t_ing:8.1f} us  "
            f"{ingest_bytes(2, H, W, padder) / t_ing / 1e6:7.1f} GB/s   torch path {h_ing:8.2f} ms  "
            f"({h_ing / t_ing:6.0f}x)")


def bench_visualize(say, rounds, pairs, iters=20, size=(440, 1024)):
    say(f"FlowInference.visualize, RAFT-base fp32, {size[0]} x {size[1]}, {iters} iterations, HIP graph; "
        f"{rounds} alternating rounds of {pairs} pairs, host clock, median round")
    frames = [np.ascontiguousarray(f.permute(1, 2, 0).numpy()) for f in demo_sequence(4, *size)]
    torch.manual_seed(0)
    inf = FlowInference(None, small=False, device="cuda", iters=iters)
    state = {"k": 0}

    def step():
        k = state["k"]
        state["k"] += 1
        inf.visualize(frames[k % 3], frames[k % 3 + 1])

    ms = {False: [], True: []}
    for on in (False, True):  # warm-up of both paths: graph capture, pinned buffers, code objects
        inf.device_io = on
        for _ in range(6):
            step()
    for _ in range(rounds):
        for on in (False, True):
            inf.device_io = on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(pairs):
                step()
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) * 1e3 / pairs)
    med = {on: statistics.median(v) for on, v in ms.items()}
    for on in (False, True):
        say(f"  device_io {'on ' if on else 'off'} {med[on]:8.3f} ms/pair   {1e3 / med[on]:7.1f} pairs/s   "
            f"(rounds: {' '.join(f'{x:.2f}' for x in ms[on])})")
    ratio = med[False] / med[True]
    say(f"  device_io on / off = {ratio:.2f}x pairs/s" + ("" if ratio >= 1 else "   (SLOWER with device_io on)"))
    return ratio


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "frame_io_bench.log"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host_reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--skip_visualize", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_frame_io.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        bench_ops(say, args.reps, args.host_reps)
        if not args.skip_visualize:
            bench_visualize(say, args.rounds, args.pairs)


if __name__ == "__main__":
    main()
