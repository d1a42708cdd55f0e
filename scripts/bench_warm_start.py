"""Warm-start microbenchmark: the HIP forward splat (csrc/forward_splat.hip) against the scipy
``forward_interpolate`` it replaces on the GPU, and what warm start costs a video stream.

* the op at the low-resolution grids of Sintel (55 x 128), 1080p (135 x 240) and 4K (270 x 480),
  for a smooth random flow (sigma = 4 px) and for a flow with under 1 % valid points (every
  target pixel searches far), beside scipy on the same input (host time, copies included);
* ``FlowInference`` pairs/s at 440 x 1024, 20 iterations, fp32, HIP graph: cold, warm through
  the device op, warm through the scipy path.

Event timing after warm-up.  The log goes to ``--out`` (default profiles/warm_start_bench.log).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raft_ros_amd.ros.node as node_mod  # noqa: E402
from raft_ros_amd.data.synthetic import demo_sequence  # noqa: E402
from raft_ros_amd.ops.warm_start import forward_splat_nearest  # noqa: E402
from raft_ros_amd.utils.utils import forward_interpolate  # noqa: E402

GRIDS = [(55, 128), (135, 240), (270, 480)]


def smooth_flow(H, W, sigma=4.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn(1, 2, -(-H // 8) + 1, -(-W // 8) + 1, generator=g)
    f = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    return (f * (sigma / f.std())).contiguous()


def sparse_flow(H, W, share=0.005, seed=0):
    g = torch.Generator().manual_seed(seed)
    f = torch.full((1, 2, H, W), 1000.0)
    keep = torch.rand(H, W, generator=g) < share
    f[0, :, keep] = torch.randn(2, int(keep.sum()), generator=g)
    return f


def valid_share(f):
    H, W = f.shape[-2:]
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    x1, y1 = xs + f[0, 0].double(), ys + f[0, 1].double()
    return ((x1 > 0) & (x1 < W) & (y1 > 0) & (y1 < H)).double().mean().item()


def time_gpu(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps  # ms


def time_host(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def scipy_splat(flow):
    """The hand-off without the device op: host round trip + two griddata calls per image."""
    return torch.stack([forward_interpolate(x) for x in flow]).to(flow.device)


def bench_op(say, reps, scipy_reps):
    say("forward splat: HIP op (event time) vs scipy forward_interpolate incl. copies (host time)")
    for H, W in GRIDS:
        for kind, f in (("smooth sigma=4", smooth_flow(H, W)), ("sparse", sparse_flow(H, W))):
            d = f.cuda()
            t_op = time_gpu(lambda: forward_splat_nearest(d), reps)
            t_sp = time_host(lambda: scipy_splat(d), scipy_reps)
            say(f"  {H:3d} x {W:3d}  {kind:14s} valid {100 * valid_share(f):5.1f} %   "
                f"HIP {1e3 * t_op:8.1f} us   scipy {t_sp:8.2f} ms   ({t_sp / t_op:7.0f}x)")


def bench_stream(say, pairs, scipy_pairs, iters=20, size=(440, 1024)):
    say(f"FlowInference, RAFT-base fp32, {size[0]} x {size[1]}, {iters} iterations, HIP graph")
    frames = [np.ascontiguousarray(f.permute(1, 2, 0).numpy()) for f in demo_sequence(4, *size)]
    rates = {}
    device_splat = node_mod.forward_splat_nearest
    for name, warm, splat, n in (("cold", False, device_splat, pairs), ("warm, device op", True, device_splat, pairs),
                                 ("warm, scipy path", True, scipy_splat, scipy_pairs)):
        torch.manual_seed(0)
        inf = node_mod.FlowInference(None, small=False, device="cuda", iters=iters, warm_start=warm)
        node_mod.forward_splat_nearest = splat
        state = {"k": 0}

        def step():
            k = state["k"]
            state["k"] += 1
            # consecutive stamps: every pair after the first is continuous
            inf.flow(frames[k % 3], frames[k % 3 + 1], prev_stamp=float(k), curr_stamp=float(k + 1))

        try:
            ms = time_gpu(step, n, warmup=6)
        finally:
            node_mod.forward_splat_nearest = device_splat
        rates[name] = 1e3 / ms
        say(f"  {name:17s} {ms:8.3f} ms/pair   {1e3 / ms:7.1f} pairs/s   (graphs: {inf.runner.num_graphs})")
    c, w = 1e3 / rates["cold"], 1e3 / rates["warm, device op"]
    say(f"  warm (device op) - cold = {1e3 * (w - c):.0f} us per pair")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "warm_start_bench.log"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--scipy_reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--scipy_pairs", type=int, default=20)
    ap.add_argument("--skip_stream", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_warm_start.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        bench_op(say, args.reps, args.scipy_reps)
        if not args.skip_stream:
            bench_stream(say, args.pairs, args.scipy_pairs)


if __name__ == "__main__":
    main()
