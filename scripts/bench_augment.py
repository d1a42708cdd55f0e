"""Training augmentation microbenchmark: ``BatchAugmentor`` through its torch ops against the HIP
ops raft_amd::augment_batch / augment_batch_sparse (csrc/augment.hip) on the same GPU.

Synthetic decoded batches (uint8 noise images, random flow) already on the device, at the shapes
of the training stages:

* chairs: 8 x 384 x 512 -> 368 x 496;
* things: 6 x 540 x 960 -> 400 x 720;
* a mixed Sintel-stage batch -> 368 x 768: 2 x 436 x 1024 (Sintel, dense), 3 x 375 x 1242 (KITTI,
  sparse) and one 1080 x 2560 (HD1K, sparse), which pads every sample of the batch to that size;
* kitti: 6 x 375 x 1242 -> 288 x 960, every sample sparse.

Three paths: ``torch`` (``native=False``), ``native`` (``native=True``: sparse samples' flow and
valid are scattered inside the op) and ``dense+torch``, composed here: the dense op
raft_amd::augment_batch and, where the mixture has sparse samples, ``_sparse_flow`` in torch ops
over the padded batch with its three boolean-mask indexings, which is what ``native=True`` did
before the op took sparse samples.  Without sparse samples that row is the native row's own code.

The paths alternate in rounds in one process with the same seed, so they draw the same
parameters; a round is a host clock around calls that end in a device synchronise; the median
round of each is reported beside the 16.6 ms training step of config #2
(profiles/r5p_launch_probe.log).  Measured are the whole call (``draw``, which both paths share
and which is torch ops on per-sample tensors, then ``apply``) and ``apply`` alone on one fixed
draw.  Device operations per batch (kernels, memsets and copies) are counted with torch.profiler
on one call of each.

The log goes to ``--out`` (default profiles/augment_bench.log).  The committed log closes with an
A/B of where the scatter runs (inside jitter pass 2 or as a launch of its own), measured once
with a build that had both; only the kept form exists, so this script does not regenerate it.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raft_ros_amd.data.augment import AugSpec, BatchAugmentor, collate_padded  # noqa: E402

STEP_MS = 16.6  # the training step at config #2, profiles/r5p_launch_probe.log

# name, crop, [(count, h, w, sparse)]
SHAPES = [
    ("chairs", (368, 496), [(8, 384, 512, False)]),
    ("things", (400, 720), [(6, 540, 960, False)]),
    ("sintel-mix", (368, 768), [(2, 436, 1024, False), (3, 375, 1242, True), (1, 1080, 2560, True)]),
    ("kitti", (288, 960), [(6, 375, 1242, True)]),
]
PATHS = ("torch", "dense+torch", "native")


def dense_op_and_sparse_torch(aug, batch, params):
    """``apply`` as ``native=True`` was before the op took sparse samples: every sample through the
    dense op, then the sparse ones' flow and valid from ``_sparse_flow``."""
    from raft_ros_amd.ops.augment import augment_batch

    flow = batch["flow"].float()
    o1, o2, of, dvalid = augment_batch(batch["img1"], batch["img2"], flow, batch["size"], params, aug.crop)
    if any(s.sparse for s in aug.specs):
        q = params
        B, Hm, Wm = batch["img1"].shape[:3]
        sf, sv = aug._sparse_flow(flow.permute(0, 3, 1, 2), batch["valid"].float(), q["sx"], q["sy"], q["resize"],
                                  q["hflip"], q["x0"], q["y0"], q["rh"], q["rw"], Hm, Wm)
        of = torch.where(q["sparse"].view(B, 1, 1, 1), sf, of)
        dvalid = torch.where(q["sparse"].view(B, 1, 1), sv, dvalid)
    return o1, o2, of, dvalid


def make_batch(groups, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    samples = []
    for n, h, w, sparse in groups:
        for _ in range(n):
            samples.append({"img1": torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8),
                            "img2": torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8),
                            "flow": torch.randn(h, w, 2, generator=g) * 8,
                            "valid": (torch.rand(h, w, generator=g) > 0.5).float() if sparse else torch.ones(h, w),
                            "spec": int(sparse)})
    return {k: v.to(dev) for k, v in collate_padded(samples).items()}


def device_ops(fn):
    """Device operations (kernels, memsets, copies) of one call, or None when the profiler fails."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # pragma: no cover - depends on the profiler of the host
        print(f"torch.profiler failed: {exc}", flush=True)
        return None


def bench_shape(say, name, crop, groups, rounds, calls):
    dev = torch.device("cuda", 0)
    batch = make_batch(groups, dev)
    B, Hm, Wm = batch["img1"].shape[:3]
    specs = [AugSpec(crop, -0.2, 0.6, True, False)]
    if any(g[3] for g in groups):
        specs.append(AugSpec(crop, -0.2, 0.4, False, True))
    augs = {path: BatchAugmentor(specs, seed=0, device=dev, native=path == "native") for path in PATHS}
    params = augs["torch"].draw(batch)  # the apply-only rows use one fixed draw
    augs["torch"].gen.manual_seed(0)

    def apply(path, p):
        if path == "dense+torch":
            return dense_op_and_sparse_torch(augs[path], batch, p)
        return augs[path].apply(batch, p)

    work = {"call": lambda path: apply(path, augs[path].draw(batch)), "apply": lambda path: apply(path, params)}
    ms = {(k, path): [] for k in work for path in PATHS}
    for k in work:  # warm-up: code objects, the allocator's pools
        for path in PATHS:
            for _ in range(3):
                work[k](path)
    for _ in range(rounds):
        for k in work:
            for path in PATHS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    work[k](path)
                torch.cuda.synchronize()
                ms[k, path].append((time.perf_counter() - t0) * 1e3 / calls)
    med = {key: statistics.median(v) for key, v in ms.items()}
    ops = {(k, path): device_ops(lambda: work[k](path)) for k in work for path in PATHS}
    cnt = lambda key: "not measured" if ops[key] is None else f"{ops[key]:5d}"  # noqa: E731
    say(f"{name}: {B} x {Hm} x {Wm} padded -> {crop[0]} x {crop[1]}, "
        f"{'with' if len(specs) > 1 else 'no'} sparse samples  ({rounds} alternating rounds of {calls} batches)")
    for k, what in (("call", "draw + apply"), ("apply", "apply alone ")):
        for path in PATHS:
            say(f"  {what}  {path:11s}  {med[k, path]:9.3f} ms/batch  {med[k, path] / STEP_MS:6.2f} x the "
                f"{STEP_MS} ms step   device operations per batch {cnt((k, path))}   "
                f"(rounds: {' '.join(f'{x:.2f}' for x in ms[k, path])})")
        say(f"  {what}  torch / native = {med[k, 'torch'] / med[k, 'native']:.1f}x   "
            f"dense+torch / native = {med[k, 'dense+torch'] / med[k, 'native']:.2f}x")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "augment_bench.log"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        say("BatchAugmentor on device-resident decoded batches (every path runs the same draw; torch and dense+torch run "
            "_sparse_flow in torch ops where the mixture has sparse samples, native scatters inside the op)")
        for name, crop, groups in SHAPES:
            bench_shape(say, name, crop, groups, args.rounds, args.calls)


if __name__ == "__main__":
    main()
