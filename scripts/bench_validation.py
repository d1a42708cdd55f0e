"""Validation-metrics benchmark: the HIP op (csrc/flow_metrics.hip) against what it replaces, and
the validators with the metrics on the host (``device_metrics`` off) and on the device (on).

At 436 x 1024 (Sintel: prediction padded to 440 x 1024, top = 2) and at 375 x 1242 with a sparse
``valid`` (KITTI: padded to 376 x 1248, left = 3):

* the op alone (event time) against the same torch ops on the GPU (``flow_metrics_ref`` on device
  tensors, event time) and against the host sequence of eval/validate.py (crop, ``.float().cpu()``,
  CPU torch ops, ``.item()``; host clock, it ends synchronised by nature);
* pairs/s of ``validate_synthetic`` at its defaults and of ``evaluate_samples`` over an in-memory
  list of samples of either size, RAFT-base fp32 with random weights, the switch off and on in
  alternating rounds of one process, host clock around calls that end in a read-back; the median
  round of each;
* device-to-host read-backs per sample (``Tensor.cpu`` / ``item`` / ``tolist`` counted) and device
  operations per sample of the metrics alone (kernels and copies seen by torch's profiler).

The log goes to ``--out`` (default profiles/validation_bench.log).
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raft_ros_amd.eval.validate as V  # noqa: E402
from raft_ros_amd.data.synthetic import synthetic_batch  # noqa: E402
from raft_ros_amd.models import RAFT  # noqa: E402
from raft_ros_amd.ops.metrics import flow_metrics, flow_metrics_ref  # noqa: E402
from raft_ros_amd.utils.utils import InputPadder  # noqa: E402
from scripts.bench_warm_start import time_gpu  # noqa: E402

CASES = {"sintel": (436, 1024), "kitti": (375, 1242)}


class Readbacks:
    """Counts ``Tensor.cpu`` / ``item`` / ``tolist`` of GPU tensors while active."""

    def __init__(self):
        self.count, self._saved = 0, {}

    def __enter__(self):
        for name in ("cpu", "item", "tolist"):
            orig = self._saved[name] = getattr(torch.Tensor, name)

            def wrapped(t, *a, _orig=orig, **k):
                self.count += int(t.is_cuda)
                return _orig(t, *a, **k)

            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self._saved.items():
            setattr(torch.Tensor, name, orig)


def host_metrics(kind, flow_pr, padder, flow_gt, valid_gt):
    """The per-sample host sequence of validate_sintel / validate_kitti."""
    flow = padder.unpad(flow_pr[0]).float().cpu()
    epe = torch.sum((flow - flow_gt) ** 2, dim=0).sqrt().view(-1)
    if kind == "sintel":
        return [epe.sum().item(), epe.numel(), (epe < 1).sum().item(), (epe < 3).sum().item(), (epe < 5).sum().item()]
    mag = torch.sum(flow_gt ** 2, dim=0).sqrt().view(-1)
    val = valid_gt.view(-1) >= 0.5
    out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()
    return [epe[val].mean().item(), 1, out[val].sum().item(), val.sum().item()]


def device_ops(fn):
    """Kernels and copies one call of ``fn`` puts on the device, as torch's profiler sees them."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def bench_op(say, kind, reps, rounds):
    dev = torch.device("cuda", 0)
    H, W = CASES[kind]
    g = torch.Generator().manual_seed(0)
    padder = InputPadder((1, 3, H, W), mode="kitti" if kind == "kitti" else "sintel")
    gt = torch.randn(2, H, W, generator=g) * 6
    pr = padder.pad((gt + torch.randn(2, H, W, generator=g) * 2)[None])[0].to(dev)
    valid = (torch.rand(H, W, generator=g) < 0.3).float() if kind == "kitti" else None
    d_gt, d_valid = gt.to(dev)[None], None if valid is None else valid.to(dev)[None]
    left, top = padder._pad[0], padder._pad[2]
    got, want = flow_metrics(pr, d_gt, d_valid, padder), flow_metrics_ref(pr.cpu(), gt[None], None if valid is None else valid[None], top, left)
    rel = ((got[0].cpu() - want[0]).abs() / want[0]).max().item()
    equal = torch.equal(got[1].cpu(), want[1])
    acc = V.MetricAccumulator(dev)
    t = {"op": [], "upd": [], "gpu": [], "host": []}
    for _ in range(rounds):
        t["op"].append(time_gpu(lambda: flow_metrics(pr, d_gt, d_valid, padder), reps))
        t["upd"].append(time_gpu(lambda: acc.update(pr, d_gt, d_valid, padder), reps))
        t["gpu"].append(time_gpu(lambda: flow_metrics_ref(pr, d_gt, d_valid, top, left), max(reps // 10, 5)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(max(reps // 10, 5)):
            host_metrics(kind, pr, padder, gt, valid)
        t["host"].append((time.perf_counter() - t0) * 1e3 / max(reps // 10, 5))
    med = {k: statistics.median(v) for k, v in t.items()}
    with Readbacks() as rb:
        host_metrics(kind, pr, padder, gt, valid)
    try:
        n_op = device_ops(lambda: flow_metrics(pr, d_gt, d_valid, padder))
        n_upd = device_ops(lambda: acc.update(pr, d_gt, d_valid, padder))
        n_host = device_ops(lambda: host_metrics(kind, pr, padder, gt, valid))
        ops_line = f"device operations per sample: op {n_op}, accumulator update {n_upd}, host sequence {n_host}"
    except Exception as exc:  # the count is a side note of the log, the timings above stand without it
        ops_line = f"device operations per sample: not counted ({type(exc).__name__}: {exc})"
    say(f"  {kind}: {H} x {W} in {pr.shape[-2]} x {pr.shape[-1]} at (top {top}, left {left}), valid {'yes' if valid is not None else 'no'}; "
        f"median of {rounds} rounds")
    say(f"    flow_metrics (HIP, event time)        {1e3 * med['op']:9.1f} us")
    say(f"    MetricAccumulator.update (op + adds)  {1e3 * med['upd']:9.1f} us")
    say(f"    same torch ops on the GPU (event)     {1e3 * med['gpu']:9.1f} us  ({med['gpu'] / med['op']:6.1f}x)")
    say(f"    host sequence: copy + CPU ops + item  {1e3 * med['host']:9.1f} us  ({med['host'] / med['op']:6.1f}x), "
        f"{rb.count} read-backs per sample (the op: 0)")
    say(f"    counts equal to the reference: {equal}; epe_sum rel err {rel:.2e}; {ops_line}")


def _timed_rounds(say, name, run, pairs, rounds):
    quiet = io.StringIO()
    res = {}
    with contextlib.redirect_stdout(quiet):
        for on in (False, True):  # warm-up of both paths
            res[on] = run(on)
    ms = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(quiet):
                run(on)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) * 1e3 / pairs)
    sync = {}
    for on in (False, True):
        with Readbacks() as rb, contextlib.redirect_stdout(quiet):
            run(on)
        sync[on] = rb.count
    med = {on: statistics.median(v) for on, v in ms.items()}
    say(f"  {name}: {pairs} pairs a round, {rounds} alternating rounds, host clock, median round")
    for on in (False, True):
        say(f"    device_metrics {'on ' if on else 'off'} {med[on]:8.3f} ms/pair  {1e3 / med[on]:7.1f} pairs/s  "
            f"{sync[on]} read-backs = {sync[on] / pairs:.2f} per pair   (rounds: {' '.join(f'{x:.2f}' for x in ms[on])})")
    say(f"    on / off = {med[True] / med[False]:.3f}x the time per pair; results off {res[False]} on {res[True]}")


def bench_validators(say, rounds, n_list):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = RAFT(Namespace(small=False, mixed_precision=False)).to(dev).eval()
    say("validators, RAFT-base fp32 (random weights), batch 1:")
    _timed_rounds(say, "validate_synthetic at its defaults (368 x 496, 24 iterations)",
                  lambda on: V.validate_synthetic(model, device_metrics=on), 16, rounds)
    for kind, iters in (("sintel", 32), ("kitti", 24)):
        H, W = CASES[kind]
        samples = []
        for s in range(n_list):
            i1, i2, flow, valid = synthetic_batch(1, H, W, seed=100 + s)
            samples.append((i1[0].contiguous(), i2[0].contiguous(), flow[0].contiguous(), valid[0].contiguous()))
        _timed_rounds(say, f"evaluate_samples over an in-memory list, {kind}: {H} x {W}, {iters} iterations",
                      lambda on: V.evaluate_samples(model, samples, kind, iters, device_metrics=on), n_list, rounds)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                   "profiles", "validation_bench.log"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=8, help="length of the in-memory sample lists")
    ap.add_argument("--skip_validators", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_validation.py measures on the GPU; none is available")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()

        say(f"device: {torch.cuda.get_device_name(0)}")
        say("op alone (back-to-back calls on the same buffers, which can stay in the 256 MiB Infinity Cache):")
        for kind in CASES:
            bench_op(say, kind, args.reps, args.rounds)
        if not args.skip_validators:
            bench_validators(say, args.rounds, args.samples)


if __name__ == "__main__":
    main()
