"""Validation and benchmark-submission writers (reference evaluate.py:21-166).

* ``validate_chairs`` (24 iterations, EPE), ``validate_sintel`` (32 iterations,
  clean + final: EPE and 1/3/5 px rates, centred padding), ``validate_kitti``
  (24 iterations, bottom padding; EPE = mean of per-image means, F1 = % of
  valid pixels with epe > 3 and epe/|gt| > 0.05);
* ``create_sintel_submission`` (optional warm start: the device forward splat of
  ``ops/warm_start.py`` on a GPU, ``forward_interpolate`` on the CPU)
  and ``create_kitti_submission``;
* ``validate_synthetic`` -- the same EPE protocol on generated pairs with exact
  ground truth, for environments without the datasets;
* ``device_metrics=True`` keeps the metrics on the model's device: the padded prediction goes to
  ``ops/metrics.py`` (the HIP op ``raft_amd::flow_metrics`` on a GPU) and a ``MetricAccumulator``
  adds up there, so nothing is read back until the dataset is finished.  ``evaluate_samples``
  holds the loop bodies and takes any sequence of samples.

Differences from the reference: the device is a parameter (not hard-coded
``.cuda()``), inference runs under ``torch.inference_mode``, and under DDP the
validation set is sharded over ranks with the per-pixel statistics reduced
exactly (sums and counts, not means of means).
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from ..data import datasets, frame_utils
from ..data.synthetic import synthetic_batch
from ..ops.metrics import flow_metrics
from ..ops.warm_start import forward_splat_nearest
from ..utils.utils import InputPadder, forward_interpolate


def _device(model) -> torch.device:
    return next(model.parameters()).device


def _shard(n: int, rank: int, world: int):
    return range(rank, n, world)


def _reduce(vals, device, world):
    t = torch.tensor(vals, dtype=torch.float64, device=device)
    if world > 1:
        torch.distributed.all_reduce(t)
    return t.tolist()


@torch.inference_mode()
def create_sintel_submission(model, iters=32, warm_start=False, output_path="sintel_submission"):
    """Write .flo files for the Sintel test set (clean + final)."""
    model.eval()
    dev = _device(model)
    for dstype in ["clean", "final"]:
        test_dataset = datasets.MpiSintel(split="test", aug_params=None, dstype=dstype)
        flow_prev, sequence_prev = None, None
        for test_id in range(len(test_dataset)):
            image1, image2, (sequence, frame) = test_dataset[test_id]
            if sequence != sequence_prev:
                flow_prev = None
            padder = InputPadder(image1.shape)
            image1, image2 = padder.pad(image1[None].to(dev), image2[None].to(dev))
            flow_low, flow_pr = model(image1, image2, iters=iters, flow_init=flow_prev, test_mode=True)
            flow = padder.unpad(flow_pr[0]).permute(1, 2, 0).cpu().numpy()
            if warm_start and dev.type == "cuda":
                flow_prev = forward_splat_nearest(flow_low)  # HIP splat: no host round trip
            elif warm_start:
                flow_prev = forward_interpolate(flow_low[0])[None].to(dev)
            output_dir = os.path.join(output_path, dstype, sequence)
            os.makedirs(output_dir, exist_ok=True)
            frame_utils.writeFlow(os.path.join(output_dir, "frame%04d.flo" % (frame + 1)), flow)
            sequence_prev = sequence


@torch.inference_mode()
def create_kitti_submission(model, iters=24, output_path="kitti_submission"):
    """Write 16-bit PNG flow files for the KITTI-2015 test set."""
    model.eval()
    dev = _device(model)
    test_dataset = datasets.KITTI(split="testing", aug_params=None)
    os.makedirs(output_path, exist_ok=True)
    for test_id in range(len(test_dataset)):
        image1, image2, (frame_id,) = test_dataset[test_id]
        padder = InputPadder(image1.shape, mode="kitti")
        image1, image2 = padder.pad(image1[None].to(dev), image2[None].to(dev))
        _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
        flow = padder.unpad(flow_pr[0]).permute(1, 2, 0).cpu().numpy()
        frame_utils.writeFlowKITTI(os.path.join(output_path, frame_id), flow)


class MetricAccumulator:
    """Validation metrics summed on the device: ``update`` issues no synchronisation, ``result``
    performs the one read-back (after an all-reduce under DDP).

    ``epe_sum`` float64 and ``counts`` int64 (5,) (ops/metrics.py COUNT_NAMES) are per pixel;
    ``mean_sum`` float64 is the sum of the per-image mean EPE (KITTI's protocol; an image without
    a counted pixel gives NaN, as ``epe[val].mean()`` does) and ``images`` their number."""

    def __init__(self, device):
        self.epe_sum = torch.zeros((), dtype=torch.float64, device=device)
        self.counts = torch.zeros(5, dtype=torch.int64, device=device)
        self.mean_sum = torch.zeros((), dtype=torch.float64, device=device)
        self.images = torch.zeros((), dtype=torch.int64, device=device)

    def update(self, flow_pr, flow_gt, valid=None, padder=None) -> None:
        """Add one image or one batch: the (padded) prediction against its ground truth."""
        epe_sum, counts = flow_metrics(flow_pr, flow_gt, valid, padder)
        if epe_sum.dim() == 0:
            epe_sum, counts = epe_sum[None], counts[None]
        self.epe_sum += epe_sum.sum()
        self.counts += counts.sum(dim=0)
        self.mean_sum += (epe_sum / counts[:, 0]).sum()
        self.images += epe_sum.shape[0]

    def result(self, world: int = 1) -> Dict[str, float]:
        """The totals on the host.  The integers travel as float64 (exact below 2^53)."""
        t = torch.cat([self.epe_sum[None], self.mean_sum[None], self.images[None].double(), self.counts.double()])
        if world > 1:
            torch.distributed.all_reduce(t)
        v = t.tolist()
        epe_sum, mean_sum, images, counts = v[0], v[1], int(v[2]), [int(c) for c in v[3:]]
        cnt = max(counts[0], 1)
        return {"epe_sum": epe_sum, "mean_sum": mean_sum, "images": images, "counts": counts,
                "epe": epe_sum / cnt, "1px": counts[1] / cnt, "3px": counts[2] / cnt, "5px": counts[3] / cnt,
                "mean-epe": mean_sum / max(images, 1), "f1": 100 * counts[4] / cnt}


def _padder(kind, shape):
    if kind == "chairs":
        return None
    return InputPadder(shape, mode="kitti") if kind == "kitti" else InputPadder(shape)


def _rank_samples(samples, rank, world, workers, pin):
    """This rank's shard of a dataset or sequence, through a DataLoader when ``workers > 0`` (the
    decoding then runs ahead of the model).  Anything without ``__getitem__`` is iterated as it is."""
    if not hasattr(samples, "__getitem__"):
        return samples
    idx = list(_shard(len(samples), rank, world))
    if workers > 0:
        return torch.utils.data.DataLoader(torch.utils.data.Subset(samples, idx), batch_size=None, shuffle=False,
                                           num_workers=workers, pin_memory=pin)
    return (samples[i] for i in idx)


def _upload(t, dev):
    """Ground truth to the model's device without blocking the host (pinned on a GPU)."""
    if dev.type != "cuda":
        return t
    return (t if t.is_pinned() else t.pin_memory()).to(dev, non_blocking=True)


@torch.inference_mode()
def evaluate_samples(model, samples: Iterable, kind: str, iters: int, rank=0, world=1, device_metrics=False,
                     workers=0) -> Dict[str, float]:
    """The loop of one validator over ``samples`` of (image1, image2, flow_gt, valid): a dataset
    or any sequence (sharded over the ranks), or a plain iterable (taken as this rank's share).

    ``kind``: "chairs" (no padding; ``epe``), "sintel" (centred padding; ``epe``, ``1px``,
    ``3px``, ``5px``) or "kitti" (bottom padding, ``valid``; ``kitti-epe``, ``kitti-f1``).  The
    model runs at batch 1 either way; ``device_metrics`` only moves the metrics."""
    if kind not in ("chairs", "sintel", "kitti"):
        raise ValueError(f"evaluate_samples: unknown kind {kind!r}")
    model.eval()
    dev = _device(model)
    it = _rank_samples(samples, rank, world, workers, pin=device_metrics and dev.type == "cuda")
    if device_metrics:
        acc = MetricAccumulator(dev)
        for image1, image2, flow_gt, valid_gt in it:
            image1, image2 = image1[None].to(dev), image2[None].to(dev)
            padder = _padder(kind, image1.shape)
            if padder is not None:
                image1, image2 = padder.pad(image1, image2)
            _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
            acc.update(flow_pr, _upload(flow_gt, dev)[None], _upload(valid_gt, dev)[None] if kind == "kitti" else None,
                       padder)
        r = acc.result(world)
        if kind == "kitti":
            return {"kitti-epe": r["mean-epe"], "kitti-f1": r["f1"]}
        return {"epe": r["epe"]} if kind == "chairs" else {k: r[k] for k in ("epe", "1px", "3px", "5px")}
    if kind == "chairs":
        s = n = 0.0
        for image1, image2, flow_gt, _ in it:
            _, flow_pr = model(image1[None].to(dev), image2[None].to(dev), iters=iters, test_mode=True)
            epe = torch.sum((flow_pr[0].float().cpu() - flow_gt) ** 2, dim=0).sqrt()
            s += epe.sum().item()
            n += epe.numel()
        s, n = _reduce([s, n], dev, world)
        return {"epe": s / max(n, 1)}
    if kind == "sintel":
        acc = np.zeros(5)  # sum epe, count, <1, <3, <5
        for image1, image2, flow_gt, _ in it:
            image1, image2 = image1[None].to(dev), image2[None].to(dev)
            padder = InputPadder(image1.shape)
            image1, image2 = padder.pad(image1, image2)
            _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
            flow = padder.unpad(flow_pr[0]).float().cpu()
            epe = torch.sum((flow - flow_gt) ** 2, dim=0).sqrt().view(-1)
            acc += [epe.sum().item(), epe.numel(), (epe < 1).sum().item(), (epe < 3).sum().item(),
                    (epe < 5).sum().item()]
        acc = np.array(_reduce(acc.tolist(), dev, world))
        cnt = max(acc[1], 1)
        return {"epe": acc[0] / cnt, "1px": acc[2] / cnt, "3px": acc[3] / cnt, "5px": acc[4] / cnt}
    acc = np.zeros(4)  # sum of per-image epe means, images, outliers, valid pixels
    for image1, image2, flow_gt, valid_gt in it:
        image1, image2 = image1[None].to(dev), image2[None].to(dev)
        padder = InputPadder(image1.shape, mode="kitti")
        image1, image2 = padder.pad(image1, image2)
        _, flow_pr = model(image1, image2, iters=iters, test_mode=True)
        flow = padder.unpad(flow_pr[0]).float().cpu()
        epe = torch.sum((flow - flow_gt) ** 2, dim=0).sqrt().view(-1)
        mag = torch.sum(flow_gt ** 2, dim=0).sqrt().view(-1)
        val = valid_gt.view(-1) >= 0.5
        out = ((epe > 3.0) & ((epe / mag) > 0.05)).float()
        acc += [epe[val].mean().item(), 1, out[val].sum().item(), val.sum().item()]
    acc = _reduce(acc.tolist(), dev, world)
    return {"kitti-epe": acc[0] / max(acc[1], 1), "kitti-f1": 100 * acc[2] / max(acc[3], 1)}


def validate_chairs(model, iters=24, rank=0, world=1, device_metrics=False, workers=0) -> Dict[str, float]:
    """EPE on the FlyingChairs validation split."""
    val_dataset = datasets.FlyingChairs(split="validation")
    epe = evaluate_samples(model, val_dataset, "chairs", iters, rank, world, device_metrics, workers)["epe"]
    if rank == 0:
        print("Validation Chairs EPE: %f" % epe)
    return {"chairs": epe}


def validate_sintel(model, iters=32, rank=0, world=1, device_metrics=False, workers=0) -> Dict[str, float]:
    """EPE and 1/3/5-px rates on the Sintel training split (clean and final)."""
    results = {}
    for dstype in ["clean", "final"]:
        val_dataset = datasets.MpiSintel(split="training", dstype=dstype)
        r = evaluate_samples(model, val_dataset, "sintel", iters, rank, world, device_metrics, workers)
        if rank == 0:
            print("Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (dstype, r["epe"], r["1px"], r["3px"], r["5px"]))
        results[dstype] = r["epe"]
    return results


def validate_kitti(model, iters=24, rank=0, world=1, device_metrics=False, workers=0) -> Dict[str, float]:
    """KITTI-2015 training split: EPE (mean of per-image means) and F1-all (%)."""
    val_dataset = datasets.KITTI(split="training")
    r = evaluate_samples(model, val_dataset, "kitti", iters, rank, world, device_metrics, workers)
    if rank == 0:
        print("Validation KITTI: %f, %f" % (r["kitti-epe"], r["kitti-f1"]))
    return r


@torch.inference_mode()
def validate_synthetic(model, iters=24, n_pairs=16, size=(368, 496), seed=12345, rank=0, world=1,
                       max_disp=20.0, device_metrics=False, workers=0) -> Dict[str, float]:
    """EPE / 1/3/5 px on generated pairs with exact ground truth (no dataset needed).  The pairs
    are generated on the model's device: ``workers`` has nothing to decode."""
    model.eval()
    dev = _device(model)
    if device_metrics:
        dacc = MetricAccumulator(dev)
        for i in _shard(n_pairs, rank, world):
            i1, i2, flow, valid = synthetic_batch(1, size[0], size[1], max_disp=max_disp, seed=seed + i, device=dev)
            _, flow_pr = model(i1, i2, iters=iters, test_mode=True)
            dacc.update(flow_pr, flow, valid)
        r = dacc.result(world)
        res = {"synthetic-epe": r["epe"], "synthetic-1px": r["1px"], "synthetic-3px": r["3px"],
               "synthetic-5px": r["5px"]}
    else:
        acc = np.zeros(5)
        for i in _shard(n_pairs, rank, world):
            i1, i2, flow, valid = synthetic_batch(1, size[0], size[1], max_disp=max_disp, seed=seed + i, device=dev)
            _, flow_pr = model(i1, i2, iters=iters, test_mode=True)
            epe = torch.sum((flow_pr.float() - flow) ** 2, dim=1).sqrt()[valid >= 0.5]
            acc += [epe.sum().item(), epe.numel(), (epe < 1).sum().item(), (epe < 3).sum().item(), (epe < 5).sum().item()]
        acc = np.array(_reduce(acc.tolist(), dev, world))
        cnt = max(acc[1], 1)
        res = {"synthetic-epe": acc[0] / cnt, "synthetic-1px": acc[2] / cnt, "synthetic-3px": acc[3] / cnt,
               "synthetic-5px": acc[4] / cnt}
    if rank == 0:
        print("Validation (synthetic) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % tuple(
            res[k] for k in ("synthetic-epe", "synthetic-1px", "synthetic-3px", "synthetic-5px")))
    return res


VALIDATORS = {"chairs": validate_chairs, "sintel": validate_sintel, "kitti": validate_kitti,
              "synthetic": validate_synthetic}


def run_validation(model, names, rank=0, world=1, device_metrics=False, workers=0) -> Dict[str, float]:
    results: Dict[str, float] = {}
    for name in names or []:
        if device_metrics or workers:
            results.update(VALIDATORS[name](model, rank=rank, world=world, device_metrics=device_metrics,
                                            workers=workers))
        else:
            results.update(VALIDATORS[name](model, rank=rank, world=world))
    return results
