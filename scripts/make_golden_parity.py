#!/usr/bin/env python3
"""Recorded outputs of the reference implementation for the CPU parity tests (run once, on CPU).

    python scripts/make_golden_parity.py --reference /path/to/reference/checkout

The reference is imported read-only (no bytecode written).  Written under ``tests/golden/``:

* ``chairs_split.txt``: the reference's FlyingChairs train/val split file, as it is;
* ``flow_viz.npz``: its colour wheel and ``flow_to_image`` (RGB and BGR) of ``viz_flow()``;
* ``raft_parity_{small,base}.npz``: for the seed-0 random-init model (``torch.manual_seed(0)`` before
  the constructor; our ``RAFT`` consumes the RNG identically -- asserted here, and a per-tensor
  checksum is stored) and the images of ``parity_images(128, 160)``: ``flow_low`` / ``flow_up`` of a
  3-iteration ``test_mode`` forward and the 2 predictions of a 2-iteration training-mode forward,
  complete, fp32;
* ``raft_grads_small_<i>.npy`` + ``raft_grads_small.json``: every parameter gradient of
  ``sum(p.abs().mean() for p in model(i1, i2, iters=2))`` for the seed-1 small model in train mode
  on ``parity_images(128, 128)``, complete, fp32, concatenated in ``named_parameters()`` order and
  cut into files below 1 MiB; the json lists the parameter names and sizes.

Consumed by tests/test_model_cpu.py, tests/test_io_cpu.py and tests/test_ops_cpu.py through
tests/golden.py.
"""
from __future__ import annotations

import argparse
import importlib
import importlib.util
import json
import os
import shutil
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
GRAD_CHUNK = 250_000  # fp32 elements per file: just under 1 MiB


def parity_images(h: int, w: int):
    """The two input images of the parity tests: uniform noise in [0, 255) from a fixed generator."""
    g = torch.Generator().manual_seed(1234)
    return torch.rand(1, 3, h, w, generator=g) * 255, torch.rand(1, 3, h, w, generator=g) * 255


def viz_flow():
    return np.random.default_rng(0).normal(size=(37, 41, 2)).astype(np.float32) * 5


def checksums(model) -> dict:
    return {k: float((v.double() ** 2).sum()) for k, v in model.state_dict().items() if v.dtype.is_floating_point}


def _args(small):
    return Namespace(small=small, mixed_precision=False, alternate_corr=False)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation")
    ref_root = os.path.abspath(ap.parse_args().reference)
    sys.dont_write_bytecode = True
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.path.append(ref_root)
    ref_raft = importlib.import_module("core.raft")
    sys.path.insert(0, ROOT)
    from raft_ros_amd.models import RAFT

    os.makedirs(OUT, exist_ok=True)
    shutil.copyfile(os.path.join(ref_root, "chairs_split.txt"), os.path.join(OUT, "chairs_split.txt"))

    spec = importlib.util.spec_from_file_location("ref_flow_viz", os.path.join(ref_root, "core", "utils", "flow_viz.py"))
    viz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(viz)
    flow = viz_flow()
    np.savez_compressed(os.path.join(OUT, "flow_viz.npz"), colorwheel=viz.make_colorwheel(),
                        rgb=viz.flow_to_image(flow, convert_to_bgr=False),
                        bgr=viz.flow_to_image(flow, convert_to_bgr=True))

    def seeded(seed, small):
        torch.manual_seed(seed)
        ref = ref_raft.RAFT(_args(small))
        torch.manual_seed(seed)
        ours = RAFT(_args(small)).state_dict()
        assert all(torch.equal(ours[k], v) for k, v in ref.state_dict().items()), "init parity"
        return ref

    for name, small in (("small", True), ("base", False)):
        ref = seeded(0, small).eval()
        i1, i2 = parity_images(128, 160)
        with torch.no_grad():
            lo, up = ref(i1, i2, iters=3, test_mode=True)
            preds = ref(i1, i2, iters=2)
        out = {f"ck/{k}": np.array(v) for k, v in checksums(ref).items()}
        out.update(flow_low=lo.numpy(), flow_up=up.numpy(), pred0=preds[0].numpy(), pred1=preds[1].numpy())
        np.savez(os.path.join(OUT, f"raft_parity_{name}.npz"), **out)

    ref = seeded(1, True).train()
    i1, i2 = parity_images(128, 128)
    sum(p.abs().mean() for p in ref(i1, i2, iters=2)).backward()
    named = [(n, p.grad) for n, p in ref.named_parameters() if p.grad is not None]
    flat = torch.cat([g.reshape(-1) for _, g in named]).numpy().astype(np.float32)
    chunks = [flat[i:i + GRAD_CHUNK] for i in range(0, flat.size, GRAD_CHUNK)]
    for i, c in enumerate(chunks):
        np.save(os.path.join(OUT, f"raft_grads_small_{i}.npy"), c)
    with open(os.path.join(OUT, "raft_grads_small.json"), "w") as f:
        json.dump({"chunks": len(chunks), "params": [[n, g.numel()] for n, g in named],
                   "ck": checksums(ref)}, f, indent=0)
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
