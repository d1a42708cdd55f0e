"""Shared inputs of the sparse augmentation tests (test_augment_sparse_cpu.py,
test_augment_sparse_gpu.py): batches with sparse ground truth (KITTI, HD1K) for the HIP op
raft_amd::augment_batch_sparse, built on the helpers of augment_cases.py.

As there, every case is a small padded batch with its crop size and parameters written by hand,
and the oracle is the CPU torch path ``BatchAugmentor.apply`` (for a sparse sample's flow and
valid that is ``_sparse_flow``), computed once per case and shared.  A sparse sample's flow and
valid must equal the oracle bitwise: the arithmetic is integer work and one fp32 multiply.  Images
and dense samples are held to the caps of augment_cases.py by the case's ``kind``.

Each case is there for one branch of the scatter, and ``premise`` measures whether it still takes
that branch (how many sources share a target, how many products are exact .5 ties); the tests
assert it, so a case that stops exercising its branch fails.
"""
import functools
from typing import Dict, Tuple

import torch

import augment_cases as ac
from raft_ros_amd.data import augment as A

PERMS = ac.PERMS


def _blocky(sample):
    """The images made constant on aligned 2 x 2 blocks.  At sx = sy = 0.5 every bilinear blend is
    an exact quarter sum of a 2 x 2 block, where the oracle's rounding of the many .5 ties is decided
    by the 1e-5 px noise of grid_sample's normalised coordinates (see ``_general_rows`` of
    augment_cases.py).  The source coordinate of a crop pixel is 2 (origin + c) + 0.5 there, so its
    four taps are one such block: the blend is the block's value whatever the weights, and the image
    caps measure the op.  The case's eraser box has even edges for the same reason.  Flow and
    valid, what the case is about, are untouched."""
    for k in ("img1", "img2"):
        h, w = sample[k].shape[:2]
        sample[k] = sample[k][::2, ::2].repeat_interleave(2, 0).repeat_interleave(2, 1)[:h, :w].contiguous()
    return sample


def _down_half():
    # exact .5 ties of x * 0.5 pin the half-to-even rounding; up to 3 x 3 sources share a target
    crop = (64, 96)
    samples = [_blocky(ac.make_sample(140, 200, 600, sparse=True)), ac.make_sample(96, 130, 601)]
    rows = [ac.sample_params(140, 200, crop, o1=PERMS[5], f1=(0.85, 1.2, 1.1, 0.04), sx=0.5, sy=0.5, x0=3, y0="max",
                             boxes=((60, 40, 50, 60),), sparse=True),
            ac.sample_params(96, 130, crop, o1=PERMS[16], f1=(1.2, 0.8, 0.9, -0.08), asym=True, o2=PERMS[2],
                             f2=(0.9, 1.1, 1.25, 0.1), sx=1.0931, sy=1.2127, hflip=True, vflip=True, x0="mid", y0=2)]
    return ac.Case("down_half", "general", crop, samples, rows, sparse_ids=(0,))


def _down_flip_tail():
    # a crop width that is no multiple of 4; dense between two sparse samples of other region sizes;
    # the last one's crop starts at the origin, where the 0 < xn rule empties row 0 and column 0
    crop = (64, 97)
    samples = [ac.make_sample(120, 160, 610, sparse=True), ac.make_sample(110, 150, 611),
               ac.make_sample(100, 140, 612, sparse=True)]
    rows = [ac.sample_params(120, 160, crop, o1=PERMS[11], f1=(1.1, 0.9, 1.2, 0.06), sx=0.8713, sy=0.8713, hflip=True,
                             x0="max", y0="mid", boxes=ac._boxes(2, 120, 160, 40, 20), sparse=True),
            ac.sample_params(110, 150, crop, o1=PERMS[19], f1=(0.8, 1.25, 0.85, -0.1), sx=1.1, sy=0.95, vflip=True,
                             x0="mid", y0="mid", boxes=ac._boxes(1, 110, 150, 0, 0)),
            ac.sample_params(100, 140, crop, o1=PERMS[7], f1=(1.25, 1.1, 0.8, 0.12), sx=0.9317, sy=0.7731, x0=0, y0=0,
                             sparse=True)]
    return ac.Case("down_flip_tail", "general", crop, samples, rows, sparse_ids=(0, 2))


def _flat(sample):
    """The images made one colour each.  At sx = 1.7, sy = 1.3 the blend weights are multiples of
    1 / 34 and 1 / 26, short fractions again: the oracle with fp32 and with fp64 sampling differ at
    1.4e-3 of the pixel-channels of a smooth image there, above the cap itself.  A blend of one
    colour is that colour whatever the weights.  The case is about the holes in flow and valid."""
    for k, rgb in (("img1", (97, 180, 41)), ("img2", (200, 33, 120))):
        sample[k] = torch.tensor(rgb, dtype=torch.uint8).expand_as(sample[k]).contiguous()
    return sample


def _up_aniso():
    # above scale 1 the scatter leaves holes and nothing collides; sx != sy
    crop = (64, 96)
    samples = [_flat(ac.make_sample(100, 150, 620, sparse=True))]
    rows = [ac.sample_params(100, 150, crop, o1=PERMS[22], f1=(0.9, 1.15, 1.05, -0.03), sx=1.7, sy=1.3, x0=0, y0=0,
                             boxes=ac._boxes(3, 100, 150, 0, 0), sparse=True)]
    return ac.Case("up_aniso", "general", crop, samples, rows, sparse_ids=(0,))


def _noresize():
    # not resized: nothing is dropped, row 0 and column 0 of the source survive
    crop = (64, 96)
    samples = [ac.make_sample(100, 150, 630, noise=True, sparse=True), ac.make_sample(120, 160, 631, noise=True, sparse=True)]
    rows = [ac.sample_params(100, 150, crop, o1=PERMS[1], f1=(1.3, 0.75, 1.1, 0.08), x0=0, y0=0,
                             boxes=ac._boxes(2, 100, 150, 0, 0), sparse=True),
            ac.sample_params(120, 160, crop, o1=PERMS[14], f1=(0.7, 1.2, 0.9, -0.12), hflip=True, x0="max", y0="max",
                             boxes=ac._boxes(1, 120, 160, 0, 0), sparse=True)]
    return ac.Case("noresize", "exact", crop, samples, rows, sparse_ids=(0, 1))


def _edge_valid():
    # valid all zero -> all-zero flow and valid; valid of 0, 0.5 and 1 -> only >= 1 counts
    crop = (64, 96)
    samples = [ac.make_sample(100, 150, 640, sparse=True), ac.make_sample(110, 140, 641, sparse=True)]
    samples[0]["valid"] = torch.zeros(100, 150)
    g = torch.Generator().manual_seed(642)
    samples[1]["valid"] = torch.randint(0, 3, (110, 140), generator=g).float() / 2
    rows = [ac.sample_params(100, 150, crop, o1=PERMS[9], f1=(1.05, 0.95, 1.2, 0.02), sx=0.8713, sy=0.8713, x0="mid", y0="mid",
                             sparse=True),
            ac.sample_params(110, 140, crop, o1=PERMS[18], f1=(0.9, 1.1, 0.8, -0.05), sx=0.9317, sy=0.9317, hflip=True,
                             x0="max", y0=3, sparse=True)]
    return ac.Case("edge_valid", "general", crop, samples, rows, sparse_ids=(0, 1))


CASE_NAMES = ["down_half", "down_flip_tail", "up_aniso", "noresize", "edge_valid"]


@functools.lru_cache(maxsize=None)
def all_cases() -> Tuple[ac.Case, ...]:
    return (_down_half(), _down_flip_tail(), _up_aniso(), _noresize(), _edge_valid())


def get_case(name: str) -> ac.Case:
    return {c.name: c for c in all_cases()}[name]


@functools.lru_cache(maxsize=None)
def oracle(name: str, mean_dtype=torch.float32):
    """The CPU torch path on the case: (img1, img2, flow, valid).  Shared, not to be modified."""
    case = get_case(name)
    return A.BatchAugmentor(case.specs, device="cpu").apply(case.batch, case.params, mean_dtype=mean_dtype)


def premise(case: ac.Case, i: int, thresh: float = 1.0) -> Dict[str, object]:
    """What sparse sample i of the case exercises, counted on the CPU with integer loops over the
    sources, apart from ``_sparse_flow``:

    * ``count``  (ch, cw) long, the sources with valid >= thresh (the op's rule is 1) that land on
      each crop pixel;
    * ``ties``   how many columns x have x * sx exactly on .5 (in fp32), resized samples only;
    * ``row0``, ``col0``  valid source pixels in the source's row 0 and column 0."""
    p = case.params
    ch, cw = case.crop
    h, w = case.sizes[i]
    valid = case.samples[i]["valid"]
    ok = (valid >= thresh).tolist()
    sx, sy = p["sx"][i], p["sy"][i]
    resize, hflip = bool(p["resize"][i]), bool(p["hflip"][i])
    rh, rw, x0, y0 = (int(p[k][i]) for k in ("rh", "rw", "x0", "y0"))
    xf = torch.arange(w).float() * sx if resize else torch.arange(w).float()
    yf = torch.arange(h).float() * sy if resize else torch.arange(h).float()
    xn, yn = torch.round(xf).long().tolist(), torch.round(yf).long().tolist()
    count = torch.zeros(ch, cw, dtype=torch.long)
    for y in range(h):
        for x in range(w):
            if not ok[y][x]:
                continue
            tx, ty = xn[x], yn[y]
            if resize and not (0 < tx < rw and 0 < ty < rh):
                continue
            if hflip:
                tx = rw - 1 - tx
            cx, cy = tx - x0, ty - y0
            if 0 <= cx < cw and 0 <= cy < ch:
                count[cy, cx] += 1
    ties = int(((xf - torch.floor(xf)) == 0.5).sum()) if resize else 0
    return {"count": count, "ties": ties, "row0": int((valid[0] >= 1).sum()), "col0": int((valid[:, 0] >= 1).sum())}
