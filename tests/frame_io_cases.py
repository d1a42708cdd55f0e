"""Inputs, host references and the acceptance rule shared by test_frame_io_cpu.py / _gpu.py."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import golden
from raft_ros_amd.utils import flow_viz

MAX_LEVELS = 1       # largest |difference| of a channel, in levels
MAX_SHARE = 1e-3     # share of an image's pixels that may differ at all (at least one pixel)


def host_image(flow: torch.Tensor, clip_flow=None, bgr=False) -> np.ndarray:
    """numpy colour coding of a (2, H, W) flow's host copy: the reference of every colour test."""
    return flow_viz.flow_to_image(flow.detach().float().cpu().permute(1, 2, 0).numpy(), clip_flow, bgr)


def check_colors(got, want, what=""):
    """The colour rule: every channel within MAX_LEVELS, at most max(1, MAX_SHARE * H * W) pixels differ."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, got.dtype, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    n_diff, cap = int((d.max(axis=-1) > 0).sum()), max(1, MAX_SHARE * want.shape[0] * want.shape[1])
    print(f"{what}: max |diff| {int(d.max()) if d.size else 0} levels, {n_diff} of {want.shape[0] * want.shape[1]} "
          f"pixels differ (cap {cap:g})")
    assert d.max() <= MAX_LEVELS, f"{what}: a channel differs by {int(d.max())} levels"
    assert n_diff <= cap, f"{what}: {n_diff} pixels differ, cap {cap:g}"


def parity_flow() -> torch.Tensor:
    """The 37 x 41 field of tests/golden/flow_viz.npz as (2, H, W)."""
    return torch.from_numpy(golden.parity_helpers()[1]()).permute(2, 0, 1).contiguous()


def scaled_batch() -> torch.Tensor:
    """B = 3 of 37 x 41 (odd H * W: unaligned image bases) with maxima 1 : 5 : 40."""
    f = parity_flow() / 5
    return torch.stack([f, f.flip(1) * 5, f.flip(2) * 40])


def gaussian(h, w, sigma, seed=0) -> torch.Tensor:
    return torch.randn(2, h, w, generator=torch.Generator().manual_seed(seed)) * sigma


def axes_field() -> torch.Tensor:
    """16 x 16 integer components u = x - 8, v = y - 8: both axes (u = 0 with v != 0, v = +0.0 with
    u < 0 and u > 0), the origin, all quadrants; the last row is v = -0.0."""
    r = torch.arange(-8.0, 8.0)
    u, v = r[None, :].expand(16, 16).clone(), r[:, None].expand(16, 16).clone()
    v[15] = -0.0
    return torch.stack([u, v])


def outlier_field() -> torch.Tensor:
    f = gaussian(64, 64, 2.0, seed=3)
    f[0, 17, 29] = 1e4
    return f


def nonfinite_field() -> torch.Tensor:
    f = gaussian(9, 13, 4.0, seed=4)
    f[0, 2, 3], f[1, 4, 5], f[0, 6, 7], f[1, 8, 12] = float("nan"), float("inf"), float("-inf"), float("nan")
    return f


@functools.lru_cache(maxsize=None)
def workload():
    """(flow, host image) of the 440 x 1024 Gaussian field, sigma = 8; the reference is computed once."""
    f = gaussian(440, 1024, 8.0, seed=1)
    return f, host_image(f)


def frames(n, h, w, seed=0) -> torch.Tensor:
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def pad_ref(fr: torch.Tensor, pads) -> torch.Tensor:
    return F.pad(fr.cpu().permute(0, 3, 1, 2).float(), list(pads), mode="replicate")
