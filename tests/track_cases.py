"""Shared cases of the point-track tests: flow fields that exercise every fate of a point, a
per-slot loop oracle written independently of the vectorised reference, and the comparison.

The specification fixes every rounding step, so no tolerance applies: ``same`` is bitwise, with a
NaN equal to a NaN at the same place.
"""
import functools
import math

import numpy as np
import torch

from raft_ros_amd.ops.consistency import ALPHA1, ALPHA2
from raft_ros_amd.ops.track import seed_points, track_points_ref

NAMES = ("pos_out", "prev", "ids_out", "age_out", "epoch_out", "status", "err2", "counts")
STEPS = 4

# name -> (B, H, W, roi, S)
CASES = {
    "37x53_S8": (2, 37, 53, (0, 0, 53, 37), 8),        # 5 x 7 = 35 cells, partial edge cells
    "roi_in_40x56": (2, 40, 56, (1, 2, 53, 37), 8),    # the unpadded image inside a padded frame
    "5x7_S1": (1, 5, 7, (0, 0, 7, 5), 1),              # a point per pixel
    "64x96_S2": (3, 64, 96, (0, 0, 96, 64), 2),        # N = 1536: more than one scan chunk
    "one_cell": (2, 6, 9, (0, 0, 9, 6), 16),           # S larger than the image: N = 1
}


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equal (so that -0.0 is not 0.0), with NaN equal to NaN."""
    a, b = a.cpu(), b.cpu()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    na, nb = a.isnan(), b.isnan()
    z = torch.zeros((), dtype=a.dtype)
    return torch.equal(na, nb) and torch.equal(torch.where(na, z, a).contiguous().view(torch.int32),
                                               torch.where(nb, z, b).contiguous().view(torch.int32))


def check(got, want, what=""):
    assert len(got) == len(want) == len(NAMES)
    for name, g, w in zip(NAMES, got, want):
        if not same(g, w):
            g, w = g.cpu(), w.cpu()
            bad = (g != w) & ~(g.isnan() & w.isnan()) if g.dtype.is_floating_point else g != w
            idx = bad.nonzero()[:5].tolist() if bad.shape == g.shape else []
            raise AssertionError(f"{what}: {name} differs at {int(bad.sum())} places, first {idx}: "
                                 f"got {[g[tuple(i)].item() for i in idx]}, want {[w[tuple(i)].item() for i in idx]}")


def fields(B, H, W, roi, S, step):
    """(fw, bw) of (B, 2, H, W): a smooth drift whose direction alternates from step to step, a
    converging region (crowding), a strip on the right and one at the top that flow out of the roi,
    bw = -fw plus noise with a patch where it is unrelated, and non-finite pixels in both."""
    left, top, w, h = roi
    g = torch.Generator().manual_seed(1000 * step + 17 * H + W)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    amp = min(2.5, 0.07 * min(w, h))
    fws, bws = [], []
    for b in range(B):
        sign = 1.0 if (step + b) % 2 == 0 else -1.0
        u = sign * amp * (1.0 + 0.6 * torch.sin(2 * math.pi * y / H + step + b))
        v = amp * 0.4 * torch.cos(2 * math.pi * x / W + b)
        cx, cy, R = left + (0.35 + 0.1 * b) * w, top + 0.5 * h, max(1.5, 0.22 * min(w, h))
        conv = (x - cx) ** 2 + (y - cy) ** 2 <= R * R
        u, v = torch.where(conv, -0.7 * (x - cx), u), torch.where(conv, -0.7 * (y - cy), v)
        right = (x >= left + w - max(1, w // 10)) & (y >= top + h // 3)
        u = torch.where(right, torch.full_like(u, float(w)), u)
        upper = (y < top + max(1, h // 12)) & (x < left + w // 3)
        v = torch.where(upper, torch.full_like(v, -float(h)), v)
        fw = torch.stack([u, v])
        bw = -fw + 0.05 * torch.randn(2, H, W, generator=g)
        y0, y1, x0, x1 = top + int(0.6 * h), top + int(0.85 * h) + 1, left + int(0.55 * w), left + int(0.8 * w) + 1
        bw[:, y0:y1, x0:x1] += 3.0  # inconsistent
        if w * h >= 35:  # non-finite pixels, placed on seeds so that the first step reads them
            sx = [left + min(gx * S + S // 2, w - 1) for gx in range(-(-w // S))]
            sy = [top + min(gy * S + S // 2, h - 1) for gy in range(-(-h // S))]
            fw[0, sy[len(sy) // 2], sx[1 % len(sx)]] = float("nan")
            fw[1, sy[-1], sx[len(sx) // 2]] = float("inf")
            fw[0, sy[0], sx[-1]] = float("-inf")
            bw[0, sy[1 % len(sy)], sx[len(sx) // 2]] = float("nan")
            bw[1, sy[len(sy) // 2], sx[-1 - (len(sx) > 2)]] = float("inf")
            bw[0, sy[-1], sx[0]] = float("-inf")
        fws.append(fw)
        bws.append(bw)
    return torch.stack(fws).contiguous(), torch.stack(bws).contiguous()


def initial_state(B, roi, S):
    """``seed_points`` with a few positions replaced: non-finite ones and points exactly on the
    right and the lower edge of the roi, one of them between two pixels."""
    left, top, w, h = roi
    pos, ids, age, epoch = seed_points(B, roi, S)
    N = ids.shape[1]
    if N >= 8:
        pos[0, 1, 0] = float("nan")
        pos[0, 2, 0] = float("inf")
        pos[0, 3, 1] = float("-inf")
        pos[0, 4] = torch.tensor([left + w - 1.0, top + h - 1.0])
        pos[0, 5] = torch.tensor([left + w - 1.0, top + 0.5 * (h - 1)])
        pos[B - 1, 6] = torch.tensor([left + 0.25 * (w - 1), top + h - 1.0])
    return pos, ids, age, epoch


@functools.lru_cache(maxsize=None)
def case(name):
    """(B, H, W, roi, S, state, [(fw, bw)] * STEPS) on the host; treat as read-only."""
    B, H, W, roi, S = CASES[name]
    return B, H, W, roi, S, initial_state(B, roi, S), [fields(B, H, W, roi, S, k) for k in range(STEPS)]


def chain(step_fn, name, use_bw=True, device=None):
    """Runs ``step_fn(pos, ids, age, epoch, fw, bw, roi, S)`` over the steps of a case, its own
    outputs feeding the next step -> [(inputs, outputs)]."""
    B, H, W, roi, S, state, flows = case(name)
    state = tuple(t.clone() if device is None else t.to(device) for t in state)
    log = []
    for fw, bw in flows:
        fw = fw if device is None else fw.to(device)
        bw = None if not use_bw else (bw if device is None else bw.to(device))
        out = step_fn(*state, fw, bw, roi, S)
        log.append(((*state, fw, bw, roi, S), out))
        state = (out[0], out[2], out[3], out[4])
    return log


@functools.lru_cache(maxsize=None)
def reference_chain(name, use_bw=True):
    """The reference's own chain on the host, computed once."""
    return chain(track_points_ref, name, use_bw)


# ---------------------------------------------------------------------------- the loop oracle
def _bilinear(f, x, y):
    """Both components of f (2, H, W) numpy at the float32 scalars (x, y), every step rounded."""
    H, W = f.shape[1:]
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = x - x0f, y - y0f
    x0, y0 = int(x0f), int(y0f)
    x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
    out = []
    for c in range(2):
        a00, a01, a10, a11 = f[c, y0, x0], f[c, y0, x1], f[c, y1, x0], f[c, y1, x1]
        t = a00 + fx * (a01 - a00)
        b = a10 + fx * (a11 - a10)
        out.append(t + fy * (b - t))
    return out


def loop_oracle(pos, ids, age, epoch, fw, bw, roi, S, alpha1=ALPHA1, alpha2=ALPHA2):
    """One step, slot by slot on numpy.float32 scalars: a dict for the claims, lists for the
    matching.  Returns the outputs as torch tensors and the claims of every image
    ({cell: [(age, slot)]}) for the tests' conditions."""
    f32 = np.float32
    pos, ids, age = pos.numpy(), ids.numpy(), age.numpy()
    fw = fw.numpy()
    bw = None if bw is None else bw.numpy()
    B, N = ids.shape
    left, top, w, h = roi
    Gx, Gy = -(-w // S), -(-h // S)
    assert N == Gx * Gy
    a1, a2 = f32(alpha1), f32(alpha2)
    e = int(epoch.item())
    pos_out, prev = np.zeros((B, N, 2), f32), np.zeros((B, N, 2), f32)
    ids_out, age_out = np.zeros((B, N), np.int64), np.zeros((B, N), np.int32)
    status, err2 = np.zeros((B, N), np.uint8), np.zeros((B, N), f32)
    counts = np.zeros((B, 4), np.int32)
    all_claims = []

    def inside(x, y):
        return bool(x >= f32(left) and x <= f32(left + w - 1) and y >= f32(top) and y <= f32(top + h - 1))

    with np.errstate(all="ignore"):
        for b in range(B):
            claims, target, cell_of = {}, {}, {}
            for j in range(N):
                px, py = pos[b, j]
                status[b, j], err2[b, j] = 2, f32(np.inf)
                if not inside(px, py):
                    continue
                f0, f1 = _bilinear(fw[b], px, py)
                qx, qy = px + f0, py + f1
                if not inside(qx, qy):
                    continue
                if bw is not None:
                    s0, s1 = _bilinear(bw[b], qx, qy)
                    du, dv = f0 + s0, f1 + s1
                    err = du * du + dv * dv
                    thr = a1 * ((f0 * f0 + f1 * f1) + (s0 * s0 + s1 * s1)) + a2
                    ok = bool(err <= thr)
                else:
                    err, ok = f32(0), True
                err2[b, j] = err
                status[b, j] = 0 if ok else 1
                if ok:
                    c = ((int(np.floor(qy)) - top) // S) * Gx + (int(np.floor(qx)) - left) // S
                    assert 0 <= c < N
                    claims.setdefault(c, []).append((int(age[b, j]), j))
                    target[j], cell_of[j] = (qx, qy), c
            owner = {c: sorted(l, key=lambda t: (-t[0], t[1]))[0][1] for c, l in claims.items()}  # oldest, then lowest slot
            lost = []
            for j in range(N):
                if status[b, j] == 0 and owner[cell_of[j]] == j:
                    pos_out[b, j], prev[b, j] = target[j], pos[b, j]
                    ids_out[b, j], age_out[b, j] = ids[b, j], age[b, j] + 1
                else:
                    if status[b, j] == 0:
                        status[b, j] = 3
                    lost.append(j)
            free = [c for c in range(N) if c not in owner]
            assert len(free) == len(lost)
            for j, c in zip(lost, free):
                gy, gx = divmod(c, Gx)
                pos_out[b, j] = (left + min(gx * S + S // 2, w - 1), top + min(gy * S + S // 2, h - 1))
                prev[b, j] = np.nan
                ids_out[b, j], age_out[b, j] = e * N + j, 0
            counts[b] = [int((status[b] == k).sum()) for k in range(4)]
            all_claims.append(claims)
    out = (pos_out, prev, ids_out, age_out, np.array([e + 1], np.int64), status, err2, counts)
    return tuple(torch.from_numpy(o) for o in out), all_claims


# ---------------------------------------------------------------------------- the workload shape
@functools.lru_cache(maxsize=None)
def workload():
    """440 x 1024, S = 8, B = 2: the state and STEPS - 1 pairs of smooth fields (host tensors)."""
    B, H, W, S = 2, 440, 1024, 8
    roi = (0, 0, W, H)
    return B, H, W, roi, S, seed_points(B, roi, S), [fields(B, H, W, roi, S, k) for k in range(3)]
