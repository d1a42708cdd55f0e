"""Seeded inputs, built on the host, and float64 / plain-torch oracles for the small streaming
kernels: the fused sequence loss (csrc/seq_loss.hip), the NHWC instance norm
(csrc/instance_norm.hip) and the update-block helpers (csrc/update_aux.hip).  Shared by
test_small_kernels_cpu.py / _gpu.py; nothing here touches the native extension.

Numbers an op takes as fp32 (``gamma``, ``max_flow``) and tensors it reads as bf16 are rounded to
that format first: the oracles compute, in float64, on the inputs as stored.
"""
import functools

import numpy as np
import torch

K_MAX_PREDS = 32  # csrc/kernel_abi.h kMaxPreds
LOSS_GRID_CAP = 2048 * 256  # seq_loss.hip loss_grid(): above this many pixels the grid-stride loop runs
EPE_STEPS = (1.0, 3.0, 5.0)

# (B, H, W, n, gamma, max_flow)
LOSS_CASES = {
    "stride": (3, 509, 515, 2, 0.8, 400.0),  # 786 405 px: half the lanes take a second stride step
    "cap": (2, 513, 512, 1, 0.8, 400.0),  # 525 312 px: a 1024-pixel second pass
    "one": (1, 1, 1, 1, 0.8, 400.0),
    "maxpreds": (1, 5, 7, K_MAX_PREDS, 0.8, 400.0),
    "params": (2, 40, 56, 12, 0.85, 50.0),
}
LOSS_CLASS_PIXELS = 12  # pixels one block of explicit classes takes (loss_case)


def f32(v: float) -> float:
    return float(np.float32(v))


# ------------------------------------------------------------------------------ sequence loss
def seq_loss_oracle(preds, gt, valid, gamma, max_flow, upstream=1.0):
    """float64 sequence loss of the reference formula: ``loss = sum_k gamma^(n-1-k) *
    mean(mask * |p_k - gt|)``, ``mask = (valid >= 0.5) & (|gt| < max_flow)``.  Returns the loss,
    the six raw sums {weighted L1, sum epe, #<1px, #<3px, #<5px, #valid} (metrics of the last
    prediction), the mask, and every prediction's gradient for the upstream gradient."""
    g, mf = f32(gamma), f32(max_flow)
    n = len(preds)
    gt64 = gt.double()
    mask = (valid.double() >= 0.5) & (gt64.pow(2).sum(1).sqrt() < mf)
    m = mask[:, None].double()
    w = [g ** (n - 1 - k) for k in range(n)]
    l1 = sum(w[k] * (m * (preds[k].double() - gt64).abs()).sum() for k in range(n))
    epe = (preds[-1].double() - gt64).pow(2).sum(1).sqrt()
    sums = [l1, (epe * mask).sum()] + [((epe < t) & mask).sum().double() for t in EPE_STEPS] + [mask.sum().double()]
    denom = float(gt.numel())  # B * 2 * H * W
    grads = [upstream * w[k] / denom * m * torch.sign(preds[k].double() - gt64) for k in range(n)]
    return {"loss": l1 / denom, "sums": torch.stack([s.double() for s in sums]), "mask": mask, "grads": grads,
            "weights": w}


def _class_block(gt, valid, preds, base, max_flow):
    """Writes LOSS_CLASS_PIXELS explicit pixels from flat pixel index ``base`` on: every mask class,
    sign(0) in one and in both components, and epe of exactly 1, 3 and 5.  Values are small dyadic
    numbers, so every difference and every square root in them is exact in fp32."""
    B, _, H, W = gt.shape
    HW = H * W
    g, v = gt.view(B, 2, HW), valid.view(B, HW)
    ps = [p.view(B, 2, HW) for p in preds]

    def put(j, gu, gv, val, du, dv):
        b, s = divmod(base + j, HW)
        g[b, 0, s], g[b, 1, s], v[b, s] = gu, gv, val
        for k, p in enumerate(ps):  # the last prediction carries (du, dv); earlier ones twice that
            f = 1.0 if k == len(ps) - 1 else 2.0
            p[b, 0, s], p[b, 1, s] = gu + f * du, gv + f * dv

    put(0, 1.5, -2.25, 0.0, 0.5, -0.5)  # valid < 0.5
    put(1, 1.5, -2.25, 0.49999997, 0.5, -0.5)  # the fp32 number just below 0.5
    put(2, 1.5, -2.25, 0.5, 0.5, -0.5)  # valid == 0.5 counts
    put(3, 0.6 * max_flow, 0.8 * max_flow, 1.0, 0.5, -0.5)  # |gt| == max_flow exactly: masked
    put(4, max_flow + 1.0, 0.0, 1.0, 0.5, -0.5)  # |gt| > max_flow
    put(5, 0.5 * max_flow, 0.0, 1.0, 0.5, -0.5)  # well inside
    put(6, 1.5, -2.25, 1.0, 0.0, 0.75)  # pred == gt in u only
    put(7, 1.5, -2.25, 1.0, -0.75, 0.0)  # pred == gt in v only
    put(8, 1.5, -2.25, 1.0, 0.0, 0.0)  # pred == gt in both
    put(9, 1.5, -2.25, 1.0, 1.0, 0.0)  # epe == 1: not < 1
    put(10, 1.5, -2.25, 1.0, 0.0, -3.0)  # epe == 3
    put(11, 1.5, -2.25, 1.0, -3.0, 4.0)  # epe == 5


def class_bases(B, H, W):
    """Flat pixel indices at which a block of explicit classes starts: the first pixels, a block
    that straddles the first image boundary, and for a field above the grid cap also the first
    pixels of the second stride step and the last pixels."""
    P, HW = B * H * W, H * W
    if P < LOSS_CLASS_PIXELS:
        return []
    bases = [0]
    if B > 1 and HW >= 2 * LOSS_CLASS_PIXELS:
        bases.append(HW - LOSS_CLASS_PIXELS // 2)
    if P > LOSS_GRID_CAP + 2 * LOSS_CLASS_PIXELS:
        bases += [LOSS_GRID_CAP, P - LOSS_CLASS_PIXELS]
    return bases


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """(preds, gt, valid, gamma, max_flow) fp32 on the host.  Random pixels keep their |gt| and the
    last prediction's epe at least 1e-3 away from the thresholds, so that fp32 and float64 agree on
    every comparison; equality is exercised by the explicit pixels of ``_class_block`` only."""
    B, H, W, n, gamma, max_flow = LOSS_CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    gt = torch.randn(B, 2, H, W, generator=gen) * 5
    valid = (torch.rand(B, H, W, generator=gen) > 0.2).float()
    preds = [gt + torch.randn(B, 2, H, W, generator=gen) * (3.0 / (k + 1)) for k in range(n)]
    if H >= 8:
        gt[0, :, 2:4] = 500.0  # rows of |gt| > max_flow
        valid[-1, 4:6] = 0.25  # rows of fractional validity
        valid[-1, 6:8] = 0.75
    if B * H * W < LOSS_CLASS_PIXELS:
        valid[:] = 1.0
    mag = gt.double().pow(2).sum(1).sqrt()
    gt[:, 0][(mag - max_flow).abs() < 1e-3] = 0.0
    epe = (preds[-1].double() - gt.double()).pow(2).sum(1).sqrt()
    near = torch.zeros_like(epe, dtype=torch.bool)
    for t in EPE_STEPS:
        near |= (epe - t).abs() < 1e-3
    preds[-1] = torch.where(near[:, None], gt, preds[-1])
    for base in class_bases(B, H, W):
        _class_block(gt, valid, preds, base, max_flow)
    return [p.contiguous() for p in preds], gt.contiguous(), valid.contiguous(), gamma, max_flow


@functools.lru_cache(maxsize=None)
def loss_expected(name, upstream=1.0):
    preds, gt, valid, gamma, max_flow = loss_case(name)
    return seq_loss_oracle(preds, gt, valid, gamma, max_flow, upstream)


def loss_classes(preds, gt, valid, max_flow):
    """Which of the classes a field has to contain are present, read off the data itself."""
    mag = gt.double().pow(2).sum(1).sqrt()
    d = preds[-1].double() - gt.double()
    epe = d.pow(2).sum(1).sqrt()
    ok = (valid >= 0.5) & (mag < f32(max_flow))
    zu, zv = d[:, 0] == 0, d[:, 1] == 0
    out = {
        "valid<0.5": (valid < 0.5).any(),
        "valid==0.5": (valid == 0.5).any(),
        "|gt|==max_flow": ((mag == f32(max_flow)) & (valid >= 0.5)).any(),
        "|gt|>max_flow": ((mag > f32(max_flow)) & (valid >= 0.5)).any(),
        "pred==gt in u only": (ok & zu & ~zv).any(),
        "pred==gt in v only": (ok & ~zu & zv).any(),
        "pred==gt in both": (ok & zu & zv).any(),
    }
    for t in EPE_STEPS:
        out[f"epe=={t:g}"] = (ok & (epe == t)).any()
    return {k: bool(v) for k, v in out.items()}


def stride_step_case():
    """The 'stride' field with every prediction equal to gt except at one valid pixel of the second
    stride step (flat index >= LOSS_GRID_CAP), where all are gt + (3, 4)."""
    _, gt, valid, gamma, max_flow = loss_case("stride")
    B, _, H, W = gt.shape
    n = LOSS_CASES["stride"][3]
    gt, valid = gt.clone(), valid.clone()
    flat = LOSS_GRID_CAP + 12345
    b, s = divmod(flat, H * W)
    assert b >= 1 and flat < B * H * W
    gt.view(B, 2, -1)[b, :, s] = torch.tensor([1.5, -2.25])
    valid.view(B, -1)[b, s] = 1.0
    preds = [gt.clone() for _ in range(n)]
    for p in preds:
        p.view(B, 2, -1)[b, :, s] += torch.tensor([3.0, 4.0])
    return preds, gt, valid, gamma, max_flow, (b, s)


# ------------------------------------------------------------------------------ instance norm
def instance_norm_oracle(x, relu=False, eps=1e-5, dy=None):
    """float64 InstanceNorm (affine=False, biased variance) of ``x`` (N, C, H, W) as stored, with
    optional ReLU; ``dx`` for the upstream ``dy`` as stored, ReLU' taken from ``xhat > 0``.
    The mean is taken about the first pixel, so that a constant channel has xhat = 0 exactly and
    not rounding noise of either sign.  Returns (y, dx or None, mean, rstd)."""
    x64 = x.double()
    x0 = x64[:, :, :1, :1]
    mean = x0 + (x64 - x0).mean((2, 3), keepdim=True)
    var = (x64 - mean).pow(2).mean((2, 3), keepdim=True)
    rstd = (var + eps).rsqrt()
    xhat = (x64 - mean) * rstd
    y = xhat.clamp_min(0) if relu else xhat
    dx = None
    if dy is not None:
        d = dy.double()
        if relu:
            d = d * (xhat > 0)
        dx = rstd * (d - d.mean((2, 3), keepdim=True) - xhat * (d * xhat).mean((2, 3), keepdim=True))
    return y, dx, mean[:, :, 0, 0], rstd[:, :, 0, 0]


NORM_SHAPES = [(2, 8, 32, 32), (2, 8, 25, 41), (3, 24, 5, 7), (1, 512, 3, 1), (1, 8, 3, 5), (2, 64, 1, 1),
               (2, 96, 37, 29)]
NORM_OFFSET_SHAPE = (2, 64, 37, 29)
NORM_OFFSETS = ("mean8", "mean32", "mean100", "const", "ints_bf16")
NORM_TOL = {torch.float32: dict(rtol=1e-4, atol=1e-4), torch.bfloat16: dict(rtol=2e-2, atol=3e-2)}


KINK = 1e-4  # no xhat other than an exact 0 is closer to the ReLU kink than this


def norm_xhat(x):
    _, _, mean, rstd = instance_norm_oracle(x)
    return (x.double() - mean[:, :, None, None]) * rstd[:, :, None, None]


def _off_kink(x, dtype):
    """``x`` in ``dtype`` with the few values whose xhat is within KINK of 0 moved up by 0.05 std:
    ReLU' jumps at xhat = 0, where the rounding of any fp32 implementation decides the side."""
    for _ in range(8):
        xs = x.to(dtype)
        xhat = norm_xhat(xs)
        bad = (xhat.abs() < KINK) & (xhat != 0)
        if not bad.any():
            return xs
        std = xs.double().std((2, 3), unbiased=False, keepdim=True)
        x = torch.where(bad, (xs.double() + 0.05 * std).float(), xs.float())
    raise AssertionError("values stay at the ReLU kink")


def _norm_seed(shape):
    return int(np.dot(shape, (1, 10, 100, 1000)))


@functools.lru_cache(maxsize=None)
def norm_case(shape, dtype):
    """(x, dy) in ``dtype``, NCHW on the host, with a different mean and std per image and channel."""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(_norm_seed(shape))
    std = 0.5 + 3.5 * torch.rand(N, C, 1, 1, generator=gen)
    mean = 6 * torch.rand(N, C, 1, 1, generator=gen) - 3
    x = torch.randn(N, C, H, W, generator=gen) * std + mean
    dy = torch.randn(N, C, H, W, generator=gen)
    return _off_kink(x, dtype), dy.to(dtype)


@functools.lru_cache(maxsize=None)
def norm_offset_case(kind):
    """(x, dy) at NORM_OFFSET_SHAPE: a per-channel mean of 8, 32 or 100 standard deviations (fp32),
    a channel constant at 3.3 (fp32), or integers in 96...104, which bf16 holds exactly."""
    N, C, H, W = NORM_OFFSET_SHAPE
    gen = torch.Generator().manual_seed(NORM_OFFSETS.index(kind) + 77)
    dy = torch.randn(N, C, H, W, generator=gen)
    if kind == "ints_bf16":
        x = torch.randint(96, 105, (N, C, H, W), generator=gen).float()
        whole = x.sum((2, 3)) % (H * W) == 0  # an integer mean would put its pixels on the ReLU kink
        x[:, :, 0, 0] = torch.where(whole, 200.0 - x[:, :, 0, 0] + (x[:, :, 0, 0] == 100), x[:, :, 0, 0])
        xs = x.bfloat16()
        assert torch.equal(_off_kink(xs, torch.bfloat16), xs)
        return xs, dy.bfloat16()
    std = 0.25 * 2 ** (4 * torch.rand(1, C, 1, 1, generator=gen))  # 0.25 ... 4
    x = torch.randn(N, C, H, W, generator=gen) * std
    if kind == "const":
        x = x + 0.5
        x[:, 5] = 3.3
    else:
        sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).view(1, C, 1, 1)
        x = x + float(kind[4:]) * std * sign
    return _off_kink(x, torch.float32), dy


# ------------------------------------------------------------------------------ update-block helpers
def bf16r(t):
    return t.bfloat16().double()


def gru_bwd_a_oracle(dH, z, q, h):
    """Closed forms of update_aux.hip for h' = (1 - z) h + z q, with respect to the pre-activations
    of z = sigmoid(a) and q = tanh(c), in float64 on the values as stored.  Returns
    (dq_pre, dz_pre, carry) and the sum of |terms| of carry = g - g z."""
    g, z, q, h = dH.double(), z.double(), q.double(), h.double()
    dq = g * z * (1 - q * q)
    dz = g * (q - h) * z * (1 - z)
    carry = g * (1 - z)
    return dq, dz, carry, g.abs() + (g * z).abs()


def gru_bwd_b_oracle(drh, r, h, carry):
    """rh = r h with r = sigmoid(b): (dr_pre, dh = carry + d(rh) r) and |carry| + |d(rh) r|."""
    g, r, h, c = drh.double(), r.double(), h.double(), carry.double()
    return g * h * r * (1 - r), c + g * r, c.abs() + (g * r).abs()


@functools.lru_cache(maxsize=None)
def gru_case(P, C, seed=0):
    """dH, drh, carry fp32 and z, r, q, h bf16 of (P, C), with z, r in {0, 1} exactly and q = +-1
    at six of every 35 entries (the first six of a single row)."""
    gen = torch.Generator().manual_seed(1000 * seed + P + C)
    rnd = lambda: torch.randn(P, C, generator=gen)  # noqa: E731
    dH, drh, carry = rnd(), rnd(), rnd()
    z, r = torch.sigmoid(2 * rnd()), torch.sigmoid(2 * rnd())
    q, h = torch.tanh(rnd()), torch.tanh(rnd())
    slot = torch.arange(P * C).view(P, C) % 35
    for t, j, v in ((z, 0, 0.0), (z, 1, 1.0), (r, 2, 1.0), (r, 3, 0.0), (q, 4, 1.0), (q, 5, -1.0)):
        t[slot == j] = v
    return dict(dH=dH, drh=drh, carry=carry, z=z.bfloat16(), r=r.bfloat16(), q=q.bfloat16(), h=h.bfloat16())


def bf16_ordinal(t):
    """bf16 values as integers in value order (+0 and -0 both 0): neighbours differ by one."""
    i = t.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7FFF), i)


def masked_cast_ref(src, mask, C):
    """``where(mask > 0, src, 0).bfloat16()`` with src zero-padded to C columns."""
    P = src.shape[0]
    full = torch.zeros(P, C)
    full[:, :src.shape[1]] = src
    if mask is not None:
        full = torch.where(mask[:, :C] > 0, full, torch.zeros(()))
    return full.bfloat16()


def masked_cast_case(P, C, Cvalid, seed=0):
    """src fp32 (P, Cvalid) and mask bf16 (P, C); the first row entries hold, as far as the row
    reaches: mask +0, -0, the smallest positive bf16 subnormal, a negative, NaN, and src NaN, +Inf
    and -Inf under a positive mask and NaN under a zero one."""
    gen = torch.Generator().manual_seed(seed + P + C)
    src = torch.randn(P, Cvalid, generator=gen)
    mask = torch.relu(torch.randn(P, C, generator=gen)).bfloat16()
    tiny = torch.tensor([1], dtype=torch.int16).view(torch.bfloat16)[0]  # 0x0001
    edge_mask = [0.0, -0.0, tiny, -1.5, float("nan"), 1.0, 2.0, tiny, 0.0]
    edge_src = [1.0, 2.0, 3.0, 4.0, 5.0, float("nan"), float("inf"), float("-inf"), float("nan")]
    for j, (m, s) in enumerate(zip(edge_mask, edge_src)):
        if j < Cvalid:
            mask[:, j] = m
            src[:, j] = s
    return src, mask


SPLIT_CASES = [(8, 0, 8, 2), (88, 80, 2, 2), (328, 0, 328, 324), (16, 12, 8, 6)]  # (G, c0, Cpad, C)


def split_width(G, c0, Cpad):
    last = c0 + Cpad - 1
    return (last // G) * 3 * G + 3 * G  # whole groups up to the one that holds the last channel


def split_pack_ref(src, dst, G, c0, Cpad):
    """hi = bf16(x), lo = bf16(x - hi), the third plane hi again, channel n = c0 + c of a group-G
    split row; channels C <= c < Cpad are zero, the rest of ``dst`` is kept."""
    out = dst.clone()
    P, C = src.shape
    x = torch.zeros(P, Cpad)
    x[:, :C] = src
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    for c in range(Cpad):
        n = c0 + c
        col = (n // G) * 3 * G + n % G
        out[:, col], out[:, col + G], out[:, col + 2 * G] = hi[:, c], lo[:, c], hi[:, c]
    return out


def split_src(P, C, seed=0):
    gen = torch.Generator().manual_seed(seed + P + C)
    x = torch.randn(P, C, generator=gen) * 3
    # zeros, a round-to-even tie of the bf16 cast on either side, a large and a small normal number
    edge = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 3.0e38, 1.0e-30])
    k = min(P * C, edge.numel())
    x.view(-1)[:k] = edge[:k]
    return x


def pixel_grid(B, H, W):
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([x, y])[None].expand(B, 2, H, W)


def flow_case(B, H, W, seed=0):
    """fp32 (B, 2, H, W) coordinates: the pixel grid plus a flow of a few pixels."""
    gen = torch.Generator().manual_seed(seed + B + H + W)
    return (pixel_grid(B, H, W) + torch.randn(B, 2, H, W, generator=gen) * 4).contiguous()


def pack_flow_ref(flow, dtype, from_coords):
    """(P, 2) of ``dtype``: the flow (coords minus the pixel grid with from_coords), pixel-major."""
    B, _, H, W = flow.shape
    f = flow - pixel_grid(B, H, W) if from_coords else flow
    return f.permute(0, 2, 3, 1).reshape(-1, 2).to(dtype)


def apply_delta_ref(coords1, delta2):
    """(coords_out, flow_out) fp32 (B, 2, H, W) from delta2 = delta[:, :2], pixel-major (P, 2)."""
    B, _, H, W = coords1.shape
    out = coords1 + delta2.reshape(B, H, W, 2).permute(0, 3, 1, 2)
    return out, out - pixel_grid(B, H, W)
