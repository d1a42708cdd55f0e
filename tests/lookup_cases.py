"""Seeded host inputs, float64 oracles, layout helpers and derived error bounds for the correlation
lookup kernels (csrc/corr_volume.hip: lookup_fwd_kernel, lookup_bwd_kernel, lookup_grad_rows_kernel,
pyramid_unpool_kernel) and the on-the-fly local correlation (csrc/local_corr.hip,
csrc/local_corr_mfma.hip).  Shared by test_lookup_cpu.py / _gpu.py; nothing here touches the native
extension.

The oracles compute in float64 on the values as stored (an fp32 or bf16 tensor upcast exactly) with
index arithmetic, no ``grid_sample``: no normalise / un-normalise rounding, zeros (not NaN) for a
non-finite query, and no division by ``size - 1``.
"""
import functools
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24  # unit roundoffs: round-to-nearest relative error of one operation / one store
U_BF16 = 2.0 ** -8
U_F16 = 2.0 ** -11
U_OUT = {torch.float32: 0.0, torch.bfloat16: U_BF16, torch.float16: U_F16}

# (Hl, Wl) per level: repeated 2x2 floor pooling of a 17x21 and of an 18x33 base.  Between them: a
# level of exactly one 16-column block (9x16), partial blocks (21, 10, 5, 2, 8, 4 columns), three
# blocks (33), windows that straddle x = 15 | 16 and 31 | 32, and the 2x2 last level of the
# smallest legal input (128 px).  No level of height or width 1: the model cannot reach one.
LEVEL_SETS = {
    "17x21": [(17, 21), (8, 10), (4, 5), (2, 2)],
    "18x33": [(18, 33), (9, 16), (4, 8), (2, 4)],
}
RANDOM_BLOCK = (2, 5, 7)  # (B, H, W) of the second query block: grid + 6 * randn


def pad16(n: int) -> int:
    return -(-n // 16) * 16


# ------------------------------------------------------------------------------ oracles
def lookup_oracle(levels, coords, r):
    """float64 radius-``r`` bilinear lookup.  ``levels``: list of (P, Hl, Wl) float64 images (one per
    query, P = B*H*W); ``coords`` (B, 2, H, W) fp32.  Returns (B, H, W, L*(2r+1)^2) float64.

    Level l: ``c = float64(coords) * 2^-l`` (exact in fp32 too).  Tap (ix, iy), channel
    ``ix * (2r+1) + iy``, sits at ``c + (ix - r, iy - r)``; floor and fraction in float64; the four
    neighbours weighted (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy; a neighbour outside
    [0, Wl) x [0, Hl) contributes 0.  A query with a non-finite component gives zeros."""
    B, _, H, W = coords.shape
    P = B * H * W
    c = coords.permute(0, 2, 3, 1).reshape(P, 2).double()
    finite = torch.isfinite(c).all(1)
    c = torch.where(finite[:, None], c, torch.zeros((), dtype=torch.float64))
    d = torch.arange(-r, r + 1, dtype=torch.float64)
    rd = 2 * r + 1
    outs = []
    for l, img in enumerate(levels):
        assert img.dtype == torch.float64 and img.shape[0] == P
        Hl, Wl = img.shape[1:]
        flat = img.reshape(P, Hl * Wl)
        t = c * 2.0 ** -l
        tx, ty = t[:, 0:1] + d, t[:, 1:2] + d  # (P, rd)
        x0f, y0f = torch.floor(tx), torch.floor(ty)
        fx, fy = tx - x0f, ty - y0f
        # |x0| may be 3e38: anything at or beyond -2 / size + 1 has both neighbours out of range
        x0 = x0f.clamp(-2, Wl + 1).long()
        y0 = y0f.clamp(-2, Hl + 1).long()

        def corner(dx, dy, wx, wy):
            xi, yi = x0 + dx, y0 + dy
            ok = ((xi >= 0) & (xi < Wl))[:, :, None] & ((yi >= 0) & (yi < Hl))[:, None, :]
            idx = yi.clamp(0, Hl - 1)[:, None, :] * Wl + xi.clamp(0, Wl - 1)[:, :, None]  # [p, ix, iy]
            v = flat.gather(1, idx.reshape(P, rd * rd)).reshape(P, rd, rd)
            w = wx[:, :, None] * wy[:, None, :]
            return torch.where(ok, w * v, torch.zeros((), dtype=torch.float64))

        o = (corner(0, 0, 1 - fx, 1 - fy) + corner(1, 0, fx, 1 - fy) + corner(0, 1, 1 - fx, fy)
             + corner(1, 1, fx, fy))
        o = torch.where(finite[:, None, None], o, torch.zeros((), dtype=torch.float64))
        outs.append(o.reshape(P, rd * rd))
    return torch.cat(outs, 1).reshape(B, H, W, len(levels) * rd * rd)


def lookup_grad_oracle(coords_list, grads_list, level_shapes, r, absolute=False):
    """The float64 adjoint of ``lookup_oracle``: level-gradient images (P, Hl, Wl) summed over the T
    lookups at ``coords_list[t]`` with window gradients ``grads_list[t]`` (B, H, W, >= L*(2r+1)^2)
    as stored; channels beyond L*(2r+1)^2 are ignored.  Taken by autograd through the oracle.
    ``absolute``: of |grads| instead; the weights are non-negative, so it is 0 exactly where no
    lookup reaches a pixel with a non-zero weight, and not where float64 terms happen to cancel."""
    B, _, H, W = coords_list[0].shape
    P, n = B * H * W, len(level_shapes) * (2 * r + 1) ** 2
    levels = [torch.zeros(P, Hl, Wl, dtype=torch.float64, requires_grad=True) for Hl, Wl in level_shapes]
    loss = 0.0
    for c, g in zip(coords_list, grads_list):
        gd = g[..., :n].double()
        loss = loss + (lookup_oracle(levels, c, r) * (gd.abs() if absolute else gd)).sum()
    return list(torch.autograd.grad(loss, levels))


def pool_levels(f, L):
    """(B, C, H, W) float64 and its repeated 2x2 floor average pools, L in total."""
    out = [f]
    for _ in range(L - 1):
        out.append(F.avg_pool2d(out[-1], 2, stride=2))
    return out


def local_lookup_oracle(f1, f2, coords, L, r):
    """The lookup of the volume that is never stored: ``f1 . pool_l(f2)^T / sqrt(C)`` in float64
    from the features as stored ((B, C, H, W) fp32, or rounded to bf16 and upcast), through
    ``lookup_oracle``.  Differentiable in f1 and f2.  Also returns the magnitude S (P, L):
    ``S[q, l] = max_pix sum_c |f1[q, c]| * pool_l(|f2|)[pix, c] / sqrt(C)``, which bounds every
    partial sum of every correlation of query q at level l."""
    levels, S = local_levels(f1, f2, L)
    return lookup_oracle(levels, coords, r), S


def local_levels(f1, f2, L):
    """The float64 volume levels (B*H*W, Hl, Wl) of ``local_lookup_oracle`` and its S (P, L)."""
    B, C, H, W = f1.shape
    a = f1.double().reshape(B, C, H * W).transpose(1, 2)  # (B, HW, C)
    levels, S = [], []
    f2d = f2.double()
    for p, pa in zip(pool_levels(f2d, L), pool_levels(f2d.detach().abs(), L)):
        Hl, Wl = p.shape[2:]
        levels.append((torch.matmul(a, p.reshape(B, C, Hl * Wl)) / math.sqrt(C)).reshape(B * H * W, Hl, Wl))
        S.append((torch.matmul(a.detach().abs(), pa.reshape(B, C, Hl * Wl)) / math.sqrt(C)).amax(2).reshape(-1))
    return levels, torch.stack(S, 1)


def level_max(levels):
    """m (P, L): the largest |value| of each query's level image."""
    return torch.stack([lv.abs().amax((1, 2)) for lv in levels], 1)


def per_channel(v, win):
    """(P, L) per query and level -> (P, L * win) per output channel."""
    return v.repeat_interleave(win, dim=1)


# ------------------------------------------------------------------------------ error bounds
def fwd_bound(oracle, m, r, out_dtype):
    """|out - oracle| <= 16 * u32 * m[q, l] + u_out * |oracle|, ``oracle`` (P, L*win), ``m`` (P, L).

    The kernel blends ``(1-fy) * ((1-fx) * a + fx * b) + fy * ((1-fx) * c + fx * d)`` in fp32 from
    exact inputs (the volume as stored; ``coords * 2^-l`` is exact).  Roundings that touch a term
    of magnitude <= m: the fraction ``c - floor(c)`` (exact except for a negative c close to 0: 1),
    ``1 - f`` (1), so a weight carries at most 2; a product weight * value adds 1 (3 on the term),
    the inner add 1, the outer product with a weight of <= 2 roundings 3, the outer add 1: at most
    3 + 1 + 3 + 1 = 8 per neighbour pair; the two pairs have weights (1-fy) and fy that sum to 1,
    so their 8s do not add, but the bound takes them as if they did: 16 roundings of u32 against
    m.  The store then rounds once to the output format: u_out * |value|, u_out = 0 / 2^-8 / 2^-11
    for fp32 / bf16 / fp16 (a subnormal fp16 result is off by <= 2^-25, below 16 * u32 * m for any
    m >= 2^-5)."""
    win = (2 * r + 1) ** 2
    return 16 * U32 * per_channel(m, win) + U_OUT[out_dtype] * oracle.abs()


def split_bound(oracle, m, r):
    """Split rows [hi | lo | hi]: hi = bf16(v), lo = bf16(v - hi).  |v - hi| <= 2^-8 |v| is exact in
    fp32, and rounding it to bf16 leaves <= 2^-8 * 2^-8 |v| = 2^-16 |v|:
    |hi + lo - oracle| <= 16 * u32 * m + 2^-16 * |oracle|."""
    win = (2 * r + 1) ** 2
    return 16 * U32 * per_channel(m, win) + 2.0 ** -16 * oracle.abs()


def grad_bound(oracle, T, gmax, bf16_rows=False, partial=None):
    """|row - oracle| <= 32 * T * u32 * gmax (+ u_bf16 * |oracle| for bf16 rows); ``gmax`` the largest
    |window gradient| as stored.

    One lookup adds to a level pixel up to four terms weight * g whose weights sum to <= 1, so the
    addend is <= gmax; a weight product (1-fx)(1-fy) carries <= 5 roundings, the product with g one
    more, the three adds three: <= 9 * u32 * gmax per lookup.  The running sum after t lookups is
    <= t * gmax and each add rounds it once: sum_t t <= T (T + 1) / 2.  Together
    (9 T + T (T + 1) / 2) u32 gmax <= 32 T u32 gmax for T <= 45.  bf16 rows are rounded once on the
    store: u_bf16 * |row|.  ``partial``: bf16 rows written in two launches are rounded after the
    first one as well, whose float64 value it is: + u_bf16 * |partial|."""
    assert T <= 45
    b = torch.full_like(oracle, 32 * T * U32 * gmax)
    if bf16_rows:
        b = b + U_BF16 * oracle.abs()
        if partial is not None:
            b = b + U_BF16 * partial.abs()
    return b


def local_bound(oracle, S, r, C, path, out_dtype=torch.float32):
    """Local correlation, per output channel; ``S`` (P, L) from ``local_lookup_oracle``, l the level.

    scalar (fp32 kernel): a C-term fp32 dot product of fp32 products, C product and C add roundings
    against partial sums <= S: 2C; the blend as in ``fwd_bound``: 16; the level's features were
    pooled l times in fp32, 4 roundings each (three adds, one scale): 4l.
    ``(2C + 16 + 4l) * u32 * S``.
    mfma (bf16 operands): bf16 x bf16 products are exact in fp32, the C adds remain: C; the pooled
    level is rounded to bf16 once: u_bf16 * S; the store u_out * |oracle|.
    ``(C + 16 + 4l) * u32 * S + u_bf16 * S + u_out * |oracle|``.
    split (three bf16 MFMA passes hi.hi + lo.hi + hi.lo): 3C adds; each operand is represented to
    2^-16 and the dropped lo.lo term is 2^-16: ``(3C + 16 + 4l) * u32 * S + 4 * 2^-16 * S``."""
    win = (2 * r + 1) ** 2
    lvl = torch.arange(S.shape[1], dtype=torch.float64)
    k = {"scalar": 2, "mfma": 1, "split": 3}[path]
    b = (k * C + 16 + 4 * lvl) * U32 * S
    if path == "mfma":
        b = b + U_BF16 * S
    elif path == "split":
        b = b + 4 * 2.0 ** -16 * S
    b = per_channel(b, win)
    if path == "mfma":
        b = b + U_OUT[out_dtype] * oracle.abs()
    return b


def e2e_fwd_bound(m, S, r, C):
    """Dense split pyramid end to end: the volume is a three-pass split GEMM of fp32 operands,
    (3C + 16) * u32 * S against the float64 volume, and the lookup of it adds 16 * u32 * m."""
    win = (2 * r + 1) ** 2
    return per_channel(16 * U32 * m + (3 * C + 16) * U32 * S, win)


# ------------------------------------------------------------------------------ layouts
def level_sizes(shapes):
    """[(Hl, Wl, off)] and the row length ld of 16-column-blocked levels, as _BuildPyramid lays
    them out."""
    sizes, off = [], 0
    for Hl, Wl in shapes:
        sizes.append((Hl, Wl, off))
        off += pad16(Wl) * Hl
    return sizes, off


def segments(sizes):
    return [v for Hl, Wl, off in sizes for v in (off, Hl, Wl)]


def blocked_views(buf, sizes):
    """(P, Wpad/16, Hl, 16) views into ``buf`` (P, pitch): the strides of _PyramidState.views with
    the buffer's own row pitch."""
    return [buf.as_strided((buf.shape[0], pad16(Wl) // 16, Hl, 16), (buf.stride(0), Hl * 16, 16, 1),
                           buf.storage_offset() + off) for Hl, Wl, off in sizes]


def to_blocked(levels, dtype, pitch_pad=0, pad_value=0.0):
    """One (P, ld + pitch_pad) buffer of ``dtype``: level pixel (y, x) at
    ``off_l + ((x // 16) * Hl + y) * 16 + x % 16``, padding columns ``pad_value`` (zero: the volume's
    contract), the pitch tail of each row NaN.  Returns (buf, sizes, ld)."""
    sizes, ld = level_sizes([lv.shape[1:] for lv in levels])
    P = levels[0].shape[0]
    buf = torch.full((P, ld + pitch_pad), float("nan"), dtype=dtype)
    for lv, view, (Hl, Wl, off) in zip(levels, blocked_views(buf, sizes), sizes):
        img = torch.full((P, Hl, pad16(Wl)), pad_value, dtype=dtype)
        img[:, :, :Wl] = lv.to(dtype)
        view.copy_(img.reshape(P, Hl, -1, 16).permute(0, 2, 1, 3))
    return buf, sizes, ld


def from_blocked(rows, sizes, padding=False):
    """The inverse: (P, Hl, Wl) images of ``rows`` (P, >= ld); ``padding``: the (P, Hl, Wpad - Wl)
    padding columns instead."""
    out = []
    for view, (Hl, Wl, off) in zip(blocked_views(rows, sizes), sizes):
        img = view.permute(0, 2, 1, 3).reshape(rows.shape[0], Hl, pad16(Wl))
        out.append(img[:, :, Wl:] if padding else img[:, :, :Wl])
    return out


def to_rowmajor(levels, dtype, pitch_pad=8):
    """The row-major twin: per level a (P, Hl*Wl + pitch_pad) buffer, NaN in the gap, and its
    (P, Hl, Wl) view of row pitch > Hl*Wl.  Returns (buffers, views)."""
    bufs, views = [], []
    for lv in levels:
        P, Hl, Wl = lv.shape
        buf = torch.full((P, Hl * Wl + pitch_pad), float("nan"), dtype=dtype)
        view = buf.as_strided((P, Hl, Wl), (buf.stride(0), Wl, 1))
        view.copy_(lv.to(dtype))
        bufs.append(buf)
        views.append(view)
    return bufs, views


def rowmajor_views(bufs, shapes):
    return [b.as_strided((b.shape[0], Hl, Wl), (b.stride(0), Wl, 1), b.storage_offset()) for b, (Hl, Wl) in
            zip(bufs, shapes)]


# ------------------------------------------------------------------------------ coordinates
def axis_values(n, r, npad=None):
    """The coordinate classes of one axis of level-0 size ``n``; ``npad``: the padded width of a
    blocked level (x axis only)."""
    e = 2.0 ** -10
    v = [-1e4, -40, -(r + 1), -(r + 1) + e, -r - e, -5.001, -1, -0.5, -1e-7, 0, 0.125, 0.5, 7, 7.875, 8, 15, 15.5, 16,
         n - 1, n - 1 + e, n - 0.5, n, n + r - e, n + r]
    if npad is not None:
        v += [npad - 0.5, npad]
    v += [40, 1e4, 999999.5, 1e6, 1e6 + 1, 2.0 ** 31, -2.0 ** 31, 3e38, -3e38]
    out = []
    for x in torch.tensor(v, dtype=torch.float32).tolist():  # as fp32 stores them, without repeats
        if x not in out:
            out.append(x)
    return out


NONFINITE = [(a, b) for v in (float("inf"), float("-inf"), float("nan")) for a, b in ((v, 3.25), (3.25, v), (v, v))]


@functools.lru_cache(maxsize=None)
def edge_coords(H0, W0, r):
    """(1, 2, 1, n) fp32: the Cartesian product of the x and y class lists, then the nine queries
    with +inf, -inf and NaN in x only, in y only and in both."""
    xs, ys = axis_values(W0, r, pad16(W0)), axis_values(H0, r)
    q = [(x, y) for x in xs for y in ys] + NONFINITE
    return torch.tensor(q, dtype=torch.float32).t().reshape(1, 2, 1, len(q)).contiguous()


def n_finite(H0, W0, r):
    return edge_coords(H0, W0, r).shape[3] - len(NONFINITE)


@functools.lru_cache(maxsize=None)
def random_coords(seed=0):
    B, H, W = RANDOM_BLOCK
    gen = torch.Generator().manual_seed(4242 + seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return (torch.stack([x, y])[None] + 6 * torch.randn(B, 2, H, W, generator=gen)).contiguous()


def window_classes(coords, shapes, r):
    """Per level, boolean masks over the finite queries of ``coords``: the level-l fraction is
    exactly 0 in x / in y, and the (2r+2)^2 neighbourhood [floor(c) - r, floor(c) + r + 1]^2 lies
    fully inside the level, fully outside it (so the result is all zeros) or partly outside, and
    whether the centre tap's four neighbours are all in range."""
    c = coords.permute(0, 2, 3, 1).reshape(-1, 2).double()
    c = c[torch.isfinite(c).all(1)]
    out = []
    for l, (Hl, Wl) in enumerate(shapes):
        t = c * 2.0 ** -l
        f = torch.floor(t)
        lo, hi = f - r, f + r + 1
        size = torch.tensor([Wl, Hl], dtype=torch.float64)
        inside = ((lo >= 0) & (hi <= size - 1)).all(1)
        outside = ((hi < 0) | (lo > size - 1)).any(1)
        centre = ((f >= 0) & (f + 1 <= size - 1)).all(1)
        out.append({"fx==0": t[:, 0] == f[:, 0], "fy==0": t[:, 1] == f[:, 1], "inside": inside, "outside": outside,
                    "partly": ~inside & ~outside, "centre": centre})
    return out


# ------------------------------------------------------------------------------ seeded values
@functools.lru_cache(maxsize=None)
def level_values(P, shapes, dtype, seed=0):
    """Level images (P, Hl, Wl) float64 of values as ``dtype`` stores them: randn scaled per query
    by 0.25 ... 4, so that an index that lands in a neighbour's row shows."""
    gen = torch.Generator().manual_seed(100 + seed + P)
    scale = 0.25 * 2 ** (4 * torch.rand(P, 1, 1, generator=gen))
    return tuple((torch.randn(P, Hl, Wl, generator=gen) * scale).to(dtype).double() for Hl, Wl in shapes)


def window_grads(shape, channels, n_valid, dtype, seed):
    """(B, H, W, channels) window gradient of ``dtype``; channels from ``n_valid`` on are NaN."""
    gen = torch.Generator().manual_seed(900 + seed)
    g = torch.randn(*shape, channels, generator=gen)
    g[..., n_valid:] = float("nan")
    return g.to(dtype)


def features(B, C, H, W, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(7000 + seed)
    return torch.randn(B, C, H, W, generator=gen).to(dtype), torch.randn(B, C, H, W, generator=gen).to(dtype)


def embed_fields(T, B, H, W, block, seed, sigma=3.0):
    """T fields (B, 2, H, W) fp32 of grid + sigma * randn whose first pixels (field-major, then
    image-major, then row-major) hold the queries of ``block`` (1, 2, 1, n), n <= T*B*H*W."""
    n = block.shape[3]
    assert n <= T * B * H * W
    gen = torch.Generator().manual_seed(300 + seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.stack([x, y]).expand(T, B, 2, H, W) + sigma * torch.randn(T, B, 2, H, W, generator=gen)
    f = f.permute(2, 0, 1, 3, 4).reshape(2, -1).clone()
    f[:, :n] = block[0, :, 0]
    f = f.reshape(2, T, B, H, W).permute(1, 2, 0, 3, 4)
    return [f[t].contiguous() for t in range(T)]


def ratio(err, bound):
    """max(|err| / bound) with 0 / 0 = 0."""
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
