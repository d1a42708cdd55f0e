"""The correlation lookup kernels, their backward and the local correlation against the float64
oracles of lookup_cases.py, elementwise within the derived bounds, at the layouts and dtypes the
model runs (16-column-blocked levels, bf16 volume, 16-bit outputs) and on the edge block of
coordinate classes.

Conventions: outputs start as NaN, so an element a kernel does not write fails; inputs carry NaN in
every pitch tail, so a read past a row fails; where the oracle is exactly 0 (a window fully out of
range, a non-finite query) the result must be ``== 0``; everything else is held elementwise to its
bound.  Every test prints ``max(|err| / bound)`` of its group."""
import functools

import pytest
import torch
import torch.nn.functional as F

import lookup_cases as K

pytestmark = pytest.mark.gpu

SETS = list(K.LEVEL_SETS)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def _ops():
    from raft_ros_amd.ops._ext import ops

    return ops()


def _hold(tag, got, oracle, bound, zero=None):
    """``got`` against ``oracle`` (same shape): no NaN, exact zeros where the oracle is 0 (or where
    ``zero`` says that nothing reaches the element), the bound everywhere else.  Returns and prints
    the largest |err| / bound."""
    got, oracle = got.detach().cpu().double().reshape(oracle.shape), oracle.detach()
    assert not torch.isnan(got).any(), f"{tag}: {int(torch.isnan(got).sum())} elements NaN (unwritten or read past a row)"
    zero = oracle == 0 if zero is None else zero
    assert (oracle[zero] == 0).all()
    assert (got[zero] == 0).all(), f"{tag}: {int((got[zero] != 0).sum())} non-zeros where the oracle is exactly 0"
    err = (got - oracle).abs()
    worst = K.ratio(err, bound)
    print(f"{tag}: max |err| / bound = {worst:.3f}")
    bad = err > bound
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements over the bound, worst ratio {worst:.3f}"
    return worst


def _blocks(name, r):
    """The two query blocks: the edge block (1, 2, 1, n) and grid + 6 randn (2, 2, 5, 7)."""
    H0, W0 = K.LEVEL_SETS[name][0]
    return {"edge": K.edge_coords(H0, W0, r), "rand": K.random_coords()}


def _npix(coords):
    return coords.shape[0] * coords.shape[2] * coords.shape[3]


def _device_levels(levels, layout, vdtype, cuda):
    """Level views on the device in ``layout`` with NaN pitch tails; keeps the buffers alive."""
    if layout == "blocked":
        buf, sizes, _ = K.to_blocked(levels, vdtype, pitch_pad=24)
        buf = buf.to(cuda)
        return K.blocked_views(buf, sizes), buf
    bufs, _ = K.to_rowmajor(levels, vdtype, pitch_pad=8)
    bufs = [b.to(cuda) for b in bufs]
    return K.rowmajor_views(bufs, [lv.shape[1:] for lv in levels]), bufs


@functools.lru_cache(maxsize=None)
def _fwd_oracle(name, block, r, L, vdtype):
    coords = _blocks(name, r)[block]
    levels = list(K.level_values(_npix(coords), tuple(K.LEVEL_SETS[name]), vdtype)[:L])
    want = K.lookup_oracle(levels, coords, r).reshape(_npix(coords), -1)
    return levels, want, K.level_max(levels)


# (r, L): the generic kernel (RC = 0) at r = 1, 3 and 6, the r = 4 all-levels kernel with one, three
# and four levels
RADIUS_LEVELS = [(1, 4), (6, 2), (3, 3), (4, 1), (4, 3), (4, 4)]


@pytest.mark.parametrize("r,L", RADIUS_LEVELS)
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("vdtype", [F32, BF16], ids=["vol32", "vol16"])
@pytest.mark.parametrize("layout", ["rowmajor", "blocked"])
def test_corr_lookup(cuda, layout, vdtype, name, r, L):
    """corr_lookup in fp32, bf16 and fp16, with out_channels = L*win and L*win + 4 (exact zeros in
    the tail).  The RAFT_LOOKUP_ALL=0 variant (r = 4 one level ahead) is read once per process: an
    A/B switch, left out."""
    win = (2 * r + 1) ** 2
    for block, coords in _blocks(name, r).items():
        levels, want, m = _fwd_oracle(name, block, r, L, vdtype)
        views, keep = _device_levels(levels, layout, vdtype, cuda)
        c = coords.to(cuda)
        for odt in (F32, BF16, F16):
            bound = K.fwd_bound(want, m, r, odt)
            for extra in (0, 4):
                out = _ops().corr_lookup(views, c, r, odt, L * win + extra if extra else 0)
                assert out.shape == (*coords.shape[:1], *coords.shape[2:], L * win + extra) and out.dtype == odt
                out = out.reshape(-1, L * win + extra)
                assert (out[:, L * win:] == 0).all()
                _hold(f"corr_lookup {layout} {name} r{r} L{L} {block} {vdtype}->{odt} +{extra}", out[:, :L * win], want, bound)
        del keep


def _flow_want(coords, dtype):
    B, _, H, W = coords.shape
    y, x = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    return (coords - torch.stack([x, y])[None]).permute(0, 2, 3, 1).reshape(-1, 2).to(dtype)


def _same(a, b):
    """Equal as values, NaN where and only where the other is NaN (payloads are free)."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("r", [4, 3])
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("odt", [BF16, F16], ids=["bf16", "fp16"])
def test_corr_lookup_into(cuda, odt, name, r):
    """corr_lookup_into on the edge block, blocked: features bit-identical to corr_lookup of the same
    dtype, the tail zero, flow8 / motion = coords - grid rounded once to the 16-bit dtype with zeros
    in lanes 2 to 7 (NaN exactly where coords - grid is NaN; +-3e38 is inf in fp16)."""
    L, win = 4, (2 * r + 1) ** 2
    coords = _blocks(name, r)["edge"]
    levels, want, m = _fwd_oracle(name, "edge", r, L, BF16)
    views, keep = _device_levels(levels, "blocked", BF16, cuda)
    c = coords.to(cuda)
    P, och = _npix(coords), L * win + 4
    out = torch.full((1, 1, P, och), float("nan"), device=cuda, dtype=odt)
    flow8 = torch.full((P, 8), float("nan"), device=cuda, dtype=odt)
    motion = torch.full((P, 16), 5.0, device=cuda, dtype=odt)
    _ops().corr_lookup_into(views, c, r, out, flow8, motion[:, 6:])
    ref_out = _ops().corr_lookup(views, c, r, odt, och)
    assert torch.equal(out.view(torch.int16), ref_out.view(torch.int16))
    _hold(f"corr_lookup_into {name} r{r} {odt}", out.reshape(P, och)[:, :L * win], want, K.fwd_bound(want, m, r, odt))
    assert (out.reshape(P, och)[:, L * win:] == 0).all()
    fw = _flow_want(coords, odt)
    assert _same(flow8[:, :2], fw) and (flow8[:, 2:] == 0).all()
    assert _same(motion[:, 6:8], fw) and (motion[:, :6] == 5).all() and (motion[:, 8:] == 5).all()
    # without the flow outputs: the same features
    out2 = torch.full_like(out, float("nan"))
    _ops().corr_lookup_into(views, c, r, out2, None, None)
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16))
    del keep


@pytest.mark.parametrize("r,L", [(4, 4), (3, 4), (4, 2), (6, 2)])
@pytest.mark.parametrize("name", SETS)
def test_corr_lookup_split_into(cuda, name, r, L):
    """corr_lookup_split_into (fp32 blocked volume -> split-bf16 rows [hi | lo | hi] of G channels):
    plane 2 is plane 0 bit for bit, hi + lo is within the split bound, channels beyond L*win are
    zero in all planes; flow8 (P, 24) and motion hold coords - grid as hi / lo / hi planes, hi the
    bf16 rounding and lo the bf16 rounding of the rest.  r = 4 is RC = 4 (all levels), r = 3 RC = 3,
    r = 6 the generic kernel."""
    win = (2 * r + 1) ** 2
    coords = _blocks(name, r)["edge"]
    levels, want, m = _fwd_oracle(name, "edge", r, L, F32)
    views, keep = _device_levels(levels, "blocked", F32, cuda)
    c = coords.to(cuda)
    P, G, Gm = _npix(coords), L * win + 4, 8
    out = torch.full((P, 3 * G), float("nan"), device=cuda, dtype=BF16)
    flow8 = torch.full((P, 24), float("nan"), device=cuda, dtype=BF16)
    motion = torch.full((P, 4 + 3 * Gm), 5.0, device=cuda, dtype=BF16)
    _ops().corr_lookup_split_into(views, c, r, out, G, flow8, motion[:, 4:], Gm)
    hi, lo, hi2 = out[:, :G], out[:, G:2 * G], out[:, 2 * G:]
    assert torch.equal(hi.contiguous().view(torch.int16), hi2.contiguous().view(torch.int16))
    assert (out.view(P, 3, G)[:, :, L * win:] == 0).all()
    _hold(f"corr_lookup_split_into {name} r{r} L{L}", hi[:, :L * win].double() + lo[:, :L * win].double(), want,
          K.split_bound(want, m, r))
    f = _flow_want(coords, F32)
    fhi = f.bfloat16()
    flo = (f - fhi.float()).bfloat16()
    finite = torch.isfinite(f).all(1)  # inf - inf: the lo plane of a non-finite flow is NaN either way
    assert _same(flow8[:, 0:2], fhi) and _same(flow8[:, 16:18], fhi) and _same(flow8[finite, 8:10], flo[finite])
    assert (flow8.view(P, 3, 8)[:, :, 2:] == 0).all()
    mo = motion[:, 4:]
    assert _same(mo[:, 0:2], fhi) and _same(mo[:, 2 * Gm:2 * Gm + 2], fhi) and _same(mo[finite, Gm:Gm + 2], flo[finite])
    assert (motion[:, :4] == 5).all() and (mo[:, 2:Gm] == 5).all() and (mo[:, Gm + 2:2 * Gm] == 5).all()
    del keep


# ------------------------------------------------------------------------------ backward
def _start_levels(P, shapes, seed):
    """Non-zero start values in (0.25, 1]: |start| <= gmax, see test_corr_lookup_backward."""
    gen = torch.Generator().manual_seed(555 + seed)
    return [(0.25 + 0.75 * torch.rand(P, Hl, Wl, generator=gen)).double() for Hl, Wl in shapes]


@functools.lru_cache(maxsize=None)
def _bwd_case(name, block, r, L, gdtype):
    coords = _blocks(name, r)[block]
    shapes = tuple(K.LEVEL_SETS[name][:L])
    win = (2 * r + 1) ** 2
    g = K.window_grads((coords.shape[0], coords.shape[2], coords.shape[3]), L * win + 4, L * win, gdtype, r + L)
    want = K.lookup_grad_oracle([coords], [g], shapes, r)
    reach = K.lookup_grad_oracle([coords], [g], shapes, r, absolute=True)
    return coords, g, want, [x == 0 for x in reach], float(g[..., :L * win].abs().max())


@pytest.mark.parametrize("r,L", [(4, 4), (3, 4), (6, 2), (1, 3)])
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("gdtype", [F32, BF16, F16], ids=["g32", "gbf16", "gf16"])
@pytest.mark.parametrize("layout", ["rowmajor", "blocked"])
def test_corr_lookup_backward(cuda, layout, gdtype, name, r, L):
    """corr_lookup_backward_ adds the transposed blend into fp32 level buffers that start from seeded
    values in (0.25, 1], from window gradients of stride L*win + 4 whose extra channels are NaN.
    In valid columns ``buffer - start`` is within the gradient bound at T = 1: the one add to the
    start value rounds a number <= |start| + gmax <= 2 gmax, which the T (T + 1) / 2 = 1 of the
    derivation takes as gmax, so it is 9 + 2 = 11 <= 32 roundings.  Rows of non-finite queries stay
    as they were, bit for bit.  The contract of a blocked buffer: its padding columns may hold
    anything finite (the kernel takes the padded width as in range), its valid columns are right;
    the pitch tail is not touched."""
    for block in ("edge", "rand"):
        coords, g, want, untouched, gmax = _bwd_case(name, block, r, L, gdtype)
        assert gmax >= 1.0
        P = _npix(coords)
        shapes = K.LEVEL_SETS[name][:L]
        start = _start_levels(P, shapes, r)
        if layout == "blocked":
            buf0, sizes, ld = K.to_blocked(start, F32, pitch_pad=24, pad_value=0.5)
            buf = buf0.to(cuda)
            _ops().corr_lookup_backward_(K.blocked_views(buf, sizes), coords.to(cuda), g.to(cuda), r)
            after = buf.cpu()
            assert torch.isnan(after[:, ld:]).all()
            for pad in K.from_blocked(after, sizes, padding=True):
                assert torch.isfinite(pad).all()
            got = K.from_blocked(after, sizes)
            same_rows = after[:, :ld], buf0[:, :ld]
        else:
            bufs0, _ = K.to_rowmajor(start, F32, pitch_pad=8)
            bufs = [b.to(cuda) for b in bufs0]
            _ops().corr_lookup_backward_(K.rowmajor_views(bufs, shapes), coords.to(cuda), g.to(cuda), r)
            after = [b.cpu() for b in bufs]
            got = K.rowmajor_views(after, shapes)
            for a, (Hl, Wl) in zip(after, shapes):
                assert torch.isnan(a[:, Hl * Wl:]).all()
            same_rows = torch.cat([a[:, :Hl * Wl] for a, (Hl, Wl) in zip(after, shapes)], 1), \
                torch.cat([b[:, :Hl * Wl] for b, (Hl, Wl) in zip(bufs0, shapes)], 1)
        bad = ~torch.isfinite(coords.permute(0, 2, 3, 1).reshape(P, 2)).all(1)
        assert torch.equal(same_rows[0][bad], same_rows[1][bad])
        for l, (gl, wl, sl, zl) in enumerate(zip(got, want, start, untouched)):
            delta = gl.double() - sl
            assert (gl.double()[zl] == sl[zl]).all()  # nothing is added where no tap reaches
            _hold(f"corr_lookup_backward_ {layout} {name} r{r} {block} {gdtype} level {l}", delta, wl,
                  K.grad_bound(wl, 1, gmax), zl)


ROW_T = (1, 16, 17, 32, 40)


@functools.lru_cache(maxsize=None)
def _rows_case(name, r, gdtype):
    """40 lookups of the edge block, rolled by 37 queries each, so that every row meets every class
    and the rows of the non-finite queries are finite in most lookups.  The oracle rows after T
    lookups for T in ROW_T (blocked, float64)."""
    H0, W0 = K.LEVEL_SETS[name][0]
    base = K.edge_coords(H0, W0, r)
    shapes = tuple(K.LEVEL_SETS[name])
    L, win = len(shapes), (2 * r + 1) ** 2
    P = base.shape[3]
    coords = [torch.roll(base, 37 * t, dims=3).contiguous() for t in range(max(ROW_T))]
    grads = [K.window_grads((1, 1, P), L * win + 4, L * win, gdtype, 10 * r + t) for t in range(max(ROW_T))]
    want, untouched, total, reach, t0 = {}, {}, None, None, 0
    for T in ROW_T:
        part = K.lookup_grad_oracle(coords[t0:T], grads[t0:T], shapes, r)
        part_abs = K.lookup_grad_oracle(coords[t0:T], grads[t0:T], shapes, r, absolute=True)
        total = part if total is None else [a + b for a, b in zip(total, part)]
        reach = part_abs if reach is None else [a + b for a, b in zip(reach, part_abs)]
        want[T], untouched[T], t0 = total, [x == 0 for x in reach], T
    gmax = {T: max(float(g[..., :L * win].abs().max()) for g in grads[:T]) for T in ROW_T}
    return coords, grads, want, untouched, gmax


@pytest.mark.parametrize("T", ROW_T)
@pytest.mark.parametrize("r", [4, 3], ids=["r4", "r3"])
@pytest.mark.parametrize("gdtype", [BF16, F32], ids=["gbf16", "g32"])
@pytest.mark.parametrize("rdtype", [F32, BF16], ids=["rows32", "rows16"])
@pytest.mark.parametrize("name", SETS)
def test_corr_lookup_grad_rows(cuda, name, rdtype, gdtype, r, T):
    """corr_lookup_grad_rows against the float64 adjoint itself (not against the per-lookup kernel,
    whose index code it shares), exactly 0 where no lookup reaches a pixel: T at the edges of the kernel's chunks of 16, and T = 40 as 32 + 8
    with ``accumulate``; r = 4 is the RC = 4 instance, r = 3 the generic one.  Every row is
    written, the rows of queries that are NaN in some lookups too, with zero from those lookups.
    Padding columns hold something finite."""
    coords, grads, want, untouched, gmax = _rows_case(name, r, gdtype)
    shapes = K.LEVEL_SETS[name]
    sizes, ld = K.level_sizes(shapes)
    P = coords[0].shape[3]
    rows = torch.full((P, ld), float("nan"), device=cuda, dtype=rdtype)
    cs, gs = [c.to(cuda) for c in coords[:T]], [g.to(cuda) for g in grads[:T]]
    for i in range(0, T, 32):
        _ops().corr_lookup_grad_rows(rows, cs[i:i + 32], gs[i:i + 32], K.segments(sizes), r, i > 0)
    after = rows.cpu()
    assert torch.isfinite(after.float()).all()
    for l, (gl, wl, zl) in enumerate(zip(K.from_blocked(after, sizes), want[T], untouched[T])):
        partial = want[32][l] if T > 32 else None
        _hold(f"corr_lookup_grad_rows {name} r{r} T{T} {gdtype}->{rdtype} level {l}", gl, wl,
              K.grad_bound(wl, T, gmax[T], rdtype == BF16, partial), zl)


def test_corr_lookup_grad_rows_batched_grid(cuda):
    """The (2, 2, 5, 7) query grid: rows of the second image index their own coordinates."""
    name, r, T = "18x33", 4, 3
    shapes = tuple(K.LEVEL_SETS[name])
    sizes, ld = K.level_sizes(shapes)
    L, win = 4, 81
    coords = [K.random_coords(t) for t in range(T)]
    grads = [K.window_grads((2, 5, 7), L * win, L * win, BF16, 70 + t) for t in range(T)]
    want = K.lookup_grad_oracle(coords, grads, shapes, r)
    reach = K.lookup_grad_oracle(coords, grads, shapes, r, absolute=True)
    gmax = max(float(g.abs().max()) for g in grads)
    rows = torch.full((70, ld), float("nan"), device=cuda)
    _ops().corr_lookup_grad_rows(rows, [c.to(cuda) for c in coords], [g.to(cuda) for g in grads], K.segments(sizes), r, False)
    for l, (gl, wl, al) in enumerate(zip(K.from_blocked(rows.cpu(), sizes), want, reach)):
        _hold(f"corr_lookup_grad_rows batched level {l}", gl, wl, K.grad_bound(wl, T, gmax), al == 0)


# ------------------------------------------------------------------------------ unpool, padding
@pytest.mark.parametrize("H,W", [(13, 22), (17, 33)])
def test_pyramid_unpool_blocked_never_reads_padding(cuda, H, W):
    """pyramid_unpool(blocked=True) with NaN in every G row that belongs to a padding column: the
    output is finite, equals the float64 unpool elementwise, and satisfies the adjoint identity
    <unpool(G), x> == sum_l <G_l, pool_l(x)> of test_pyramid_unpool_is_the_pool_adjoint."""
    B, C = 2, 16
    shapes = [(H >> l, W >> l) for l in range(4)]
    sizes, ld = K.level_sizes(shapes)
    gen = torch.Generator().manual_seed(H * W)
    imgs = [torch.randn(B * C, Hl, Wl, generator=gen) for Hl, Wl in shapes]  # (B*C) "queries" of (Hl, Wl)
    buf, _, _ = K.to_blocked(imgs, F32, pad_value=float("nan"))
    G = buf.reshape(B, C, ld).permute(0, 2, 1).contiguous()  # (B, ld, C)
    assert torch.isnan(G).any()
    out = _ops().pyramid_unpool(G.to(cuda), H, W, K.segments(sizes), True).cpu()
    assert out.shape == (B, H * W, C) and torch.isfinite(out).all()
    want = torch.zeros(B, C, H, W, dtype=torch.float64)
    for l, img in enumerate(imgs):
        Hl, Wl = img.shape[1:]
        up = F.interpolate(img.double().reshape(B, C, Hl, Wl), scale_factor=2 ** l, mode="nearest") * 0.25 ** l
        want[:, :, :up.shape[2], :up.shape[3]] += up
    got = out.double().permute(0, 2, 1).reshape(B, C, H, W)
    # four terms of |g| * 4^-l, three fp32 adds and the exact scalings
    mag = sum(F.interpolate(img.abs().double().reshape(B, C, *img.shape[1:]), scale_factor=2 ** l).amax() * 0.25 ** l
              for l, img in enumerate(imgs))
    err = (got - want).abs().max().item()
    print(f"pyramid_unpool blocked {H}x{W}: max |err| / (4 u32 mag) = {err / (4 * K.U32 * float(mag)):.3f}")
    assert err <= 4 * K.U32 * float(mag)
    x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
    lhs = (got * x).sum()
    rhs = sum((img.double().reshape(B, C, *img.shape[1:]) * p).sum() for img, p in zip(imgs, K.pool_levels(x, 4)))
    assert abs((lhs - rhs) / rhs).item() < 1e-6


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("H,W", [(17, 21), (18, 33)])
def test_volume_padding_columns_are_zero(cuda, H, W, split):
    """The forward volume's padding columns are exactly zero in every level: the lookups take the
    padded width as in range and rely on it."""
    from raft_ros_amd.ops.corr import CorrPyramid

    f1, f2 = K.features(1, 64, H, W, H + W)
    cp = CorrPyramid(f1.to(cuda), f2.to(cuda), 4, 4, split=split)
    st = cp.state
    assert st.buf.dtype == (F32 if split else BF16) and [s[:2] for s in st.sizes] == [(H >> l, W >> l) for l in range(4)]
    buf = st.buf.cpu()
    assert torch.isfinite(buf.float()).all()
    for l, pad in enumerate(K.from_blocked(buf, st.sizes, padding=True)):
        assert pad.shape[2] == -(W >> l) % 16 and (pad == 0).all(), l  # 18x33: level 1 is one whole block
    for lv in K.from_blocked(buf, st.sizes):
        assert lv.float().abs().max() > 0.1


# ------------------------------------------------------------------------------ end to end
def _edge_fields(T, B, H, W, r, seed, n=None):
    """T coordinate fields that hold the edge block of an HxW level set, the nine non-finite queries
    first."""
    block = K.edge_coords(H, W, r)
    nf = len(K.NONFINITE)
    block = torch.cat([block[..., -nf:], block[..., :-nf]], 3)
    return K.embed_fields(T, B, H, W, block[..., :n].contiguous() if n else block, seed)


def test_corr_pyramid_split_end_to_end(cuda):
    """CorrPyramid(split=True) at 2 x 64 x 17 x 21: three lookups whose fields hold the edge block,
    then backward.  The forward is within 16 u32 m + (3C + 16) u32 S of the float64 lookup of the
    float64 volume; f1.grad and f2.grad match float64 autograd to the 3e-5 relative norm of
    test_corr_pyramid_split_is_fp32_faithful; non-finite queries give zeros."""
    from raft_ros_amd.ops.corr import CorrPyramid

    B, C, H, W, r, L, T = 2, 64, 17, 21, 4, 4, 3
    f1, f2 = K.features(B, C, H, W, 11)
    fields = _edge_fields(T, B, H, W, r, 3)
    gouts = [K.window_grads((B, H, W), L * 81, L * 81, F32, 40 + t) for t in range(T)]
    a, b = f1.to(cuda).requires_grad_(True), f2.to(cuda).requires_grad_(True)
    cp = CorrPyramid(a, b, L, r, split=True)
    outs = [cp(c.to(cuda)) for c in fields]  # (B, Ch, H, W) views of NHWC
    a64, b64 = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    levels, S = K.local_levels(a64, b64, L)
    m = K.level_max([lv.detach() for lv in levels])
    bound = K.e2e_fwd_bound(m, S, r, C)
    loss64 = 0.0
    for t, (o, c, g) in enumerate(zip(outs, fields, gouts)):
        want = K.lookup_oracle(levels, c, r)
        _hold(f"CorrPyramid split end to end lookup {t}", o.permute(0, 2, 3, 1).reshape(B * H * W, -1),
              want.reshape(B * H * W, -1), bound)
        loss64 = loss64 + (want * g.double()).sum()
    sum((o.permute(0, 2, 3, 1) * g.to(cuda)).sum() for o, g in zip(outs, gouts)).backward()
    w1, w2 = torch.autograd.grad(loss64, (a64, b64))
    for tag, got, want in (("f1", a.grad, w1), ("f2", b.grad, w2)):
        rel = ((got.cpu().double() - want).norm() / want.norm()).item()
        print(f"CorrPyramid split end to end d{tag}: relative norm {rel:.3e} (3e-5)")
        assert torch.isfinite(got).all() and rel < 3e-5


# ------------------------------------------------------------------------------ local correlation
LB, LH, LW = 4, 17, 21


@functools.lru_cache(maxsize=None)
def _local_field(r):
    """(4, 2, 17, 21): the edge block, then grid + 3 randn; in that smooth part a far-out query and a
    NaN query sit in the middle of 8x4 tiles of the last image."""
    f = _edge_fields(1, LB, LH, LW, r, 21)[0]
    assert K.edge_coords(LH, LW, r).shape[3] < 3 * LH * LW + 5 * LW  # rows 5.. of the last image are smooth
    f[3, :, 9, 10] = torch.tensor([-3.0e4, 5.0e5])
    f[3, :, 13, 4] = torch.tensor([float("nan"), 6.5])
    return f.contiguous()


@functools.lru_cache(maxsize=None)
def _local_case(C, r, rounded):
    """Features (bf16 values when ``rounded``), field, upstream gradient, float64 oracle, S and the
    float64 feature gradients."""
    f1, f2 = K.features(LB, C, LH, LW, C + r, BF16 if rounded else F32)
    f1, f2 = f1.float(), f2.float()
    coords = _local_field(r)
    win = (2 * r + 1) ** 2
    g = K.window_grads((LB, LH, LW), 4 * win, 4 * win, F32, C)
    a64, b64 = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
    want, S = K.local_lookup_oracle(a64, b64, coords, 4, r)
    w1, w2 = torch.autograd.grad((want * g.double()).sum(), (a64, b64))
    return f1, f2, coords, g, want.detach().reshape(LB * LH * LW, -1), S, w1, w2


def _nonfinite_pixels(coords):
    return ~torch.isfinite(coords).all(1)  # (B, H, W)


def _local_run(cuda, f1, f2, coords, g, r, split, grad=True, out_dtype=None):
    from raft_ros_amd.ops.corr import LocalCorrPyramid

    a, b = f1.to(cuda).requires_grad_(grad), f2.to(cuda).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        lc = LocalCorrPyramid(a, b, 4, r, split=split)
        out = lc(coords.to(cuda), out_dtype=out_dtype)  # (B, Ch, H, W)
        if grad:
            (out.float() * g.to(cuda).permute(0, 3, 1, 2)).sum().backward()
    return lc, out.detach().permute(0, 2, 3, 1).reshape(LB * LH * LW, -1), a.grad, b.grad


def test_local_corr_scalar_fp32(cuda):
    """The exact scalar kernel (split=True with autograd): forward within (2C + 16 + 4l) u32 S, dF1
    exactly zero at non-finite queries, dF1 and dF2 against float64 autograd at the 1e-4 of
    test_local_corr_fwd_bwd."""
    C, r = 64, 4
    f1, f2, coords, g, want, S, w1, w2 = _local_case(C, r, False)
    lc, out, d1, d2 = _local_run(cuda, f1, f2, coords, g, r, split=True)
    assert not lc.mfma
    _hold("LocalCorrPyramid scalar fp32", out, want, K.local_bound(want, S, r, C, "scalar"))
    bad = _nonfinite_pixels(coords)
    assert bad.sum() == len(K.NONFINITE) + 1 and (d1.cpu().permute(0, 2, 3, 1)[bad] == 0).all()
    torch.testing.assert_close(d1.cpu().double(), w1, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(d2.cpu().double(), w2, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("C,r", [(64, 4), (128, 3)])
@pytest.mark.parametrize("odt", [F32, BF16], ids=["out32", "out16"])
def test_local_corr_mfma_bf16(cuda, C, r, odt):
    """The MFMA kernel on bf16 operands: forward within (C + 16 + 4l) u32 S + u_bf16 S + u_out
    |oracle| (32 queries share one window box: the far-out and the NaN query sit inside smooth
    tiles), dF1 zero at non-finite queries, gradients to the 2e-2 relative norm of
    test_local_corr_mfma_matches_dense_reference."""
    f1, f2, coords, g, want, S, w1, w2 = _local_case(C, r, True)
    lc, out, d1, d2 = _local_run(cuda, f1, f2, coords, g, r, split=False, out_dtype=odt)
    assert lc.mfma and not lc.split_mfma and out.dtype == odt
    _hold(f"LocalCorrPyramid MFMA bf16 C{C} r{r} {odt}", out, want, K.local_bound(want, S, r, C, "mfma", odt))
    bad = _nonfinite_pixels(coords)
    assert (d1.cpu().permute(0, 2, 3, 1)[bad] == 0).all()
    for tag, got, w in (("dF1", d1, w1), ("dF2", d2, w2)):
        rel = ((got.cpu().double() - w).norm() / w.norm()).item()
        print(f"LocalCorrPyramid MFMA bf16 C{C} r{r} {tag}: relative norm {rel:.3e} (2e-2)")
        assert torch.isfinite(got).all() and rel < 2e-2


def test_local_corr_split_mfma(cuda):
    """The split-bf16 MFMA kernel (fp32 inference): within (3C + 16 + 4l) u32 S + 4 2^-16 S."""
    C, r = 64, 4
    f1, f2, coords, g, want, S, _, _ = _local_case(C, r, False)
    lc, out, _, _ = _local_run(cuda, f1, f2, coords, g, r, split=True, grad=False)
    assert lc.mfma and lc.split_mfma
    _hold("LocalCorrPyramid split MFMA", out, want, K.local_bound(want, S, r, C, "split"))


@pytest.mark.parametrize("split", [True, False], ids=["scalar", "mfma"])
def test_local_corr_deterministic_backward(cuda, split):
    """The deterministic (fixed-point) dF2 accumulation on the same field: against the float-atomic
    one to the 1e-5 relative norm of test_deterministic_local_corr_grads_match_float_atomics, and
    against float64 autograd like the float-atomic mode; dF1 zero at non-finite queries."""
    C, r = 64, 4
    f1, f2, coords, g, want, S, w1, w2 = _local_case(C, r, not split)
    prev = torch.are_deterministic_algorithms_enabled()
    grads = {}
    try:
        for det in (False, True):
            torch.use_deterministic_algorithms(det, warn_only=True)
            _, _, d1, d2 = _local_run(cuda, f1, f2, coords, g, r, split=split)
            grads[det] = (d1.cpu().double(), d2.cpu().double())
    finally:
        torch.use_deterministic_algorithms(prev)
    rel = ((grads[True][1] - grads[False][1]).norm() / grads[False][1].norm()).item()
    print(f"LocalCorrPyramid deterministic vs float-atomic dF2 ({'scalar' if split else 'mfma'}): {rel:.3e} (1e-5)")
    assert rel < 1e-5
    bad = _nonfinite_pixels(coords)
    assert (grads[True][0].permute(0, 2, 3, 1)[bad] == 0).all()
    if split:
        torch.testing.assert_close(grads[True][0], w1, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(grads[True][1], w2, rtol=1e-4, atol=1e-4)
    else:
        for got, w in zip(grads[True], (w1, w2)):
            assert ((got - w).norm() / w.norm()).item() < 2e-2
