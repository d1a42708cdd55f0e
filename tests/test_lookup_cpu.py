"""The float64 oracles, layout helpers, coordinate classes and error bounds of lookup_cases.py,
checked on the host against ops/reference.py evaluated in float64 and against the layout code of
ops/corr.py.  No GPU."""
import pytest
import torch

import lookup_cases as K
from raft_ros_amd.ops import corr as corr_ops
from raft_ros_amd.ops import reference as ref

SETS = list(K.LEVEL_SETS)


def _ref_lookup(levels, coords, r):
    """reference.pyramid_lookup's levels loop in the dtype of ``levels`` (its own ends in
    ``.float()``): (B, H, W, L*(2r+1)^2)."""
    B, _, H, W = coords.shape
    dt = levels[0].dtype
    c = coords.to(dt).permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    delta = ref.window_offsets(r, dtype=dt)[None]
    outs = [ref.bilinear_sampler(lv[:, None], c / (2 ** l) + delta).reshape(B, H, W, -1) for l, lv in enumerate(levels)]
    return torch.cat(outs, -1)


def _finite_block(name, r):
    H0, W0 = K.LEVEL_SETS[name][0]
    c = K.edge_coords(H0, W0, r)
    return c[..., :K.n_finite(H0, W0, r)].contiguous()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("r", [1, 3, 4, 6])
def test_lookup_oracle_matches_float64_reference(name, r):
    shapes = tuple(K.LEVEL_SETS[name])
    for coords in (_finite_block(name, r), K.random_coords()):
        P = coords.shape[0] * coords.shape[2] * coords.shape[3]
        levels = list(K.level_values(P, shapes, torch.float32))
        got = K.lookup_oracle(levels, coords, r)
        want = _ref_lookup(levels, coords, r)
        err = (got - want).abs().max().item()
        print(name, r, tuple(coords.shape), "oracle vs float64 reference", err)
        assert err < 1e-12


@pytest.mark.parametrize("name", SETS)
def test_lookup_grad_oracle_matches_float64_autograd(name):
    shapes, r, T = tuple(K.LEVEL_SETS[name]), 4, 2
    n = len(shapes) * (2 * r + 1) ** 2
    cs = [_finite_block(name, r), _finite_block(name, r).flip(3).contiguous()]
    P = cs[0].shape[3]
    gs = [K.window_grads((1, 1, P), n + 4, n, torch.float32, t) for t in range(T)]
    got = K.lookup_grad_oracle(cs, gs, shapes, r)
    levels = [torch.zeros(P, Hl, Wl, dtype=torch.float64, requires_grad=True) for Hl, Wl in shapes]
    loss = sum((_ref_lookup(levels, c, r) * g[..., :n].double()).sum() for c, g in zip(cs, gs))
    want = torch.autograd.grad(loss, levels)
    for l, (a, b) in enumerate(zip(got, want)):
        err = (a - b).abs().max().item()
        print(name, "level", l, "grad oracle vs float64 autograd", err)
        assert err < 1e-12 and b.abs().max() > 0.1


@pytest.mark.parametrize("rounded", [False, True])
def test_local_lookup_oracle_matches_float64_reference(rounded):
    B, C, H, W, L, r = 1, 16, 17, 21, 4, 3
    f1, f2 = K.features(B, C, H, W, 1, torch.bfloat16 if rounded else torch.float32)
    block = _finite_block("17x21", r)
    coords = K.embed_fields(3, B, H, W, block[..., :3 * H * W].contiguous(), 5)[1]
    got, S = K.local_lookup_oracle(f1, f2, coords, L, r)
    win = (2 * r + 1) ** 2
    for l, p in enumerate(K.pool_levels(f2.double(), L)):
        want = ref.local_corr(f1.double(), p, coords.double() / 2 ** l, r).permute(0, 2, 3, 1) / C ** 0.5
        err = (got[..., l * win:(l + 1) * win] - want).abs().max().item()
        print("local oracle level", l, err)
        assert err < 1e-11
        assert (got[..., l * win:(l + 1) * win].abs().reshape(-1, win).amax(1) <= S[:, l]).all()
    assert S.shape == (B * H * W, L) and (S > 0).all()


def test_non_finite_queries_give_exact_zeros():
    name, r = "18x33", 4
    shapes = tuple(K.LEVEL_SETS[name])
    coords = K.edge_coords(*shapes[0], r)
    P, nf = coords.shape[3], len(K.NONFINITE)
    assert not torch.isfinite(coords[0, :, 0, -nf:]).all(0).any() and torch.isfinite(coords[0, :, 0, :-nf]).all()
    levels = list(K.level_values(P, shapes, torch.float32))
    out = K.lookup_oracle(levels, coords, r)
    assert (out[0, 0, -nf:] == 0).all() and not torch.isnan(out).any()
    n = len(shapes) * (2 * r + 1) ** 2
    g = K.window_grads((1, 1, P), n, n, torch.float32, 3)
    for lv in K.lookup_grad_oracle([coords], [g], shapes, r):
        assert (lv[-nf:] == 0).all() and torch.isfinite(lv).all()
    f1, f2 = K.features(1, 8, 17, 21, 2)
    field = K.embed_fields(1, 1, 17, 21, coords[..., -nf:].contiguous(), 1)[0]
    f1 = f1.requires_grad_(True)
    lo, _ = K.local_lookup_oracle(f1, f2, field, 4, 2)
    assert (lo.reshape(-1, lo.shape[-1])[:nf] == 0).all()
    lo.sum().backward()
    assert (f1.grad.reshape(8, -1)[:, :nf] == 0).all() and f1.grad.abs().max() > 0


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_blocked_layout_round_trip_and_index(name, dtype):
    shapes = tuple(K.LEVEL_SETS[name])
    P = 3
    levels = K.level_values(P, shapes, dtype)
    buf, sizes, ld = K.to_blocked(levels, dtype, pitch_pad=24)
    assert buf.shape == (P, ld + 24) and torch.isnan(buf[:, ld:]).all() and not torch.isnan(buf[:, :ld]).any()
    for back, pad, lv in zip(K.from_blocked(buf, sizes), K.from_blocked(buf, sizes, padding=True), levels):
        assert torch.equal(back.double(), lv) and (pad == 0).all() and pad.shape[2] == K.pad16(lv.shape[2]) - lv.shape[2]
    # the documented index, pixel by pixel
    for lv, (Hl, Wl, off) in zip(levels, sizes):
        y, x = torch.meshgrid(torch.arange(Hl), torch.arange(Wl), indexing="ij")
        idx = off + ((x // 16) * Hl + y) * 16 + x % 16
        assert torch.equal(buf[:, idx.reshape(-1)].double(), lv.reshape(P, -1))
    # the strides of _PyramidState.views (pitch ld) on a buffer without a pitch tail
    tight, sizes2, ld2 = K.to_blocked(levels, dtype)
    st = corr_ops._PyramidState(len(shapes), 4)
    st.sizes, st.ld = sizes2, ld2
    for a, b in zip(st.views(tight), K.blocked_views(tight, sizes2)):
        assert a.shape == b.shape and a.stride() == b.stride() and a.storage_offset() == b.storage_offset()
    assert st.segments() == K.segments(sizes2)
    # and the order _concat_levels(blocked=True) gives the pooled operand: level images as (1, P, Hl, Wl)
    fs = [lv.float()[None] for lv in levels]
    cat = corr_ops._concat_levels(fs, ld2, [off for _, _, off in sizes2], nchw=True, blocked=True)
    assert torch.equal(cat[0].to(dtype).float(), tight.float())


@pytest.mark.parametrize("name", SETS)
def test_rowmajor_twin_has_nan_gaps(name):
    shapes = tuple(K.LEVEL_SETS[name])
    levels = K.level_values(2, shapes, torch.float32)
    bufs, views = K.to_rowmajor(levels, torch.float32)
    for b, v, lv in zip(bufs, views, levels):
        n = lv.shape[1] * lv.shape[2]
        assert v.stride(0) > n and torch.isnan(b[:, n:]).all() and torch.equal(v.double(), lv)


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("r", [1, 3, 4, 6])
def test_every_coordinate_class_is_present(name, r):
    shapes = K.LEVEL_SETS[name]
    H0, W0 = shapes[0]
    coords = K.edge_coords(H0, W0, r)
    q = coords[0, :, 0].t()  # (n, 2)
    e = 2.0 ** -10

    def f32(v):
        return torch.tensor(v, dtype=torch.float32)

    for axis, n, extra in ((0, W0, [K.pad16(W0) - 0.5, K.pad16(W0)]), (1, H0, [])):
        named = [-1e4, -40, -(r + 1), -(r + 1) + e, -r - e, -5.001, -1, -0.5, -1e-7, 0, 0.125, 0.5, 7, 7.875, 8, 15,
                 15.5, 16, n - 1, n - 1 + e, n - 0.5, n, n + r - e, n + r, 40, 1e4, 999999.5, 1e6, 1e6 + 1, 2.0 ** 31,
                 -2.0 ** 31, 3e38, -3e38] + extra
        for v in named:
            assert (q[:, axis] == f32(v)).any(), (axis, v)
        for v in (float("inf"), float("-inf")):
            assert ((q[:, axis] == v) & torch.isfinite(q[:, 1 - axis])).any() and (q == v).all(1).any()
        assert (torch.isnan(q[:, axis]) & torch.isfinite(q[:, 1 - axis])).any()
    assert torch.isnan(q).all(1).any()
    assert ((q[:, 0] >= W0) & (q[:, 0] < K.pad16(W0)) & (q[:, 1] >= 0) & (q[:, 1] < H0)).any()  # in [Wl, Wpad)
    # the distinct values survive fp32: just inside / outside are not the border itself
    assert f32(-(r + 1) + e) > -(r + 1) and f32(-r - e) < -r and f32(W0 + r - e) < W0 + r and f32(-1e-7) < 0
    for l, cls in enumerate(K.window_classes(coords, shapes, r)):
        Hl, Wl = shapes[l]
        for k in ("fx==0", "fy==0", "partly", "outside"):
            assert cls[k].any(), (l, k)
        assert (cls["fx==0"] & cls["fy==0"] & ~cls["outside"]).any(), l
        assert (~cls["fx==0"] & ~cls["fy==0"] & ~cls["outside"]).any(), l
        # a (2r+2)^2 neighbourhood fits a level only if the level is that large; in a smaller one the
        # most a window can have inside is its centre tap with all four neighbours
        if min(Hl, Wl) >= 2 * r + 2:
            assert cls["inside"].any(), l
        else:
            assert not cls["inside"].any(), l
        assert (cls["centre"] & cls["partly"]).any(), l
    # level 0 integers are halves, quarters and eighths further up
    t15 = [15 * 2.0 ** -l for l in range(4)]
    assert (q == f32(15.0)).any() and [t - int(t) for t in t15] == [0.0, 0.5, 0.75, 0.875]


def test_random_block_shape():
    c = K.random_coords()
    assert c.shape == (2, 2, 5, 7) and torch.isfinite(c).all()


@pytest.mark.parametrize("name", SETS)
def test_forward_bound_is_of_the_right_order(name):
    """The fp32 reference (grid_sample, which normalises and un-normalises the coordinates) against
    the oracle lies within the forward bound with 16 replaced by 32, and not orders below it: the
    bound is neither unreachable nor loose by orders of magnitude."""
    shapes, r = tuple(K.LEVEL_SETS[name]), 4
    win = (2 * r + 1) ** 2
    worst = 0.0
    for coords in (_finite_block(name, r), K.random_coords()):
        # |x| <= 1e4: beyond, the reference's fp32 normalisation is off by whole pixels, all zeros anyway
        keep = (coords.abs() <= 1e4).all(1).reshape(-1)
        P = keep.numel()
        levels = list(K.level_values(P, shapes, torch.float32))
        want = K.lookup_oracle(levels, coords, r).reshape(P, -1)
        got = ref.pyramid_lookup([lv.float()[:, None] for lv in levels], coords, r).permute(0, 2, 3, 1).reshape(P, -1)
        bound = 2 * K.fwd_bound(want, K.level_max(levels), r, torch.float32)
        err = (got.double() - want).abs()
        assert (err[keep] <= bound[keep]).all(), K.ratio(err[keep], bound[keep])
        worst = max(worst, K.ratio(err[keep], bound[keep]))
    print(name, "fp32 reference error / (32 u32 m)", worst)
    assert worst > 0.01


def test_bounds_scale_as_documented():
    o = torch.tensor([[2.0, -4.0]], dtype=torch.float64)
    m = torch.tensor([[8.0, 16.0]], dtype=torch.float64)
    b = K.fwd_bound(o, m, 0, torch.bfloat16)
    assert torch.equal(b, torch.tensor([[16 * K.U32 * 8 + 2.0 ** -8 * 2, 16 * K.U32 * 16 + 2.0 ** -8 * 4]], dtype=torch.float64))
    assert torch.equal(K.fwd_bound(o, m, 0, torch.float32), 16 * K.U32 * m)
    assert torch.equal(K.split_bound(o, m, 0), 16 * K.U32 * m + 2.0 ** -16 * o.abs())
    assert torch.equal(K.grad_bound(o, 17, 3.0), torch.full_like(o, 32 * 17 * K.U32 * 3.0))
    S = torch.tensor([[1.0, 2.0]], dtype=torch.float64)
    assert torch.equal(K.local_bound(o, S, 0, 64, "scalar"), torch.tensor([[144 * K.U32, 148 * K.U32 * 2]], dtype=torch.float64))
    assert torch.equal(K.local_bound(o, S, 0, 64, "split"),
                       torch.tensor([[208 * K.U32 + 4 * 2.0 ** -16, (212 * K.U32 + 4 * 2.0 ** -16) * 2]], dtype=torch.float64))
