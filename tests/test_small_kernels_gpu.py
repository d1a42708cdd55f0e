"""The small streaming HIP kernels against float64 / plain-torch oracles (small_kernel_cases.py):
the fused sequence loss above its grid cap and at its edges, the NHWC instance norm at its chunk and
row-count boundaries and with |mean| >> std, and the update-block helpers on strided column slices
with guarded outputs."""
import pytest
import torch
import torch.nn.functional as F

import small_kernel_cases as K
from raft_ros_amd.train import loss as L

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24


def _ops():
    from raft_ros_amd.ops._ext import ops

    return ops()


# ------------------------------------------------------------------------------ sequence loss
def _run_loss(cuda, preds, gt, valid, gamma, max_flow, upstream=1.0):
    """Fused loss, metrics and gradients for ``(upstream * loss).backward()``, on the host."""
    p = [t.to(cuda).requires_grad_(True) for t in preds]
    g, v = gt.to(cuda), valid.to(cuda)
    assert L._fused_ok(p, g)
    loss, m = L.sequence_loss(p, g, v, gamma, max_flow)
    (upstream * loss).backward()
    sums = _ops().seq_loss([t.detach() for t in p], g, v, gamma, max_flow)
    return loss.detach().cpu(), {k: t.cpu() for k, t in m.items()}, sums.cpu(), [t.grad.cpu() for t in p]


def _check_grads(grads, want, mask, preds, gt, n):
    m = mask[:, None].expand_as(gt)
    for k, (g, w) in enumerate(zip(grads, want)):
        d = preds[k] - gt
        zero = ~m | (d == 0)
        assert (g[zero] == 0).all() and (g[~zero] != 0).all(), k  # the zero pattern, exactly
        assert torch.equal(torch.sign(g), torch.sign(w).float()), k  # the sign, exactly
        err = (g.double() - w).abs()
        assert (err <= (n + 1) * EPS24 * w.abs()).all(), (k, (err / w.abs().clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("name", ["stride", "cap", "one", "maxpreds", "params"])
def test_seq_loss_matches_float64_oracle(cuda, name):
    """Loss, raw sums, metrics and every gradient, with an upstream gradient of 2.5; 'stride' and
    'cap' are above the 2048-block grid cap and run the grid-stride loop of both kernels."""
    preds, gt, valid, gamma, max_flow = K.loss_case(name)
    want = K.loss_expected(name, 2.5)
    loss, m, sums, grads = _run_loss(cuda, preds, gt, valid, gamma, max_flow, 2.5)
    s = want["sums"]
    print(name, "loss", loss.item(), want["loss"].item(), "sums", sums.tolist(), s.tolist())
    assert torch.equal(sums[2:].double(), s[2:]) and s[5] < 2 ** 24  # counts: exact integers
    torch.testing.assert_close(loss.double(), want["loss"], rtol=1e-5, atol=0)
    torch.testing.assert_close(sums[:2].double(), s[:2], rtol=1e-5, atol=0)
    cnt = s[5].clamp_min(1.0)
    for j, k in enumerate(("epe", "1px", "3px", "5px")):
        torch.testing.assert_close(m[k].double(), s[1 + j] / cnt, rtol=1e-5, atol=0)
    _check_grads(grads, want["grads"], want["mask"], preds, gt, len(preds))


def test_seq_loss_inside_a_sum_with_another_term(cuda):
    preds, gt, valid, gamma, max_flow = K.loss_case("params")
    want = K.loss_expected("params", 1.0)
    p = [t.to(cuda).requires_grad_(True) for t in preds]
    other = torch.arange(5.0, device=cuda, requires_grad=True)
    loss, _ = L.sequence_loss(p, gt.to(cuda), valid.to(cuda), gamma, max_flow)
    (loss + 0.5 * (other * other).sum()).backward()
    assert torch.equal(other.grad, other.detach())
    _check_grads([t.grad.cpu() for t in p], want["grads"], want["mask"], preds, gt, len(preds))


def test_seq_loss_stride_step_pixel(cuda):
    """Every prediction equals gt except at one valid pixel that only the second grid-stride step
    reaches: the raw sums follow exactly, and the gradient is non-zero at its two entries only."""
    preds, gt, valid, gamma, max_flow, (b, s) = K.stride_step_case()
    want = K.seq_loss_oracle(preds, gt, valid, gamma, max_flow)
    _, _, sums, grads = _run_loss(cuda, preds, gt, valid, gamma, max_flow)
    nvalid = want["sums"][5].item()
    print("stride step sums", sums.tolist(), "valid", nvalid)
    # 7 * (1 + gamma): one product and one sum in fp32, the rest of the field adds zeros
    torch.testing.assert_close(sums[0].double(), torch.tensor(7 * sum(want["weights"]), dtype=torch.float64),
                               rtol=2 * EPS24, atol=0)
    assert sums[1:].tolist() == [5.0, nvalid - 1, nvalid - 1, nvalid - 1, nvalid]  # 5 is not < 5
    B = gt.shape[0]
    for k, g in enumerate(grads):
        hit = torch.zeros_like(g, dtype=torch.bool)
        hit.view(B, 2, -1)[b, :, s] = True
        assert (g[~hit] == 0).all() and (g[hit] > 0).all(), k
    _check_grads(grads, want["grads"], want["mask"], preds, gt, len(preds))


def test_seq_loss_all_invalid_batch(cuda):
    preds, gt, valid, gamma, max_flow = K.loss_case("params")
    for v, g in ((torch.zeros_like(valid), gt), (valid, torch.full_like(gt, 300.0))):  # by valid, by |gt|
        loss, m, sums, grads = _run_loss(cuda, preds, g, v, gamma, max_flow, 2.5)
        assert loss.item() == 0 and sums.tolist() == [0.0] * 6
        assert all(t.item() == 0 and torch.isfinite(t) for t in m.values())
        assert all((t == 0).all() for t in grads)


def test_seq_loss_is_deterministic(cuda):
    preds, gt, valid, gamma, max_flow = K.loss_case("stride")
    a = _run_loss(cuda, preds, gt, valid, gamma, max_flow, 2.5)
    b = _run_loss(cuda, preds, gt, valid, gamma, max_flow, 2.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


def test_seq_loss_33_predictions_take_the_fallback(cuda):
    preds, gt, valid, gamma, max_flow = K.loss_case("maxpreds")
    preds = preds + [preds[-1].clone()]
    assert len(preds) == K.K_MAX_PREDS + 1
    want = K.seq_loss_oracle(preds, gt, valid, gamma, max_flow)
    p = [t.to(cuda).requires_grad_(True) for t in preds]
    assert not L._fused_ok(p, gt.to(cuda))
    loss, _ = L.sequence_loss(p, gt.to(cuda), valid.to(cuda), gamma, max_flow)
    torch.testing.assert_close(loss.detach().cpu().double(), want["loss"], rtol=1e-5, atol=0)
    with pytest.raises(RuntimeError, match="1..32 predictions"):
        _ops().seq_loss([t.detach() for t in p], gt.to(cuda), valid.to(cuda), gamma, max_flow)
    with pytest.raises(RuntimeError, match="1..32 predictions"):
        _ops().seq_loss_backward([t.detach() for t in p], gt.to(cuda), valid.to(cuda), torch.ones(1, device=cuda),
                                 gamma, max_flow)


# ------------------------------------------------------------------------------ instance norm
def _run_norm(cuda, x, dy, relu):
    """(y, dx, mean, rstd) of the HIP op through InstanceNorm2dNHWC and autograd.grad, on the host."""
    from raft_ros_amd.ops.norm import InstanceNorm2dNHWC

    xd = x.to(cuda).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = InstanceNorm2dNHWC(x.shape[1])(xd, relu=relu)
    assert y.dtype == x.dtype and y.is_contiguous(memory_format=torch.channels_last)
    (dx,) = torch.autograd.grad(y, xd, dy.to(cuda))
    _, stats = _ops().instance_norm_fwd(xd.detach(), relu, 1e-5)
    return y.detach().cpu(), dx.cpu(), stats[..., 0].cpu(), stats[..., 1].cpu()


def _check_norm(got, want, dtype, tag):
    y, dx, mean, rstd = got
    yw, dxw, meanw, rstdw = want
    tol = K.NORM_TOL[dtype]
    print(tag, "max |y - oracle| %.3g" % (y.double() - yw).abs().max().item(),
          "max |dx - oracle| %.3g" % (dx.double() - dxw).abs().max().item())
    torch.testing.assert_close(y.double(), yw, **tol)
    torch.testing.assert_close(dx.double(), dxw, **tol)
    # the saved statistics are fp32 for either dtype
    torch.testing.assert_close(mean.double(), meanw, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(rstd.double(), rstdw, rtol=1e-4, atol=0)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", K.NORM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_instance_norm_matches_float64_oracle(cuda, shape, dtype, relu):
    x, dy = K.norm_case(shape, dtype)
    got = _run_norm(cuda, x, dy, relu)
    _check_norm(got, K.instance_norm_oracle(x, relu, 1e-5, dy), dtype, f"{shape} {dtype} relu={relu}")
    if shape[2] * shape[3] == 1:  # one pixel: x - mean is exactly 0
        assert (got[0] == 0).all() and (got[1] == 0).all()


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("kind", K.NORM_OFFSETS)
def test_instance_norm_with_a_mean_far_from_zero(cuda, kind, relu):
    """|mean| of 8, 32 and 100 standard deviations, a constant channel, and bf16-exact integers
    around 100: E[x^2] - E[x]^2 in fp32 loses 2 log2(mean / std) bits here.  torch's fp32
    instance_norm on the same device input has to meet the tolerance first, so that a failure
    points at the kernel and not at the case.  Measured on an MI355X, max |y - oracle| in fp32:
    the sums of x and x^2 that the kernel used to take gave 7.0e-5 / 1.0e-3 / 9.7e-3 at
    8 / 32 / 100 std and 3.8e-4 on the constant channel (tolerance 1e-4); the pivoted,
    Chan-combined statistics give 3.6e-6 / 5.3e-6 / 1.2e-5 and an exact 0, torch 3.0e-6 /
    1.1e-5 / 3.1e-5 and 9e-7."""
    x, dy = K.norm_offset_case(kind)
    want = K.instance_norm_oracle(x, relu, 1e-5, dy)
    tol = K.NORM_TOL[x.dtype]
    xr = x.to(cuda).float().requires_grad_(True)
    yr = F.instance_norm(xr, eps=1e-5)
    yr = torch.relu(yr) if relu else yr
    (dxr,) = torch.autograd.grad(yr, xr, dy.to(cuda).float())
    print(kind, "torch fp32: max |y - oracle| %.3g" % (yr.detach().cpu().double() - want[0]).abs().max().item(),
          "max |dx - oracle| %.3g" % (dxr.cpu().double() - want[1]).abs().max().item())
    torch.testing.assert_close(yr.detach().cpu().double(), want[0], **tol)
    # torch's y on the constant channel is rounding noise of either sign, and so is its ReLU' there
    ch = [c for c in range(x.shape[1]) if not (kind == "const" and relu and c == 5)]
    torch.testing.assert_close(dxr.cpu().double()[:, ch], want[1][:, ch], **tol)
    got = _run_norm(cuda, x, dy, relu)
    _check_norm(got, want, x.dtype, f"{kind} relu={relu} kernel:")
    if kind == "const":  # the sums about the pivot are exactly 0: the mean is exact and y is 0
        assert (got[0][:, 5] == 0).all() and (got[2][:, 5] == K.f32(3.3)).all()


# ------------------------------------------------------------------------------ update-block helpers
GUARD = 7.0
P_BIG = 2 * 23 * 31


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _sliced(cuda, t, width, c0, fill=GUARD):
    """``t`` (P, C) as columns [c0, c0 + C) of a guard-filled (P, width) device buffer."""
    buf = torch.full((t.shape[0], width), fill, dtype=t.dtype, device=cuda)
    buf[:, c0:c0 + t.shape[1]] = t.to(cuda)
    return buf, buf[:, c0:c0 + t.shape[1]]


def _guarded(cuda, P, C, width, c0, dtype, fill):
    buf = torch.full((P, width), fill, dtype=dtype, device=cuda)
    return buf, buf[:, c0:c0 + C]


def _guard_kept(buf, c0, C, fill):
    """Every column outside [c0, c0 + C) still holds the guard, bitwise."""
    keep = torch.ones(buf.shape[1], dtype=torch.bool)
    keep[c0:c0 + C] = False
    return _same_bits(buf[:, keep.to(buf.device)], torch.full_like(buf[:, keep.to(buf.device)], fill))


def _within_one_bf16_ulp(got, want64):
    """``got`` (bf16) against the float64 oracle rounded to bf16: at most one bf16 step apart."""
    d = (K.bf16_ordinal(got.cpu()) - K.bf16_ordinal(want64.bfloat16())).abs()
    return d.max().item() <= 1


@pytest.mark.parametrize("P,C,c0", [(P_BIG, 128, 128), (P_BIG, 126, 1), (1, 128, 128), (1, 126, 1)])
def test_gru_backward_helpers_match_float64_oracle(cuda, P, C, c0):
    assert (P_BIG * 126) % 256 and (1 * 128) % 256  # these two end inside a 256-thread block
    t = K.gru_case(P, C)
    W = 384
    nan = float("nan")
    _, dH = _sliced(cuda, t["dH"], W, c0)
    (_, z), (_, q), (_, h), (_, r) = (_sliced(cuda, t[k], W, c0) for k in ("z", "q", "h", "r"))
    dq_buf, dq = _guarded(cuda, P, C, W, c0, torch.bfloat16, GUARD)
    dz_buf, dz = _guarded(cuda, P, C, 2 * C + 3, 0, torch.bfloat16, GUARD)  # first half of a z || r dy
    c_buf, carry = _guarded(cuda, P, C, W, c0, torch.float32, nan)
    _ops().gru_bwd_a(dH, z, q, h, dq, dz, carry)
    dq_w, dz_w, carry_w, terms = K.gru_bwd_a_oracle(t["dH"], t["z"], t["q"], t["h"])
    assert _within_one_bf16_ulp(dq, dq_w) and _within_one_bf16_ulp(dz, dz_w)
    assert ((carry.cpu().double() - carry_w).abs() <= 4 * EPS24 * terms).all()
    assert _guard_kept(dq_buf, c0, C, GUARD) and _guard_kept(dz_buf, 0, C, GUARD) and _guard_kept(c_buf, c0, C, nan)
    # saturated gates: z in {0, 1} and q = +-1 give exact zeros
    sat_z = (t["z"] == 0) | (t["z"] == 1)
    assert (dz.cpu()[sat_z] == 0).all() and (dq.cpu()[(t["q"].abs() == 1) | (t["z"] == 0)] == 0).all()

    # stage b, in place on d(rh): the oracle works on a copy taken before the call
    drh_buf, drh = _sliced(cuda, t["drh"], W, c0, fill=nan)
    _, carry_in = _sliced(cuda, t["carry"], W, c0)
    dr_buf, dr = _guarded(cuda, P, C, 2 * C + 3, C, torch.bfloat16, GUARD)  # second half of the z || r dy
    before = drh.clone()
    _ops().gru_bwd_b(drh, r, h, carry_in, dr)
    assert _same_bits(before, t["drh"])
    dr_w, dh_w, terms = K.gru_bwd_b_oracle(t["drh"], t["r"], t["h"], t["carry"])
    assert _within_one_bf16_ulp(dr, dr_w)
    assert ((drh.cpu().double() - dh_w).abs() <= 4 * EPS24 * terms).all()
    assert _guard_kept(drh_buf, c0, C, nan) and _guard_kept(dr_buf, C, C, GUARD)
    sat_r = (t["r"] == 0) | (t["r"] == 1)
    assert (dr.cpu()[sat_r] == 0).all()


def test_gru_backward_helpers_check_their_arguments(cuda):
    """Narrow operands, wrong dtypes and a wrong pixel count raise before any launch.  The narrow
    operands are views of full-width buffers: no extent passed here is ever out of bounds."""
    P, C = 4, 16
    f = lambda dt, p=P: torch.zeros(p, C, dtype=dt, device=cuda)  # noqa: E731
    f32, b16 = torch.float32, torch.bfloat16
    k = _ops()
    a = dict(dH=f(f32), z=f(b16), q=f(b16), h=f(b16), dq=f(b16), dz=f(b16), carry=f(f32))
    b = dict(drh=f(f32), r=f(b16), h=f(b16), carry=f(f32), dr=f(b16))
    k.gru_bwd_a(*a.values())
    k.gru_bwd_b(*b.values())  # the well-formed calls pass
    for op, args, first in ((k.gru_bwd_a, a, "dH"), (k.gru_bwd_b, b, "drh")):
        for name, t in args.items():
            bad = [dict(args, **{name: t.float() if t.dtype == b16 else t.bfloat16()}),  # dtype
                   dict(args, **{name: f(t.dtype, P + 1)[:P - 1]})]  # pixel count
            if name != first:
                bad.append(dict(args, **{name: t[:, :C - 1]}))  # narrower than C
            else:
                bad.append(dict(args, **{name: f(t.dtype, P + 1)}))  # more pixels than the others
            for kw in bad:
                with pytest.raises(RuntimeError, match="raft_amd"):
                    op(*kw.values())


@pytest.mark.parametrize("P", [P_BIG, 1])
@pytest.mark.parametrize("C,Cvalid,use_mask", [(128, 126, True), (128, 128, True), (128, 126, False), (72, 72, True)])
def test_masked_cast_is_bitwise(cuda, P, C, Cvalid, use_mask):
    src, mask = K.masked_cast_case(P, C, Cvalid)
    _, s = _sliced(cuda, src, 384, 256)
    _, m = _sliced(cuda, mask, 3 * C, C)
    out_buf, out = _guarded(cuda, P, C, 200, 64, torch.bfloat16, GUARD)
    _ops().masked_cast(s, m if use_mask else None, out)
    want = K.masked_cast_ref(src, mask if use_mask else None, C)
    got = out.cpu()
    assert torch.equal(got.isnan(), want.isnan())  # NaN under a positive mask stays NaN
    assert torch.equal(_bits(got)[~want.isnan()], _bits(want)[~want.isnan()])
    if Cvalid < C:
        assert (_bits(got)[:, Cvalid:] == 0).all()  # the columns past src are +0
    assert _guard_kept(out_buf, 64, C, GUARD)


@pytest.mark.parametrize("P", [P_BIG, 1])
@pytest.mark.parametrize("G,c0,Cpad,C", K.SPLIT_CASES)
def test_split_pack_is_bitwise(cuda, P, G, c0, Cpad, C):
    x = K.split_src(P, C)
    _, src = _sliced(cuda, x, C + 5, 3)
    width = K.split_width(G, c0, Cpad)
    buf, dst = _guarded(cuda, P, width, width + 9, 4, torch.bfloat16, GUARD)
    _ops().split_pack(src, dst, G, c0, Cpad)
    want = K.split_pack_ref(x, torch.full((P, width), GUARD, dtype=torch.bfloat16), G, c0, Cpad)
    assert _same_bits(dst, want)  # planes, zero padding channels and the untouched rest of the row
    assert _guard_kept(buf, 4, width, GUARD)
    hi = x.bfloat16()
    n = c0 + torch.arange(C)
    col = (n // G) * 3 * G + n % G
    got = dst.cpu()
    assert _same_bits(got[:, col], hi) and _same_bits(got[:, col + 2 * G], hi)
    assert _same_bits(got[:, col + G], (x - hi.float()).bfloat16())


@pytest.mark.parametrize("H,W", [(5, 7), (23, 31)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("from_coords", [False, True], ids=["flow", "coords"])
@pytest.mark.parametrize("with_motion", [False, True], ids=["flow8", "motion"])
def test_pack_flow_is_bitwise(cuda, H, W, dtype, from_coords, with_motion):
    B = 2
    flow = K.flow_case(B, H, W)
    flow[1, 0, 2, 3] = 70000.0  # past the fp16 range
    P = B * H * W
    flow8 = torch.full((P, 8), GUARD, dtype=dtype, device=cuda)
    mo_buf, motion = _guarded(cuda, P, 2, 128, 126, dtype, GUARD)
    mo3_buf, motion3 = _guarded(cuda, P, 3, 90, 80, dtype, GUARD)  # a wider slice: only 2 columns are written
    for buf, mo, c0 in ((mo_buf, motion, 126), (mo3_buf, motion3, 80)):
        flow8.fill_(GUARD)
        _ops().pack_flow(flow.to(cuda), flow8, mo if with_motion else None, from_coords)
        want = K.pack_flow_ref(flow, dtype, from_coords)
        assert _same_bits(flow8[:, :2], want)
        assert (_bits(flow8.cpu())[:, 2:] == 0).all()  # +0
        if with_motion:
            assert _same_bits(mo[:, :2], want) and _guard_kept(buf, c0, 2, GUARD)
        else:
            assert _guard_kept(buf, 0, 0, GUARD)


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (2, 23, 31), (1, 1, 1)])
def test_apply_delta_is_bitwise(cuda, B, H, W):
    coords1 = K.flow_case(B, H, W)
    P = B * H * W
    delta = torch.randn(P, 2, generator=torch.Generator().manual_seed(P)) * 2
    d_buf, d = _sliced(cuda, delta, 8, 3)
    out = torch.full((2, B, 2, H, W), float("nan"), device=cuda)
    _ops().apply_delta(coords1.to(cuda), d, out[0], out[1])
    want_c, want_f = K.apply_delta_ref(coords1, delta)
    assert _same_bits(out[0], want_c) and _same_bits(out[1], want_f)
    assert _guard_kept(d_buf, 3, 2, GUARD)
