"""The oracles and case builders of small_kernel_cases.py, checked on the host: each oracle against
an independent float64 formulation (autograd, the torch fallback of sequence_loss, F.instance_norm),
and each field for the classes it claims to contain."""
import pytest
import torch
import torch.nn.functional as F

import small_kernel_cases as K
from raft_ros_amd.train import loss as L


def test_gru_backward_closed_forms_match_float64_autograd():
    """h' = (1 - z) h + z q and rh = r h with z = sigmoid(a), r = sigmoid(b), q = tanh(c):
    gradients with respect to the pre-activations a, b, c and to h."""
    gen = torch.Generator().manual_seed(0)
    shape = (37, 11)
    a, b, c, h = (torch.randn(shape, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(4))
    dH, drh = (torch.randn(shape, generator=gen, dtype=torch.float64) for _ in range(2))
    z, r, q = torch.sigmoid(a), torch.sigmoid(b), torch.tanh(c)

    da, dc, carry = torch.autograd.grad((1 - z) * h + z * q, (a, c, h), dH, retain_graph=True)
    dq_o, dz_o, carry_o, _ = K.gru_bwd_a_oracle(dH, z.detach(), q.detach(), h.detach())
    tol = dict(rtol=0, atol=1e-12)
    torch.testing.assert_close(dq_o, dc, **tol)
    torch.testing.assert_close(dz_o, da, **tol)
    torch.testing.assert_close(carry_o, carry, **tol)

    db, dh_rh = torch.autograd.grad(r * h, (b, h), drh)
    dr_o, dh_o, _ = K.gru_bwd_b_oracle(drh, r.detach(), h.detach(), carry)
    torch.testing.assert_close(dr_o, db, **tol)
    torch.testing.assert_close(dh_o, carry + dh_rh, **tol)


def test_gru_case_holds_the_saturated_gates():
    for P, C in ((1, 128), (2 * 23 * 31, 126)):
        t = K.gru_case(P, C)
        assert all(v.shape == (P, C) for v in t.values())
        for name, vals in (("z", (0.0, 1.0)), ("r", (0.0, 1.0)), ("q", (1.0, -1.0))):
            for v in vals:
                assert (t[name] == v).any(), (P, C, name, v)


@pytest.mark.parametrize("name", ["maxpreds", "params", "one"])
@pytest.mark.parametrize("upstream", [1.0, 2.5])
def test_loss_oracle_matches_float64_fallback(name, upstream):
    preds, gt, valid, gamma, max_flow = K.loss_case(name)
    want = K.seq_loss_oracle(preds, gt, valid, gamma, max_flow, upstream)
    p64 = [p.double().requires_grad_(True) for p in preds]
    assert not L._fused_ok(p64, gt.double())
    # the oracle takes gamma as the op does, rounded to fp32
    loss, m = L.sequence_loss(p64, gt.double(), valid.double(), K.f32(gamma), max_flow)
    (upstream * loss).backward()
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(loss.detach(), want["loss"], **tol)
    s = want["sums"]
    cnt = s[5].clamp_min(1.0)
    for j, k in enumerate(("epe", "1px", "3px", "5px")):
        torch.testing.assert_close(m[k], s[1 + j] / cnt, **tol)
    for p, g in zip(p64, want["grads"]):
        torch.testing.assert_close(p.grad, g, **tol)


@pytest.mark.parametrize("name", sorted(K.LOSS_CASES))
def test_loss_fields_hold_every_class(name):
    B, H, W, n, _, max_flow = K.LOSS_CASES[name]
    preds, gt, valid, _, _ = K.loss_case(name)
    assert len(preds) == n and gt.shape == (B, 2, H, W) and valid.shape == (B, H, W)
    assert all(p.dtype == torch.float32 and p.is_contiguous() for p in preds + [gt, valid])
    if B * H * W < K.LOSS_CLASS_PIXELS:  # 1 x 1 x 1: one valid pixel
        assert K.loss_expected(name)["sums"][5] == B * H * W
        return
    got = K.loss_classes(preds, gt, valid, max_flow)
    assert all(got.values()), got
    HW = H * W
    if B * HW > K.LOSS_GRID_CAP:  # the same classes among the pixels of the second stride step
        def cut(t):  # (B, 2, H, W) -> (1, 2, 1, pixels from the cap on), in the kernels' flat order
            return t.reshape(B, 2, HW).permute(1, 0, 2).reshape(1, 2, 1, -1)[..., K.LOSS_GRID_CAP:]

        tail = K.loss_classes([cut(p) for p in preds], cut(gt), valid.reshape(1, 1, -1)[..., K.LOSS_GRID_CAP:],
                              max_flow)
        assert all(tail.values()), tail
    # no random pixel sits where fp32 and float64 could disagree on a comparison
    e = K.loss_expected(name)
    epe = (preds[-1].double() - gt.double()).pow(2).sum(1).sqrt()
    for t in K.EPE_STEPS:
        d = (epe - t).abs()
        assert ((d == 0) | (d >= 1e-3)).all()
    assert 0 < e["sums"][5] < B * HW


def test_stride_step_case_differs_at_one_late_pixel():
    preds, gt, valid, gamma, max_flow, (b, s) = K.stride_step_case()
    B, _, H, W = gt.shape
    assert b * H * W + s >= K.LOSS_GRID_CAP
    for p in preds:
        d = (p - gt).view(B, 2, -1)
        assert d[b, :, s].tolist() == [3.0, 4.0]
        assert d.abs().sum() == 7.0
    e = K.seq_loss_oracle(preds, gt, valid, gamma, max_flow)
    nvalid = e["sums"][5].item()
    assert e["sums"].tolist() == [7 * sum(e["weights"]), 5.0, nvalid - 1, nvalid - 1, nvalid - 1, nvalid]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(3, 24, 5, 7), (2, 8, 25, 41), (1, 8, 3, 5)])
def test_norm_oracle_matches_float64_instance_norm(shape, relu):
    x, dy = K.norm_case(shape, torch.float32)
    y, dx, mean, rstd = K.instance_norm_oracle(x, relu, 1e-5, dy)
    one = K.norm_case((2, 64, 1, 1), torch.float32)  # F.instance_norm refuses one pixel: y = dx = 0
    y1, dx1, mean1, _ = K.instance_norm_oracle(one[0], relu, 1e-5, one[1])
    assert (y1 == 0).all() and (dx1 == 0).all() and torch.equal(mean1, one[0].double()[:, :, 0, 0])
    xr = x.double().requires_grad_(True)
    yr = F.instance_norm(xr, eps=1e-5)
    if relu:
        yr = torch.relu(yr)
    (dxr,) = torch.autograd.grad(yr, xr, dy.double())
    torch.testing.assert_close(y, yr, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dx, dxr, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(mean, x.double().mean((2, 3)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rstd, (x.double().var((2, 3), unbiased=False) + 1e-5).rsqrt(), rtol=1e-12, atol=0)


def test_norm_cases_are_what_they_claim():
    x, _ = K.norm_case((2, 96, 37, 29), torch.float32)
    m, s = x.mean((2, 3)), x.std((2, 3))
    assert m.flatten().unique().numel() == m.numel() and (s.max() / s.min()) > 3  # per (n, c)
    for kind in ("mean8", "mean32", "mean100"):
        x, _ = K.norm_offset_case(kind)
        ratio = x.double().mean((2, 3)).abs() / x.double().std((2, 3))
        k = float(kind[4:])
        assert x.dtype == torch.float32 and (ratio > 0.9 * k).all() and (ratio < 1.1 * k).all()
        assert (x.mean((2, 3)) > 0).any() and (x.mean((2, 3)) < 0).any()
    x, _ = K.norm_offset_case("const")
    assert (x[:, 5] == K.f32(3.3)).all() and (x[:, 4].std() > 0)
    x, dy = K.norm_offset_case("ints_bf16")
    assert x.dtype == dy.dtype == torch.bfloat16
    assert x.min() == 96 and x.max() == 104 and (x.float() == x.float().round()).all()
    # ReLU' is decided by rounding nowhere: xhat is an exact 0 or at least KINK away from it
    cases = [K.norm_offset_case(k)[0] for k in K.NORM_OFFSETS]
    cases += [K.norm_case(s, dt)[0] for s in K.NORM_SHAPES for dt in (torch.float32, torch.bfloat16)]
    for x in cases:
        xhat = K.norm_xhat(x).abs()
        assert ((xhat == 0) | (xhat >= K.KINK)).all()
    assert (K.norm_xhat(K.norm_offset_case("const")[0])[:, 5] == 0).all()


def test_helper_cases_and_references():
    # masked_cast: every mask and src edge present, NaN and non-positive masks give +0
    src, mask = K.masked_cast_case(1, 128, 126)
    assert mask.view(torch.int16)[0, :3].tolist() == [0, -32768, 1] and mask[0, 3] < 0 and mask[0, 4].isnan()
    assert src[0, 5].isnan() and src[0, 6] == float("inf") and src[0, 7] == float("-inf")
    out = K.masked_cast_ref(src, mask, 128)
    assert out.view(torch.int16)[0, [0, 1, 3, 4, 8, 126, 127]].tolist() == [0] * 7
    assert out[0, 2] == 3.0 and out[0, 5].isnan() and out[0, 6] == float("inf") and out[0, 7] == float("-inf")
    assert torch.equal(K.masked_cast_ref(src, None, 128)[:, 9:126], src[:, 9:].bfloat16())
    # split_pack: hi + lo carries 16 bits of x; the group boundary case lands in two groups
    G, c0, Cpad, C = K.SPLIT_CASES[3]
    x = K.split_src(5, C)
    dst = torch.full((5, K.split_width(G, c0, Cpad)), 7.0, dtype=torch.bfloat16)
    out = K.split_pack_ref(x, dst, G, c0, Cpad)
    assert K.split_width(G, c0, Cpad) == 96
    assert torch.equal(out[:, 12:16], x[:, :4].bfloat16()) and torch.equal(out[:, 48:50], x[:, 4:6].bfloat16())
    assert torch.equal(out[:, 44:48], out[:, 12:16]) and (out[:, 50:52] == 0).all() and (out[:, :12] == 7).all()
    rec = out[:, 12:16].double() + out[:, 28:32].double()
    assert ((rec - x[:, :4].double()).abs() <= x[:, :4].double().abs() * 2.0 ** -16).all()
    # pack_flow / apply_delta: the grid is (x, y)
    g = K.pixel_grid(2, 5, 7)
    assert g[1, 0, 3, 6] == 6 and g[1, 1, 3, 6] == 3
    c = K.flow_case(2, 5, 7)
    assert torch.equal(K.pack_flow_ref(c, torch.float16, True).view(2, 5, 7, 2)[1, 3, 6], (c - g)[1, :, 3, 6].half())
    d = torch.randn(70, 2)
    co, fl = K.apply_delta_ref(c, d)
    assert torch.equal(co[1, :, 3, 6], c[1, :, 3, 6] + d[35 + 27]) and torch.equal(fl, co - g)
