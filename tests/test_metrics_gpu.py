"""Validation metrics on the GPU: the HIP op on device copies against the torch reference on the
host tensors (``counts`` exactly, ``epe_sum`` within 1e-12 relative: both sides sum identical fp32
terms in float64 and differ only in association), the constructed classes of the threshold field,
bitwise per-pixel rounding, independence of the batch, graph capture, and the validators with the
metrics kept on the device.
"""
import pytest
import torch

import metrics_cases as mc
import raft_ros_amd.eval.validate as V
from raft_ros_amd.ops.metrics import flow_metrics, flow_metrics_ref

pytestmark = pytest.mark.gpu

LOOP_REL = 1e-5  # the host loops sum in fp32 (within 1.02e-7 of the float64 sum as measured): two orders of margin


def _run(pr, gt, valid, dev, top=0, left=0, what=""):
    """Host tensors (B, ...) -> the op's results on the host, checked against the reference."""
    padder = mc.Padder(top, left) if (top or left or pr.shape[-2:] != gt.shape[-2:]) else None
    got = flow_metrics(pr.to(dev), gt.to(dev), None if valid is None else valid.to(dev), padder)
    assert all(g.device.type == "cuda" for g in got)
    assert got[0].shape == (gt.shape[0],) and got[1].shape == (gt.shape[0], 5)
    mc.check(got, flow_metrics_ref(pr, gt, valid, top, left), what)
    return [g.cpu() for g in got]


@pytest.mark.parametrize("with_valid", [False, True])
def test_crop_and_scalar_path(cuda, with_valid):
    """37 x 41 inside 40 x 48 at (1, 3), 1e6 around it: a read outside the crop shows."""
    pr, gt = mc.field(37, 41, seed=1)
    valid = mc.random_valid(37, 41, seed=2) if with_valid else None
    s, c = _run(mc.padded(pr, 1, 3, 40, 48), gt, valid, cuda, 1, 3, what="37x41 in 40x48")
    assert s[0] < 37 * 41 * 100.0 and 0 < c[0, 1] < c[0, 2] < c[0, 3] < c[0, 0] and c[0, 4] > 0
    flat = _run(pr, gt, valid, cuda, what="37x41 unpadded")
    assert torch.equal(flat[0], s) and torch.equal(flat[1], c)  # where the crop lies does not matter


@pytest.mark.parametrize("case", ["all-vector", "gt-vector", "aligned-crop"])
def test_vector_paths(cuda, case):
    h, w, top, left, hp, wp = {"all-vector": (8, 16, 0, 0, 8, 16), "gt-vector": (6, 12, 1, 2, 8, 16),
                               "aligned-crop": (8, 16, 0, 4, 8, 24)}[case]
    pr, gt = mc.field(h, w, seed=3, b=3, scales=(1.0, 0.25, 3.0))
    for valid in (None, mc.random_valid(h, w, seed=4, b=3)):
        _run(mc.padded(pr, top, left, hp, wp), gt, valid, cuda, top, left, what=f"{case} valid={valid is not None}")


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 3), (33, 32), (260, 256)])
def test_tails_and_partials(cuda, shape):
    """(33, 32): just over one block per image; (260, 256): 65 partials, more than a wave of them."""
    h, w = shape
    pr, gt = mc.field(h, w, seed=5, b=2, scales=(1.0, 2.0))
    _run(pr, gt, None, cuda, what=f"{shape}")
    _run(pr, gt, mc.random_valid(h, w, seed=6, b=2), cuda, what=f"{shape} valid")


@pytest.mark.parametrize("w", [8, 5])
def test_threshold_classes(cuda, w):
    pr, gt, valid, want = mc.threshold_batch(w)
    _, c = _run(pr, gt, valid, cuda, what=f"threshold pixels, width {w}")
    for k, (pix, cls) in enumerate(mc.THRESHOLD_PIXELS):
        assert c[k].tolist() == list(cls), (k, pix, c[k].tolist())
    pr, gt, valid, want = mc.threshold_field(w)
    _, c = _run(pr, gt, valid, cuda, what=f"threshold field, width {w}")
    assert torch.equal(c, want)


def test_nonfinite_values(cuda):
    clean, bad, gt, valid = mc.nonfinite_fields(counted=True)
    s, c = _run(bad, gt, valid, cuda, what="NaN / inf at counted pixels")
    assert torch.isnan(s).all()
    for sign, val in ((1.0, float("inf")), (-1.0, float("-inf"))):  # an infinite error alone: the sum is +inf
        one = clean.clone()
        one[0, 1, 4, 5] = val
        s, _ = _run(one, gt, valid, cuda, what=f"{val} at a counted pixel")
        assert s[0] == float("inf")
    clean, bad, gt, valid = mc.nonfinite_fields(counted=False)
    a = _run(clean, gt, valid, cuda, what="clean")
    b = _run(bad, gt, valid, cuda, what="NaN / inf at uncounted pixels")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    nan_valid = valid.clone()
    nan_valid[0, 0, 0] = float("nan")  # a NaN valid is not >= 0.5
    _run(clean, gt, nan_valid, cuda, what="NaN in valid")


def test_per_pixel_rounding(cuda):
    """One counted pixel per image: the sum is that pixel's fp32 epe, bit for bit (sqrtf, the order
    of the subtraction, contraction off)."""
    pr, gt, valid, want = mc.single_pixel_batch()
    s, c = _run(pr, gt, valid, cuda, what="64 single pixels")
    assert torch.equal(s, want), (s - want).abs().max().item()
    assert (c[:, 0] == 1).all()


def test_independence_and_determinism(cuda):
    pr, gt = mc.field(37, 41, seed=7, b=3, scales=(1.0, 0.25, 3.0))
    valid = mc.random_valid(37, 41, seed=8, b=3)
    valid[1] = 0.0  # an image without a counted pixel
    frame = mc.padded(pr, 1, 3, 40, 48)
    s, c = _run(frame, gt, valid, cuda, 1, 3, what="B=3")
    assert s[1] == 0.0 and (c[1] == 0).all() and c[0, 0] > 0
    d = [t.to(cuda) for t in (frame, gt, valid)]
    again = flow_metrics(*d, mc.Padder(1, 3))
    assert torch.equal(again[0].cpu(), s) and torch.equal(again[1].cpu(), c)
    for b in range(3):  # an image of a batch is that image alone, the sum included
        one = flow_metrics(d[0][b], d[1][b], d[2][b], mc.Padder(1, 3))
        assert one[0].shape == () and one[1].shape == (5,)
        assert one[0].cpu() == s[b] and torch.equal(one[1].cpu(), c[b])
    pr, gt = mc.field(260, 256, seed=9, b=3)  # several partials per image
    d = [t.to(cuda) for t in (pr, gt)]
    whole = flow_metrics(*d)
    for b in range(3):
        one = flow_metrics(d[0][b:b + 1], d[1][b:b + 1])
        assert torch.equal(one[0], whole[0][b:b + 1]) and torch.equal(one[1], whole[1][b:b + 1])


def test_graph_capture(cuda):
    pr, gt = mc.field(37, 41, seed=10, b=2)
    valid = mc.random_valid(37, 41, seed=11, b=2)
    d = [t.to(cuda) for t in (mc.padded(pr, 1, 3, 40, 48), gt, valid)]
    padder = mc.Padder(1, 3)
    eager = flow_metrics(*d, padder)
    static = [torch.zeros_like(t) for t in d]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flow_metrics(*static, padder)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = flow_metrics(*static, padder)
    for s, t in zip(static, d):
        s.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])
    graph.replay()  # nothing accumulates between replays
    torch.cuda.synchronize()
    assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])


def test_op_argument_checks(cuda):
    op = torch.ops.raft_amd.flow_metrics
    pr, gt, va = torch.zeros(1, 2, 8, 8, device=cuda), torch.zeros(1, 2, 4, 8, device=cuda), torch.ones(1, 4, 8, device=cuda)
    for bad in ((pr.half(), gt, None, 0, 0), (pr, gt.half(), None, 0, 0), (pr, gt, va.half(), 0, 0),
                (pr, gt, va[:, :, :4], 0, 0), (pr, gt, va[0], 0, 0), (pr, gt, None, 5, 0), (pr, gt, None, 0, 1),
                (pr, gt, None, -1, 0), (pr[..., ::2], gt[..., ::2], None, 0, 0), (pr, gt.cpu(), None, 0, 0),
                (pr, gt, va.cpu(), 0, 0), (pr.cpu(), gt.cpu(), None, 0, 0), (pr, torch.zeros(2, 2, 4, 8, device=cuda), None, 0, 0),
                (torch.zeros(1, 3, 8, 8, device=cuda), gt, None, 0, 0)):
        with pytest.raises(RuntimeError):
            op(*bad)
    s, c = op(pr, gt, va, 4, 0)  # the crop may touch the frame's edge
    assert s.tolist() == [0.0] and c.tolist() == [[32, 32, 32, 32, 0]]
    s, c = op(torch.zeros(0, 2, 8, 8, device=cuda), torch.zeros(0, 2, 4, 8, device=cuda), None, 0, 0)
    assert s.shape == (0,) and s.dtype == torch.float64 and c.shape == (0, 5) and c.dtype == torch.int32
    s, c = op(torch.zeros(2, 2, 8, 8, device=cuda), torch.zeros(2, 2, 0, 8, device=cuda), None, 0, 0)
    assert s.tolist() == [0.0, 0.0] and c.tolist() == [[0] * 5] * 2


# ---------------------------------------------------------------------------- the validators
def _compare(off, on, exact):
    print("off", off, "on", on)
    assert set(off) == set(on)
    for k in exact:  # the same predictions, the same integers
        assert on[k] == off[k], k
    for k in set(off) - set(exact):
        assert abs(on[k] - off[k]) <= LOOP_REL * abs(off[k]), k


def test_validate_synthetic_on_the_device(cuda):
    model = mc.small_model(cuda)
    off = V.validate_synthetic(model, iters=2, n_pairs=3, size=(128, 128))
    with mc.Readbacks() as rb:
        orig = V.MetricAccumulator.result
        before = []
        V.MetricAccumulator.result = lambda self, world=1: (before.append(rb.count), orig(self, world))[1]
        try:
            on = V.validate_synthetic(model, iters=2, n_pairs=3, size=(128, 128), device_metrics=True)
        finally:
            V.MetricAccumulator.result = orig
    assert before == [0] and rb.count == 1  # nothing is read back before result(), which reads once
    _compare(off, on, ("synthetic-1px", "synthetic-3px", "synthetic-5px"))


@pytest.mark.parametrize("case", list(mc.SAMPLE_CASES))
def test_validator_over_in_memory_samples(cuda, case):
    kind = mc.SAMPLE_CASES[case][0]
    model, samples = mc.case_model(case, cuda), mc.samples(case)
    off = V.evaluate_samples(model, samples, kind, iters=2)
    with mc.Readbacks() as rb:
        orig = V.MetricAccumulator.result
        before = []
        V.MetricAccumulator.result = lambda self, world=1: (before.append(rb.count), orig(self, world))[1]
        try:
            on = V.evaluate_samples(model, samples, kind, iters=2, device_metrics=True)
        finally:
            V.MetricAccumulator.result = orig
    assert before == [0] and rb.count == 1
    _compare(off, on, ("1px", "3px", "5px") if kind == "sintel" else ("kitti-f1",))
