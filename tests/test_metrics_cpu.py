"""Validation metrics without a GPU: the torch reference against an independent numpy float64
computation and the constructed classes of the threshold field, the Python layer's argument
checks, ``MetricAccumulator`` against the host loops of eval/validate.py, the DataLoader path and
the command line.
"""
import functools

import numpy as np
import pytest
import torch

import metrics_cases as mc
import raft_ros_amd.eval.validate as V
from raft_ros_amd import ops
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops.metrics import flow_metrics, flow_metrics_ref

# fp32 epe against the float64 one: du, dv (2^-24 each, doubled by the square), the squares, their
# sum, halved by the root, and the root itself: 3 * 2^-24 relative per pixel, so of the sum too
EPE_REL = 3 * 2.0 ** -24
# the host loops sum in fp32, the accumulator in float64: torch's CPU fp32 sum and mean were within
# 1.02e-7 relative of the float64 sum on random fields from 37 x 41 to 375 x 1242
LOOP_REL = 1e-5


# ---------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("with_valid", [False, True])
def test_reference_against_numpy(with_valid):
    pr, gt = mc.field(37, 41, seed=1, b=3, scales=(1.0, 0.25, 3.0))
    valid = mc.random_valid(37, 41, seed=2, b=3) if with_valid else None
    want_s, want_c, epe64 = mc.numpy_reference(pr.numpy(), gt.numpy(), None if valid is None else valid.numpy())
    # no pixel within an fp32 ulp of a threshold: the counts must then be exact
    mag64 = np.sqrt(gt[:, 0].double().numpy() ** 2 + gt[:, 1].double().numpy() ** 2)
    for t in (1.0, 3.0, 5.0):
        assert np.abs(epe64 - t).min() > 1e-5
    assert np.abs(epe64 / mag64 - 0.05).min() > 1e-6
    for top, left, hp, wp in ((0, 0, 37, 41), (1, 3, 40, 48)):
        got_s, got_c = flow_metrics_ref(mc.padded(pr, top, left, hp, wp), gt, valid, top, left)
        assert got_s.dtype == torch.float64 and got_c.dtype == torch.int32 and got_c.shape == (3, 5)
        assert np.array_equal(got_c.numpy(), want_c)
        rel = np.abs(got_s.numpy() - want_s) / want_s
        print("rel err of epe_sum against float64:", rel)
        assert (rel <= EPE_REL).all()
        # and against numpy's fp32 steps (its sqrt is correctly rounded): the same terms, so within REL
        p, g = pr.numpy(), gt.numpy()
        du, dv = p[:, 0] - g[:, 0], p[:, 1] - g[:, 1]
        epe32 = np.sqrt(du * du + dv * dv)
        assert epe32.dtype == np.float32
        steps = np.where(True if valid is None else valid.numpy() >= 0.5, epe32.astype(np.float64), 0.0).sum(axis=(1, 2))
        assert (np.abs(got_s.numpy() - steps) <= mc.REL * steps).all(), np.abs(got_s.numpy() - steps) / steps
        assert all(0 < got_c[b, k] < got_c[b, 0] for b in range(3) for k in range(1, 5))  # every count is exercised


@pytest.mark.parametrize("w", [8, 5])
def test_reference_threshold_classes(w):
    pr, gt, valid, want = mc.threshold_batch(w)
    s, c = flow_metrics_ref(pr, gt, valid)
    for k, (pix, cls) in enumerate(mc.THRESHOLD_PIXELS):
        assert c[k].tolist() == list(cls), (k, pix, c[k].tolist())
    assert torch.equal(c, want)
    pr, gt, valid, want = mc.threshold_field(w)
    assert torch.equal(flow_metrics_ref(pr, gt, valid)[1], want)


def test_reference_nonfinite_and_rounding():
    clean, bad, gt, valid = mc.nonfinite_fields(counted=False)
    a, b = flow_metrics_ref(clean, gt, valid), flow_metrics_ref(bad, gt, valid)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])  # a select: uncounted NaN / inf are dropped
    clean, bad, gt, valid = mc.nonfinite_fields(counted=True)
    s, c = flow_metrics_ref(bad, gt, valid)
    assert torch.isnan(s).all() and c[0, 0] == flow_metrics_ref(clean, gt, valid)[1][0, 0]
    pr, gt, valid, want = mc.single_pixel_batch()
    s, c = flow_metrics_ref(pr, gt, valid)
    assert torch.equal(s, want) and (c[:, 0] == 1).all()
    s, c = flow_metrics_ref(pr, gt, torch.zeros_like(valid))
    assert (s == 0).all() and (c == 0).all()


# ---------------------------------------------------------------------------- the Python layer
def test_wrapper_shapes_and_cpu_path():
    pr, gt = mc.field(37, 41, seed=1, b=3)
    valid = mc.random_valid(37, 41, seed=2, b=3)
    want = flow_metrics_ref(pr, gt, valid)
    got = flow_metrics(pr, gt, valid)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    got = flow_metrics(mc.padded(pr, 1, 3, 40, 48), gt, valid, padder=mc.Padder(1, 3, 2, 4))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    one = flow_metrics(pr[1], gt[1], valid[1])  # (2, H, W) in: B dropped
    assert one[0].shape == () and one[1].shape == (5,)
    assert one[0] == want[0][1] and torch.equal(one[1], want[1][1])
    from raft_ros_amd.utils.utils import InputPadder

    p = InputPadder((1, 3, 37, 41))
    assert (p._pad[2], p._pad[0]) == (1, 3)
    got = flow_metrics(p.pad(pr)[0], gt, valid, padder=p)  # replicate padding: the border is not read
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # half and non-contiguous inputs are converted
    h = flow_metrics(pr.half(), gt.half())
    w = flow_metrics_ref(pr.half().float(), gt.half().float())
    assert torch.equal(h[0], w[0]) and torch.equal(h[1], w[1])
    wide = torch.zeros(3, 2, 37, 82)
    wide[..., ::2] = pr
    got = flow_metrics(wide[..., ::2], gt, valid)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    empty = flow_metrics(torch.zeros(0, 2, 4, 4), torch.zeros(0, 2, 4, 4))
    assert empty[0].shape == (0,) and empty[0].dtype == torch.float64 and empty[1].shape == (0, 5)
    empty = flow_metrics(torch.zeros(2, 2, 0, 4), torch.zeros(2, 2, 0, 4))
    assert empty[0].tolist() == [0.0, 0.0] and empty[1].tolist() == [[0] * 5] * 2
    assert ops.flow_metrics is flow_metrics and ops.flow_metrics_ref is flow_metrics_ref


def test_wrapper_errors():
    f, v = torch.zeros(2, 5, 7), torch.ones(5, 7)
    for bad in ((torch.zeros(3, 5, 7), f), (f, torch.zeros(5, 7)), (f, torch.zeros(1, 2, 5, 7)), (f.long(), f),
                (f, f.to(torch.uint8)), (f.numpy(), f), (torch.zeros(2, 2, 5, 7), torch.zeros(3, 2, 5, 7)),
                (torch.zeros(2, 8, 8), f),               # a larger prediction without a padder
                (f, f, torch.ones(5, 8)), (f, f, v[None]), (f, f, v.numpy())):
        with pytest.raises(ValueError):
            flow_metrics(*bad)
    with pytest.raises(ValueError):  # the crop leaves the prediction
        flow_metrics(torch.zeros(2, 8, 8), f, padder=mc.Padder(4, 0))
    with pytest.raises(ValueError):
        flow_metrics(torch.zeros(2, 8, 8), f, padder=mc.Padder(0, 2))


@pytest.mark.skipif(not _ext.is_loaded(), reason=f"native library not built: {_ext.load_error()}")
def test_fake_kernel_shapes_and_dtypes():
    pr, gt = torch.empty(3, 2, 24, 24, device="meta"), torch.empty(3, 2, 17, 23, device="meta")
    for valid in (None, torch.empty(3, 17, 23, device="meta")):
        s, c = _ext.ops().flow_metrics(pr, gt, valid, 2, 1)
        assert s.shape == (3,) and s.dtype == torch.float64 and s.device.type == "meta"
        assert c.shape == (3, 5) and c.dtype == torch.int32


# ---------------------------------------------------------------------------- the consumers
def test_accumulator_totals():
    pr, gt = mc.field(9, 13, seed=3, b=4)
    valid = mc.random_valid(9, 13, seed=4, b=4)
    valid[3] = 0.0  # an image without a counted pixel: its mean is NaN
    s, c = flow_metrics_ref(pr, gt, valid)
    acc = V.MetricAccumulator(torch.device("cpu"))
    acc.update(pr[:2], gt[:2], valid[:2])
    acc.update(pr[2], gt[2], valid[2])  # the unbatched form
    r = acc.result()
    assert r["images"] == 3 and r["counts"] == c[:3].sum(0).tolist()
    assert r["epe_sum"] == pytest.approx(s[:3].sum().item(), rel=1e-14)
    assert r["mean_sum"] == pytest.approx((s[:3] / c[:3, 0]).sum().item(), rel=1e-14)
    assert r["epe"] == r["epe_sum"] / r["counts"][0] and r["f1"] == 100 * r["counts"][4] / r["counts"][0]
    acc.update(pr[3], gt[3], valid[3])
    r = acc.result()
    assert r["images"] == 4 and np.isnan(r["mean-epe"]) and r["counts"] == c.sum(0).tolist()


@functools.lru_cache(maxsize=None)
def _host_loop(case):
    """The host loop (the switch off) over the in-memory samples, computed once."""
    return V.evaluate_samples(mc.case_model(case), mc.samples(case), mc.SAMPLE_CASES[case][0], iters=2)


def _compare(kind, off, on):
    print(kind, "off", off, "on", on)
    assert set(off) == set(on)
    exact = ("1px", "3px", "5px") if kind == "sintel" else ("kitti-f1",)
    for k in exact:  # the same predictions, the same integers
        assert on[k] == off[k], k
    for k in set(off) - set(exact):
        assert abs(on[k] - off[k]) <= LOOP_REL * abs(off[k]), k


@pytest.mark.parametrize("case", list(mc.SAMPLE_CASES))
def test_accumulator_against_the_host_loop(case):
    kind = mc.SAMPLE_CASES[case][0]
    off = _host_loop(case)
    on = V.evaluate_samples(mc.case_model(case), mc.samples(case), kind, iters=2, device_metrics=True)
    _compare(kind, off, on)
    assert 0 < (off["1px"] if kind == "sintel" else off["kitti-f1"]) < 100


def test_shards_add_up_to_the_whole():
    """Two ranks' accumulators summed (what the all-reduce does) against one rank's."""
    case = "kitti-36x50"
    model, samples = mc.case_model(case), mc.samples(case)
    whole = V.evaluate_samples(model, samples, "kitti", iters=2, device_metrics=True)
    parts = []
    for rank in (0, 1):
        acc = V.MetricAccumulator(torch.device("cpu"))
        with torch.inference_mode():
            for i1, i2, gt, va in (samples[i] for i in range(rank, 3, 2)):
                p = V.InputPadder(i1[None].shape, mode="kitti")
                _, flow_pr = model(*p.pad(i1[None], i2[None]), iters=2, test_mode=True)
                acc.update(flow_pr, gt[None], va[None], p)
        parts.append(acc.result())
    assert parts[0]["images"] + parts[1]["images"] == 3
    f1 = 100 * (parts[0]["counts"][4] + parts[1]["counts"][4]) / (parts[0]["counts"][0] + parts[1]["counts"][0])
    assert f1 == whole["kitti-f1"]
    epe = (parts[0]["mean_sum"] + parts[1]["mean_sum"]) / 3
    assert epe == pytest.approx(whole["kitti-epe"], rel=1e-14)


def test_result_all_reduces_under_a_process_group(tmp_path):
    """``result(world > 1)`` hands one float64 tensor to the all-reduce (a one-rank gloo group: the
    sum over its ranks is the rank's own totals)."""
    import torch.distributed as dist

    pr, gt = mc.field(9, 13, seed=3, b=2)
    acc = V.MetricAccumulator(torch.device("cpu"))
    acc.update(pr, gt)
    alone = acc.result()
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        assert acc.result(world=2) == alone
    finally:
        dist.destroy_process_group()


def test_chairs_kind_and_plain_iterables():
    model = mc.case_model("sintel-37x41")
    shaped = [(i1[:, :32, :40], i2[:, :32, :40], gt[:, :32, :40], va[:32, :40]) for i1, i2, gt, va in
              mc.samples("sintel-37x41")]
    off = V.evaluate_samples(model, shaped, "chairs", iters=2)
    on = V.evaluate_samples(model, iter(shaped), "chairs", iters=2, device_metrics=True)  # an iterator: no len()
    assert set(off) == set(on) == {"epe"} and abs(on["epe"] - off["epe"]) <= LOOP_REL * off["epe"]
    with pytest.raises(ValueError):
        V.evaluate_samples(model, shaped, "things", iters=2)


@pytest.mark.parametrize("case", ["kitti-36x50", "sintel-37x41"])
def test_workers_give_the_same_result(case):
    kind, model, samples = mc.SAMPLE_CASES[case][0], mc.case_model(case), mc.samples(case)
    one = V.evaluate_samples(model, samples, kind, iters=2, device_metrics=True)
    two = V.evaluate_samples(model, samples, kind, iters=2, device_metrics=True, workers=2)
    assert one == two
    assert V.evaluate_samples(model, samples, kind, iters=2, workers=2) == _host_loop(case)


def test_validate_synthetic_switch(capsys):
    model = mc.small_model()
    off = V.validate_synthetic(model, iters=2, n_pairs=3, size=(128, 128))
    line_off = capsys.readouterr().out
    on = V.validate_synthetic(model, iters=2, n_pairs=3, size=(128, 128), device_metrics=True)
    line_on = capsys.readouterr().out
    assert line_off.startswith("Validation (synthetic) EPE: ") and line_on.startswith("Validation (synthetic) EPE: ")
    for k in ("synthetic-1px", "synthetic-3px", "synthetic-5px"):
        assert on[k] == off[k]
    assert abs(on["synthetic-epe"] - off["synthetic-epe"]) <= LOOP_REL * off["synthetic-epe"]
    res = V.run_validation(model, [], device_metrics=True, workers=0)
    assert res == {}


def test_evaluate_cli_device_metrics(tmp_path, monkeypatch, capsys):
    import evaluate
    import train
    from raft_ros_amd.utils import checkpoint

    ck = str(tmp_path / "m.pth")
    checkpoint.save_weights(mc.small_model(), ck)
    seen = {}

    def small_synthetic(model, **kw):  # the command line's keywords on a short run
        seen.update(kw)
        return V.validate_synthetic(model, n_pairs=2, size=(128, 128), **kw)

    monkeypatch.setattr(evaluate, "validate_synthetic", small_synthetic)
    base = ["--model", ck, "--small", "--dataset", "synthetic", "--device", "cpu", "--iters", "1"]
    off = evaluate.main(base)
    assert "device_metrics" not in seen
    on = evaluate.main(base + ["--device_metrics", "--val_workers", "2"])
    assert seen["device_metrics"] is True and seen["workers"] == 2
    assert on["synthetic-1px"] == off["synthetic-1px"] and on["synthetic-epe"] >= 0
    assert capsys.readouterr().out.count("Validation (synthetic) EPE: ") == 2
    args = train.build_parser().parse_args(["--stage", "chairs", "--device_metrics"])
    assert args.device_metrics is True
    assert train.build_parser().parse_args(["--stage", "chairs"]).device_metrics is False
