"""Working-resolution inference without a GPU: the two torch references against independent
oracles (frame_scale_cases.py), the Python layer, the fake kernels and the consumers
(FlowInference(scale=D), the ROS node with fakes, demo.py --scale)."""
import csv
import os
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import frame_io_cases as fc
import frame_scale_cases as sc
from raft_ros_amd import ops
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops.frame_scale import (ingest_frames_scaled, ingest_frames_scaled_ref, scaled_shape, upscale_flow,
                                          upscale_flow_ref)
from raft_ros_amd.ops.track import seed_points, track_points_ref
from raft_ros_amd.ros.node import FlowInference, RaftRosNode
from raft_ros_amd.utils.utils import InputPadder
from test_ros_cpu import FakeBridge, FakeRospy, Msg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- downscale reference
@pytest.mark.parametrize("pads", sc.PADS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape,D", sc.CPU_SHAPES)
def test_downscale_reference_is_the_per_cell_loop(shape, D, n, pads):
    fr, got = sc.down_case(shape, D, n, pads)
    h, w = sc.ceil_div(shape[0], D), sc.ceil_div(shape[1], D)
    assert got.dtype == torch.float32 and got.shape == (n, 3, h + pads[2] + pads[3], w + pads[0] + pads[1])
    assert torch.equal(got, sc.down_loop_oracle(fr, D, pads))
    # cv2's INTER_AREA for integer factors: the pooling with partial windows divided by their own size
    pool = F.avg_pool2d(fr.permute(0, 3, 1, 2).float(), D, ceil_mode=True, count_include_pad=False)
    assert torch.equal(got, F.pad(pool, list(pads), mode="replicate"))


def test_downscale_whole_image_in_one_partial_cell():
    fr, got = sc.down_case((5, 3), 8, 1, (0, 0, 0, 0))
    assert got.shape == (1, 3, 1, 1)
    want = (fr.double().sum(dim=(1, 2)) / 15).float()
    assert torch.equal(got[:, :, 0, 0], want)


@pytest.mark.parametrize("pads", sc.PADS + ((3, 4, 1, 2),))
def test_downscale_by_one_is_ingest(pads):
    fr = sc.frames(2, 13, 17, seed=5)
    assert torch.equal(ingest_frames_scaled_ref(fr, 1, pads), fc.pad_ref(fr, pads))
    out, padder = ingest_frames_scaled(fr, 1)
    assert torch.equal(out, ops.ingest_frames(fr)[0]) and tuple(padder._pad) == (3, 4, 1, 2)


def test_fp32_division_is_the_rounded_quotient():
    """Every (sum, count) the op can meet: the fp32 division of the exact integers is the float64
    quotient rounded to fp32."""
    sums = torch.arange(0, 64 * 255 + 1, dtype=torch.int32)[:, None]
    counts = torch.arange(1, 65, dtype=torch.int32)[None, :]
    got = sums.float() / counts.float()
    assert torch.equal(got, (sums.double() / counts.double()).float())


# ---------------------------------------------------------------------------- upscale reference
TINY = (((5, 7), 2), ((5, 7), 3), ((4, 6), 4), ((5, 3), 8), ((9, 13), 5), ((6, 5), 1))


@pytest.mark.parametrize("pads", sc.PADS)
@pytest.mark.parametrize("shape,D", TINY)
def test_upscale_reference_is_the_per_pixel_loop(shape, D, pads):
    hp, wp, left, top, w, h = sc.low_geometry(shape, D, pads)
    flow = sc.gaussian_flow(2, hp, wp, seed=D)
    geo = (D, left, top, w, h, shape[0], shape[1])
    got = upscale_flow_ref(flow, *geo)
    assert got.dtype == torch.float32 and got.shape == (2, 2) + shape and got.is_contiguous()
    assert sc.same(got, sc.up_loop_oracle(flow, *geo))


@pytest.mark.parametrize("shape,D", [((5, 7), 2), ((9, 13), 3), ((9, 13), 5)])
def test_upscale_nonfinite_entries_follow_the_sequence(shape, D):
    """NaN and +-inf propagate as the line-by-line sequence dictates: a tap of weight zero still
    enters through ``fx * (a01 - a00)``, an inf minus an inf is a NaN."""
    hp, wp, left, top, w, h = sc.low_geometry(shape, D, (1, 2, 3, 0))
    flow = sc.gaussian_flow(1, hp, wp, seed=11)
    flow[0, 0, top, left] = float("nan")
    flow[0, 1, top + h - 1, left + w - 1] = float("inf")
    flow[0, 0, top + h // 2, left + w // 2] = float("-inf")
    flow[0, 1, top + h // 2, left + 1] = float("inf")
    flow[0, 1, top + h // 2, left + 2] = float("inf")
    flow[:, :, :top] = float("nan")  # the padding is never read
    flow[:, :, :, :left] = float("nan")
    flow[:, :, :, left + w:] = float("nan")
    geo = (D, left, top, w, h, shape[0], shape[1])
    got, want = upscale_flow_ref(flow, *geo), sc.up_loop_oracle(flow, *geo)
    assert sc.same(got, want)
    assert want.isnan().any() and want.isinf().any() and want.isfinite().any()


FLOAT64_SHAPES = sc.CPU_SHAPES + (((33, 70), 8), ((6, 1920), 3), ((6, 999), 5), ((6, 999), 2))


@pytest.mark.parametrize("pads", sc.PADS)
@pytest.mark.parametrize("shape,D", FLOAT64_SHAPES)
def test_upscale_reference_against_float64(shape, D, pads):
    flow, geo, got = sc.up_case(shape, D, 2, pads)
    want = sc.up_float64(flow, *geo)
    _, left, top, w, h = geo[:5]
    err, bound = float((got.double() - want).abs().max()), sc.up_bound(D, flow[:, :, top:top + h, left:left + w])
    print(f"{shape} D={D} pads={pads}: max |ref - float64| {err:.3g}, bound {bound:.3g} ({err / bound:.3f} of it)")
    assert err <= bound


@pytest.mark.parametrize("pads", sc.PADS)
@pytest.mark.parametrize("shape,D,coef", [
    ((37, 41), 2, sc.AFFINE), ((16, 24), 4, sc.AFFINE), ((33, 70), 8, sc.AFFINE),
    ((37, 41), 3, sc.AFFINE), ((9, 13), 5, sc.AFFINE_ODD), ((37, 41), 2, sc.AFFINE_ODD), ((6, 1920), 3, sc.AFFINE_ODD),
])
def test_upscale_of_an_affine_field_is_the_affine_map(shape, D, coef, pads):
    """Independent of the oracle's formula: bilinear sampling reproduces an affine field, so the
    output is D times the field at the output pixel's centre in low-resolution coordinates."""
    hp, wp, left, top, w, h = sc.low_geometry(shape, D, pads)
    flow = sc.affine_low(hp, wp, left, top, coef)
    H, W = shape
    got = upscale_flow_ref(flow, D, left, top, w, h, H, W)
    want, inside = sc.affine_expected(D, w, h, H, W, coef)
    assert inside.any() and not inside.all()
    err = float((got.double() - want)[:, :, inside].abs().max())
    bound = sc.up_bound(D, flow[:, :, top:top + h, left:left + w])
    print(f"{shape} D={D}: max |ref - affine| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    if coef is sc.AFFINE and D in (2, 4, 8):  # dyadic coefficients and weights: every step is exact
        assert err == 0.0


@pytest.mark.parametrize("pads,mode", [((3, 4, 1, 2), "sintel"), ((3, 4, 0, 3), "kitti")])
def test_upscale_by_one_is_unpad(pads, mode):
    padder = InputPadder((2, 3, 13, 17), mode=mode)
    assert tuple(padder._pad) == pads
    flow = sc.gaussian_flow(2, 16, 24, seed=3)
    want = padder.unpad(flow)
    assert torch.equal(upscale_flow_ref(flow, 1, pads[0], pads[2], 17, 13, 13, 17), want)
    assert torch.equal(upscale_flow(flow, padder, 1, (13, 17)), want)


@pytest.mark.parametrize("shape,D", [((1, 12), 3), ((12, 1), 4), ((1, 1), 2), ((3, 9), 3), ((8, 2), 2)])
def test_upscale_of_single_rows_and_columns(shape, D):
    """h = 1 and / or w = 1: every weight along that axis is zero, the one sample is repeated."""
    H, W = shape
    hp, wp, left, top, w, h = sc.low_geometry(shape, D, (1, 2, 3, 0))
    flow = sc.gaussian_flow(1, hp, wp, seed=2)
    geo = (D, left, top, w, h, H, W)
    got = upscale_flow_ref(flow, *geo)
    assert sc.same(got, sc.up_loop_oracle(flow, *geo))
    img = flow[:, :, top:top + h, left:left + w]
    if h == 1:
        assert torch.equal(got, got[:, :, 0:1].expand_as(got))
    if w == 1:
        assert torch.equal(got, got[:, :, :, 0:1].expand_as(got))
    if h == 1 and w == 1:
        assert torch.equal(got, (img * D).expand_as(got))


@pytest.mark.parametrize("D", [2, 3, 4, 5, 8])
def test_upscale_is_interpolates_convention(D):
    """The loose check: ``F.interpolate(align_corners=False)`` times D is the same convention with
    fp32 source coordinates.  Its weight is off by at most ~4 * 2^-24 * n per axis (the coordinate
    ``(x + 0.5) / D - 0.5 < n`` after three roundings and a rounded ``1 / D``), each times a
    difference of neighbours <= 2 max|flow|, times D, beside this op's own bound; a wrong convention
    (corners aligned, a half-pixel shift) is off by a fraction of sigma."""
    h, w = 12, 20
    flow = sc.gaussian_flow(2, h, w, sigma=5.0, seed=D)
    got = upscale_flow_ref(flow, D, 0, 0, w, h, h * D, w * D)
    want = F.interpolate(flow, scale_factor=D, mode="bilinear", align_corners=False) * D
    err = float((got - want).abs().max())
    tol = 2.0 ** -24 * D * float(flow.abs().max()) * (16 + 16 * max(h, w))
    print(f"D={D}: max |ref - F.interpolate * D| {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol < 0.05 * 5.0


# ---------------------------------------------------------------------------- the Python layer
def test_scaled_shape_and_exports():
    assert scaled_shape(1080, 1920, 2) == (540, 960) and scaled_shape(37, 41, 3) == (13, 14)
    assert scaled_shape(5, 3, 8) == (1, 1) and scaled_shape(7, 9, 1) == (7, 9)
    assert ops.ingest_frames_scaled is ingest_frames_scaled and ops.upscale_flow is upscale_flow
    assert ops.ingest_frames_scaled_ref is ingest_frames_scaled_ref and ops.upscale_flow_ref is upscale_flow_ref
    assert ops.scaled_shape is scaled_shape


def test_wrappers_on_the_cpu():
    fr = sc.frames(2, 37, 41, seed=1)
    out, padder = ingest_frames_scaled(fr, 3)
    assert (padder.ht, padder.wd) == (13, 14) and tuple(padder._pad) == (1, 1, 1, 2) and out.shape == (2, 3, 16, 16)
    assert torch.equal(out, ingest_frames_scaled_ref(fr, 3, (1, 1, 1, 2)))
    assert torch.equal(ingest_frames_scaled(list(fr.numpy()), 3)[0], out)  # a list of arrays
    assert tuple(ingest_frames_scaled(fr, 3, mode="kitti")[1]._pad) == (1, 1, 0, 3)
    flow = sc.gaussian_flow(2, 16, 16, seed=2)
    up = upscale_flow(flow, padder, 3, (37, 41))
    assert up.shape == (2, 2, 37, 41) and torch.equal(up, upscale_flow_ref(flow, 3, 1, 1, 14, 13, 37, 41))
    assert torch.equal(upscale_flow(flow.double(), padder, 3, (37, 41)), up)  # converted like the siblings
    assert torch.equal(upscale_flow(flow, padder, 3, (38, 42)), upscale_flow_ref(flow, 3, 1, 1, 14, 13, 38, 42))
    assert ingest_frames_scaled(sc.frames(0, 8, 8), 2)[0].shape == (0, 3, 8, 8)


def test_wrappers_reject_bad_input():
    fr = sc.frames(1, 16, 16)
    for bad in (fr.float(), fr[0], fr[..., :2], torch.zeros(1, 0, 4, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ingest_frames_scaled(bad, 2)
    for D in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            ingest_frames_scaled(fr, D)
    with pytest.raises(ValueError):
        ingest_frames_scaled([], 2)
    with pytest.raises(ValueError):
        ingest_frames_scaled([fr[0].numpy(), fr[0, :8].numpy()], 2)
    _, padder = ingest_frames_scaled(fr, 2)
    flow = torch.zeros(1, 2, 8, 8)
    upscale_flow(flow, padder, 2, (16, 16))
    bads = [dict(flow=flow[0]), dict(flow=torch.zeros(1, 3, 8, 8)), dict(flow=flow.long()), dict(flow=flow.numpy()),
            dict(flow=torch.zeros(1, 2, 8, 16)), dict(scale=0), dict(scale=9), dict(scale=3), dict(size=(17, 16)),
            dict(size=(16, 18)), dict(size=(16,)), dict(size=(0, 16))]
    for kw in bads:
        a = dict(flow=flow, scale=2, size=(16, 16))
        a.update(kw)
        with pytest.raises(ValueError):
            upscale_flow(a["flow"], padder, a["scale"], a["size"])
    with pytest.raises(ValueError):
        scaled_shape(16, 16, 0)
    with pytest.raises(ValueError):
        FlowInference(None, small=True, device="cpu", scale=9)


@pytest.mark.skipif(not _ext.is_loaded(), reason=f"native library not built: {_ext.load_error()}")
def test_fake_kernel_shapes_and_dtypes():
    m = dict(device="meta")
    out = _ext.ops().ingest_frames_scaled(torch.empty(2, 37, 41, 3, dtype=torch.uint8, **m), 3, 1, 1, 1, 2)
    assert out.shape == (2, 3, 16, 16) and out.dtype == torch.float32 and out.device.type == "meta"
    out = _ext.ops().upscale_flow(torch.empty(2, 2, 16, 16, **m), 3, 1, 1, 14, 13, 37, 41)
    assert out.shape == (2, 2, 37, 41) and out.dtype == torch.float32 and out.device.type == "meta"


# ---------------------------------------------------------------------------- FlowInference
# The model refuses inputs below 128 x 128, so the frames are the smallest whose half is accepted:
# 249 x 299 -> 125 x 150 (both odd: partial last cells) -> padded to 128 x 152 (1 / 2 and 1 / 1).
HW = (249, 299)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(0)
    return [(rng.rand(*HW, 3) * 255).astype(np.uint8) for _ in range(3)]


@pytest.fixture(scope="module")
def inference():
    torch.manual_seed(0)
    return FlowInference(None, small=True, device="cpu", iters=2, consistency=True, track=True, track_cell=32, scale=2)


def _compose(inf, a, b, both=False):
    """ingest -> runner -> upscale by hand."""
    H, W = a.shape[:2]
    images, padder = ingest_frames_scaled(torch.from_numpy(np.stack([a, b])), 2)
    assert images.shape == (2, 3, 128, 152) and tuple(padder._pad) == (1, 1, 1, 2)
    i1, i2 = images[0:1], images[1:2]
    with torch.inference_mode():
        if both:
            i1, i2 = torch.cat([i1, i2]), torch.cat([i2, i1])
        _, up = inf.runner(i1, i2)
        return upscale_flow(up, padder, 2, (H, W))


def test_flow_inference_scale_on_the_cpu(frames, inference):
    a, b, c = frames
    inf = inference
    assert inf.scale == 2
    flow = inf.flow(a, b)
    assert flow.shape == (1, 2) + HW and flow.dtype == torch.float32
    assert torch.equal(flow, _compose(inf, a, b))
    img = inf.visualize(a, b)
    assert img.shape == HW + (3,) and img.dtype == np.uint8  # the camera frame, not the padded size
    assert np.array_equal(img, fc.host_image(flow[0], bgr=True))
    # both directions: one upscale of the batch of two
    want = _compose(inf, a, b, both=True)
    fw, occ, err2, counts = inf.flow_checked(a, b)
    assert torch.equal(fw, want[0:1]) and occ.shape == (1,) + HW
    assert torch.allclose(fw, flow, atol=1e-3)  # the batch of two rounds differently from the single pair
    want_occ = ops.fb_consistency_ref(want[0:1], want[1:2])
    assert torch.equal(occ, want_occ[0]) and sc.same(err2, want_occ[1]) and torch.equal(counts, want_occ[2])
    img2, mask = inf.visualize_checked(a, b)
    assert img2.shape == HW + (3,) and mask.shape == HW and np.array_equal(img2, fc.host_image(fw[0], bgr=True))
    # tracks: on the whole camera frame, no pad shift
    flow_t, tr = inf.tracks(a, b, prev_stamp=1.0, curr_stamp=2.0)
    assert torch.equal(flow_t, want[0:1])
    roi = (0, 0, HW[1], HW[0])
    ref = track_points_ref(*seed_points(1, roi, 32), want[0:1].contiguous(), want[1:2].contiguous(), roi, 32)
    assert tr["points"].shape == (8 * 10, 2) and tr["status"].tolist() == ref[5][0].tolist()
    assert sc.same(torch.from_numpy(tr["points"]), ref[0][0]) and sc.same(torch.from_numpy(tr["prev"]), ref[1][0])
    kept = tr["status"] == 0
    assert kept.any()
    for key in ("points", "prev"):
        x, y = tr[key][kept, 0], tr[key][kept, 1]
        assert (x >= 0).all() and (x <= HW[1] - 1).all() and (y >= 0).all() and (y <= HW[0] - 1).all()
    img3, mask3, tr3 = inf.visualize_tracks(b, c, prev_stamp=2.0, curr_stamp=3.0)  # continuous with the pair above
    assert img3.shape == HW + (3,) and mask3.shape == HW and inf._tracker.resets == 1 and tr3["age"].max() == 2
    # the continuity key holds the camera size: a frame one row taller has the same low-resolution shape
    taller = [np.concatenate([x, x[-1:]]) for x in (c, a)]
    _, tr4 = inf.tracks(*taller, prev_stamp=3.0, curr_stamp=4.0)
    assert scaled_shape(HW[0] + 1, HW[1], 2) == scaled_shape(*HW, 2) and inf._tracker.resets == 2
    assert tr4["age"].max() == 1


def test_flow_inference_scale_keeps_warm_start(frames):
    a, b, c = frames
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, warm_start=True, scale=2)
    inf.flow(a, b, prev_stamp=1.0, curr_stamp=2.0)
    assert inf._warm_shape == (1, 3, 128, 152) and inf._warm_flow.shape == (1, 2, 16, 19)  # the low resolution's
    warm = inf.flow(b, c, prev_stamp=2.0, curr_stamp=3.0)
    cold = inf.flow(b, c)
    assert warm.shape == cold.shape == (1, 2) + HW and not torch.equal(warm, cold)


def test_scale_one_is_todays_path(frames, inference):
    a, b = frames[0][:124, :150], frames[1][:124, :150]
    torch.manual_seed(0)
    plain = FlowInference(None, small=True, device="cpu", iters=2)
    assert plain.scale == 1
    inference.scale = 1
    try:
        got = inference.flow(a, b)
        assert got.shape == (1, 2, 128, 152) and torch.equal(got, plain.flow(a, b))
        assert np.array_equal(inference.visualize(a, b), plain.visualize(a, b))
    finally:
        inference.scale = 2


def test_the_model_refuses_a_half_below_its_minimum():
    """70 x 90 frames reduced by 2 are 35 x 45, padded 40 x 48: below the 128 x 128 the model
    accepts, with or without the working resolution."""
    rng = np.random.RandomState(1)
    a, b = [(rng.rand(70, 90, 3) * 255).astype(np.uint8) for _ in range(2)]
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, scale=2)
    i1, _ = inf._padded_pair(a, b)
    assert i1.shape == (1, 3, 40, 48)
    with pytest.raises(ValueError, match="at least 128x128"):
        inf.flow(a, b)


# ---------------------------------------------------------------------------- ROS node
class Recorder:
    def visualize(self, prev, curr, prev_stamp=None, curr_stamp=None):
        return np.zeros(prev.shape, np.uint8)


def test_node_passes_the_scale(monkeypatch):
    import raft_ros_amd.ros.node as node_mod

    seen = {}

    def fake_inference(weight_path, small, device, **kw):
        seen.clear()
        seen.update(kw)
        return Recorder()

    monkeypatch.setattr(node_mod, "FlowInference", fake_inference)
    base = {"/ROS/prev_img": "/p", "/ROS/curr_img": "/c", "/RAFT/weight_path": "", "/RAFT/is_small": True,
            "/RAFT/device": "cpu"}
    node = RaftRosNode(FakeRospy(dict(base)), image_msg=object, cv_bridge_cls=FakeBridge)
    assert node.scale == 1 and seen.get("scale", 1) == 1
    node = RaftRosNode(FakeRospy(dict(base, **{"/RAFT/scale": 3})), image_msg=object, cv_bridge_cls=FakeBridge)
    assert node.scale == 3 and seen["scale"] == 3 and isinstance(seen["scale"], int)
    img = np.zeros((16, 24, 3), np.uint8)
    out = node.process_pair(Msg(1.0, img), Msg(2.0, img))
    assert out.data.shape == (16, 24, 3)


def test_config_yaml_has_the_scale():
    text = open(os.path.join(ROOT, "ros", "config", "config.yaml")).read()
    assert "scale: 1" in text


# ---------------------------------------------------------------------------- demo.py
def test_demo_scale_flag(tmp_path):
    import demo

    frames_dir = tmp_path / "frames"
    os.makedirs(frames_dir)
    for k in (16, 17, 18):
        shutil.copy(os.path.join(ROOT, "demo-frames", "frame_%04d.png" % k), frames_dir)
    W, H = Image.open(frames_dir / "frame_0016.png").size
    assert (W, H) == (1024, 436)
    torch.manual_seed(0)
    outs = demo.main(["--path", str(frames_dir), "--device", "cpu", "--small", "--iters", "2", "--scale", "2",
                      "--occlusion", "--tracks", "--track_cell", "64", "--warm_start", "--output", str(tmp_path / "out")])
    assert [os.path.basename(f) for f in outs] == ["flow_0000.png", "flow_0001.png"]
    raw = np.array(Image.open(frames_dir / "frame_0016.png").convert("RGB"))
    for k, f in enumerate(outs):
        pic = np.array(Image.open(f))
        assert pic.shape == (2 * H, W, 3)  # [image; flow] at the raw frame's size, not the padded low resolution's
        occ = np.array(Image.open(tmp_path / "out" / ("occ_%04d.png" % k)))
        assert occ.shape == (H, W) and set(np.unique(occ).tolist()) <= {0, 128, 255}
    assert np.array_equal(np.array(Image.open(outs[0]))[:H], raw)  # the raw frame itself on top
    with open(tmp_path / "out" / "tracks.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "id", "x", "y", "prev_x", "prev_y", "age"] and len(rows) > 1
    for r in rows[1:]:
        x, y, px, py = map(float, r[2:6])
        assert 0 <= x <= W - 1 and 0 <= y <= H - 1 and 0 <= px <= W - 1 and 0 <= py <= H - 1
