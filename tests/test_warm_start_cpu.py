"""Warm start without a GPU: the Python layer, the brute-force oracle, the fake kernel, and the
consumers (FlowInference, the ROS node with fakes, demo.py --warm_start)."""
import os
import types
from argparse import Namespace

import numpy as np
import pytest
import torch
from PIL import Image

import warm_start_cases as wc
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops.reference import forward_splat_nearest_ref
from raft_ros_amd.ops.warm_start import forward_splat_nearest
from raft_ros_amd.ros.node import FlowInference, RaftRosNode
from raft_ros_amd.utils.utils import forward_interpolate
from test_ros_cpu import FakeBridge, FakeRospy, Msg

MAX_EXCLUDED = 0.01  # share of pixels whose two nearest points are closer than 1e-9 in d2


def test_cpu_path_is_forward_interpolate():
    f = wc.case("random3", (16, 24))
    out = forward_splat_nearest(f)
    assert out.shape == f.shape and out.dtype == torch.float32 and out.device.type == "cpu"
    for b in range(f.shape[0]):
        want = forward_interpolate(f[b])
        assert torch.equal(out[b], want)                      # a batch is the per-image results
        assert torch.equal(forward_splat_nearest(f[b]), want)  # (2, H, W) in, (2, H, W) out
    assert torch.equal(forward_splat_nearest(wc.case("all_out", (16, 24))), torch.zeros(2, 2, 16, 24))
    with pytest.raises(ValueError):
        forward_splat_nearest(torch.zeros(3, 16, 24))


@pytest.mark.parametrize("shape", wc.SHAPES)
@pytest.mark.parametrize("name", wc.RANDOM)
def test_oracle_matches_scipy_where_unambiguous(name, shape):
    want, gap = wc.oracle(name, shape)
    keep = gap >= 1e-9
    excluded = 1.0 - keep.double().mean().item()
    print(f"{name} {shape}: excluded {excluded:.4f}")
    assert excluded <= MAX_EXCLUDED
    keep = keep[:, None].expand_as(want)
    assert torch.equal(want[keep], wc.scipy_result(name, shape)[keep])


@pytest.mark.parametrize("shape", wc.SHAPES)
@pytest.mark.parametrize("name", sorted(wc.RING_TIES))
def test_oracle_ring_boundary_tie(name, shape):
    _, (xt, yt), expect = wc.RING_TIES[name]
    out = forward_splat_nearest_ref(wc.case("ring_" + name, shape))
    assert tuple(out[0, :, yt, xt].tolist()) == expect


def test_oracle_edge_cases():
    shape = (17, 23)
    assert torch.equal(wc.oracle("all_out", shape)[0], torch.zeros(2, 2, *shape))
    one = wc.oracle("one_point", shape)[0]
    assert (one[0, 0] == 0.5).all() and (one[0, 1] == -0.25).all() and (one[1, 0] == -0.5).all()
    assert torch.isfinite(wc.oracle("non_finite", shape)[0]).all()
    # zero flow: row 0 / column 0 are not valid points, so their pixels take a neighbour's flow
    # (still zero) and the moved block shows only where it landed
    z = wc.oracle("zero_with_block", shape)[0]
    assert (z[0, :, 8:12, 8:15] == torch.tensor([6.0, 5.0])[:, None, None]).all()
    f = wc.case("random3", shape)
    assert torch.equal(forward_splat_nearest_ref(f[1]), wc.oracle("random3", shape)[0][1])  # (2, H, W) form


@pytest.mark.skipif(not _ext.is_loaded(), reason=f"native library not built: {_ext.load_error()}")
def test_fake_kernel_shape_and_dtype():
    f = torch.empty(3, 2, 17, 23, device="meta")
    out = _ext.ops().forward_splat_nearest(f)
    assert out.shape == f.shape and out.dtype == torch.float32 and out.device.type == "meta"


# ---------------------------------------------------------------------------- FlowInference
class RecordingRunner:
    """Stands in for GraphedRAFT: records flow_init, returns a flow that depends on the call."""

    def __init__(self):
        self.inits, self.lows = [], []

    def __call__(self, image1, image2, flow_init=None):
        self.inits.append(flow_init)
        H, W = image1.shape[-2:]
        low = wc._randn(H // 8, W // 8, 2.0, 100 + len(self.lows))[None]
        self.lows.append(low)
        return low, torch.zeros(1, 2, H, W)


@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(0)
    return [(rng.rand(128, 160, 3) * 255).astype(np.uint8) for _ in range(3)]


def _warm_inference(warm_start=True):
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, warm_start=warm_start)
    inf.runner = RecordingRunner()
    return inf


def test_flow_inference_warm_and_cold_calls(frames):
    inf = _warm_inference()
    r = inf.runner
    a, b, c = frames
    inf.flow(a, b, prev_stamp=1.0, curr_stamp=2.0)
    assert r.inits[-1] is None  # first pair
    inf.flow(b, c, prev_stamp=2.0, curr_stamp=3.0)
    assert torch.equal(r.inits[-1], forward_splat_nearest(r.lows[0]))  # continuous pair
    inf.flow(a, b, prev_stamp=3.5, curr_stamp=4.0)
    assert r.inits[-1] is None  # stamp gap
    inf.flow(b, c, prev_stamp=4.0, curr_stamp=5.0)
    assert torch.equal(r.inits[-1], forward_splat_nearest(r.lows[2]))  # and warm again after it
    inf.flow(a, b, curr_stamp=6.0)
    assert r.inits[-1] is None  # missing stamp
    inf.flow(b, c, prev_stamp=6.0)
    assert r.inits[-1] is not None  # the previous call still left its state
    inf.flow(a, b, prev_stamp=None, curr_stamp=None)
    inf.flow(b, c, prev_stamp=None, curr_stamp=None)
    assert r.inits[-1] is None  # no stamps at all: never warm
    inf.flow(a, b, prev_stamp=7.0, curr_stamp=8.0)
    inf.flow(b[:120], c[:120], prev_stamp=8.0, curr_stamp=9.0)
    assert r.inits[-1] is None  # frame size changed
    inf.flow(b[:120], c[:120], prev_stamp=9.0, curr_stamp=10.0)
    assert r.inits[-1] is not None
    inf.reset_warm_start()
    inf.flow(b[:120], c[:120], prev_stamp=10.0, curr_stamp=11.0)
    assert r.inits[-1] is None  # reset_warm_start()


def test_flow_inference_off_never_warm_and_unchanged(frames):
    a, b, c = frames
    off = _warm_inference(warm_start=False)
    off.flow(a, b, prev_stamp=1.0, curr_stamp=2.0)
    off.flow(b, c, prev_stamp=2.0, curr_stamp=3.0)
    assert off.runner.inits == [None, None]
    torch.manual_seed(0)
    plain = FlowInference(None, small=True, device="cpu", iters=2)
    torch.manual_seed(0)
    off = FlowInference(None, small=True, device="cpu", iters=2, warm_start=False)
    for (p, q), (s, t) in zip(((a, b), (b, c)), ((1.0, 2.0), (2.0, 3.0))):
        assert plain.visualize(p, q).tobytes() == off.visualize(p, q, prev_stamp=s, curr_stamp=t).tobytes()


def test_flow_inference_warm_start_runs_the_model(frames):
    """The real runner on the CPU: the warm second pair equals the model called with the splat."""
    a, b, c = frames
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, warm_start=True)
    to_t = lambda x: torch.from_numpy(x).permute(2, 0, 1).float()[None]  # noqa: E731
    with torch.no_grad():
        low0, _ = inf.model(to_t(a), to_t(b), iters=2, test_mode=True)
        _, want = inf.model(to_t(b), to_t(c), iters=2, flow_init=forward_splat_nearest(low0), test_mode=True)
    inf.flow(a, b, prev_stamp=1.0, curr_stamp=2.0)
    got = inf.flow(b, c, prev_stamp=2.0, curr_stamp=3.0)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------- ROS node
class StampRecorder:
    def __init__(self, warm_start):
        self.warm_start = warm_start
        self.calls = []

    def visualize(self, prev, curr, prev_stamp=None, curr_stamp=None):
        self.calls.append((prev_stamp, curr_stamp))
        return np.zeros(prev.shape, np.uint8)


@pytest.mark.parametrize("param,expect", [({"/RAFT/warm_start": True}, (1.0, 2.0)), ({}, (None, None))])
def test_node_passes_stamps_only_with_the_parameter(param, expect):
    rospy = FakeRospy({"/ROS/prev_img": "/p", "/ROS/curr_img": "/c", **param})
    rec = StampRecorder(bool(param))
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=rec)
    assert node.warm_start is bool(param)
    img = np.zeros((16, 24, 3), np.uint8)
    node.process_pair(Msg(1.0, img), Msg(2.0, img))
    assert rec.calls == [expect]
    assert len(rospy.pubs[0].sent) == 1 and rospy.pubs[0].sent[0].header.stamp.t == 2.0


def test_node_builds_inference_from_parameters(monkeypatch):
    import raft_ros_amd.ros.node as node_mod

    seen = {}

    def fake_inference(weight_path, small, device, **kw):
        seen.update(kw, small=small, device=device)
        return StampRecorder(kw["warm_start"])

    monkeypatch.setattr(node_mod, "FlowInference", fake_inference)
    base = {"/ROS/prev_img": "/p", "/ROS/curr_img": "/c", "/RAFT/weight_path": "", "/RAFT/is_small": True,
            "/RAFT/device": "cpu"}
    RaftRosNode(FakeRospy(dict(base)), image_msg=object, cv_bridge_cls=FakeBridge)
    assert seen["warm_start"] is False and seen["iters"] == 20  # missing parameters: off, 20 iterations
    RaftRosNode(FakeRospy(dict(base, **{"/RAFT/warm_start": True, "/RAFT/iters": 12})), image_msg=object,
                cv_bridge_cls=FakeBridge)
    assert seen["warm_start"] is True and seen["iters"] == 12


def test_config_yaml_has_the_new_keys():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "ros", "config", "config.yaml")).read()
    assert "warm_start: false" in text and "iters: 20" in text


# ---------------------------------------------------------------------------- demo.py
def _write_frames(path, n=3):
    from raft_ros_amd.data.synthetic import demo_sequence

    os.makedirs(path)
    for k, fr in enumerate(demo_sequence(n, 128, 160)):
        Image.fromarray(fr.permute(1, 2, 0).numpy()).save(os.path.join(path, "frame_%04d.png" % k))


def test_demo_warm_start_flag(tmp_path):
    import demo
    from raft_ros_amd.models import RAFT
    from raft_ros_amd.utils.utils import InputPadder

    frames_dir = str(tmp_path / "frames")
    _write_frames(frames_dir)
    common = ["--path", frames_dir, "--device", "cpu", "--small", "--iters", "2"]
    torch.manual_seed(0)
    warm = demo.main(common + ["--warm_start", "--output", str(tmp_path / "warm")])
    torch.manual_seed(0)
    cold = demo.main(common + ["--output", str(tmp_path / "cold")])
    assert len(warm) == len(cold) == 2 and all(os.path.exists(f) for f in warm + cold)
    read = lambda f: open(f, "rb").read()  # noqa: E731
    assert read(warm[0]) == read(cold[0])  # the first pair has nothing to start from
    assert read(warm[1]) != read(cold[1])  # the second starts from the first pair's flow

    # without the flag: byte-identical to the loop demo.py ran before it had the flag
    torch.manual_seed(0)
    model = RAFT(Namespace(small=True, mixed_precision=False, alternate_corr=False)).eval()
    files = sorted(os.listdir(frames_dir))
    with torch.inference_mode():
        for k, (f1, f2) in enumerate(zip(files[:-1], files[1:])):
            image1 = demo.load_image(os.path.join(frames_dir, f1), "cpu")
            image2 = demo.load_image(os.path.join(frames_dir, f2), "cpu")
            image1, image2 = InputPadder(image1.shape).pad(image1, image2)
            _, flow_up = model(image1, image2, iters=2, test_mode=True)
            out = str(tmp_path / ("parent_%d.png" % k))
            demo.viz(image1, flow_up, out)
            assert read(out) == read(cold[k])
