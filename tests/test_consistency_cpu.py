"""Forward-backward consistency without a GPU: the torch reference against a per-pixel loop, the
Python layer, the fake kernel, and the consumers (FlowInference's bidirectional mode, the ROS node
with fakes, demo.py --occlusion)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import consistency_cases as cc
from raft_ros_amd import ops
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops.consistency import fb_consistency, fb_consistency_ref
from raft_ros_amd.ops.warm_start import forward_splat_nearest
from raft_ros_amd.ros.node import FlowInference, RaftRosNode
from test_ros_cpu import FakeBridge, FakeRospy, Msg


# ---------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("alphas", [(0.01, 0.5), (0.05, 0.125)])
def test_reference_is_the_per_pixel_loop(alphas):
    """5 x 7, numpy.float32 scalars in the specification's order: bitwise."""
    fw, bw = cc.random_pair(5, 7, seed=1)
    fw[:, 2, 3] = torch.tensor([0.5, -0.25])   # fractional target well inside
    fw[:, 0, 0] = torch.tensor([6.0, 4.0])     # the corner (W-1, H-1) exactly
    occ, err2, counts = fb_consistency_ref(fw[None], bw[None], *alphas)
    w_occ, w_err2, w_counts = cc.loop_reference(fw.numpy(), bw.numpy(), *alphas)
    assert occ.dtype == torch.uint8 and err2.dtype == torch.float32 and counts.dtype == torch.int32
    assert len(set(w_occ.ravel().tolist())) == 3  # the loop saw every class
    assert np.array_equal(occ[0].numpy(), w_occ)
    assert err2[0].numpy().tobytes() == w_err2.tobytes()
    assert np.array_equal(counts[0].numpy(), w_counts)


def test_reference_on_the_special_fields():
    fw, bw = cc.edge_pair()
    occ, err2, counts = fb_consistency_ref(fw[None], bw[None])
    for (y, x), (_, want) in cc.EDGE_POINTS.items():
        if want is not None:
            assert occ[0, y, x] == want and err2[0, y, x] == float("inf"), (y, x)
        else:
            assert occ[0, y, x] != 2 and torch.isfinite(err2[0, y, x]), (y, x)
    assert occ[0, 3, 20] == 1 and occ[0, 8, 0] != 2  # reads the large last column; -0.0 is inside
    w = cc.loop_reference(fw.numpy(), bw.numpy(), 0.01, 0.5)
    assert np.array_equal(occ[0].numpy(), w[0]) and err2[0].numpy().tobytes() == w[1].tobytes()
    assert counts[0].tolist() == [int((occ == 1).sum()), int((occ == 2).sum())]

    fw, bw = cc.nonfinite_pair()
    occ, err2, _ = fb_consistency_ref(fw[None], bw[None])
    for (_, y, x) in cc.NONFINITE_FW:
        assert occ[0, y, x] == 2 and err2[0, y, x] == float("inf")
    y, x = cc.NONFINITE_SAMPLER
    assert occ[0, y, x] == 1 and torch.isnan(err2[0, y, x])


def test_parity_field_has_every_class():
    fw, bw = cc.parity_pair()
    assert fw.shape == (2, 37, 41)
    shares = cc.class_shares(fb_consistency_ref(fw[None], bw[None])[0])
    print("class shares", shares)
    assert min(shares) >= cc.MIN_SHARE


# ---------------------------------------------------------------------------- the Python layer
def test_wrapper_shapes_and_cpu_path():
    fw, bw = cc.scaled_batch()
    want = fb_consistency_ref(fw, bw, 0.01, 0.5)
    got = fb_consistency(fw, bw)  # the defaults are 0.01 and 0.5
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert got[0].shape == (3, 37, 41) and got[1].shape == (3, 37, 41) and got[2].shape == (3, 2)
    one = fb_consistency(fw[1], bw[1])  # (2, H, W) in: B dropped
    assert one[0].shape == (37, 41) and one[1].shape == (37, 41) and one[2].shape == (2,)
    assert all(torch.equal(o, w[1]) for o, w in zip(one, want))
    # half and non-contiguous inputs are converted
    h = fb_consistency(fw.half(), bw.half())
    assert all(torch.equal(g, w) for g, w in zip(h, fb_consistency_ref(fw.half().float(), bw.half().float())))
    wide_f, wide_b = torch.zeros(3, 2, 37, 82), torch.zeros(3, 2, 37, 82)
    wide_f[..., ::2], wide_b[..., ::2] = fw, bw
    assert all(torch.equal(g, w) for g, w in zip(fb_consistency(wide_f[..., ::2], wide_b[..., ::2]), want))
    other = fb_consistency(fw, bw, alpha1=0.0, alpha2=1e-3)
    assert other[2][:, 0].sum() > want[2][:, 0].sum()  # a tighter criterion: more inconsistent pixels
    empty = fb_consistency(torch.zeros(0, 2, 4, 4), torch.zeros(0, 2, 4, 4))
    assert empty[0].shape == (0, 4, 4) and empty[2].shape == (0, 2)
    empty = fb_consistency(torch.zeros(2, 2, 0, 4), torch.zeros(2, 2, 0, 4))
    assert empty[0].shape == (2, 0, 4) and empty[2].tolist() == [[0, 0], [0, 0]]


def test_wrapper_errors():
    f = torch.zeros(2, 5, 7)
    for bad in ((torch.zeros(3, 5, 7), f), (f, torch.zeros(5, 7)), (f, torch.zeros(2, 5, 8)),
                (f, torch.zeros(1, 2, 5, 7)), (f.long(), f), (f, f.to(torch.uint8)), (f.numpy(), f)):
        with pytest.raises(ValueError):
            fb_consistency(*bad)


def test_ops_export():
    assert ops.fb_consistency is fb_consistency and ops.fb_consistency_ref is fb_consistency_ref


@pytest.mark.skipif(not _ext.is_loaded(), reason=f"native library not built: {_ext.load_error()}")
def test_fake_kernel_shapes_and_dtypes():
    f = torch.empty(3, 2, 17, 23, device="meta")
    occ, err2, counts = _ext.ops().fb_consistency(f, f, 0.01, 0.5)
    assert occ.shape == (3, 17, 23) and occ.dtype == torch.uint8 and occ.device.type == "meta"
    assert err2.shape == (3, 17, 23) and err2.dtype == torch.float32
    assert counts.shape == (3, 2) and counts.dtype == torch.int32


# ---------------------------------------------------------------------------- FlowInference
class RecordingRunner:
    """Stands in for GraphedRAFT: records its inputs, returns flows that depend on the call."""

    def __init__(self):
        self.calls, self.lows, self.ups = [], [], []

    def __call__(self, image1, image2, flow_init=None):
        self.calls.append((image1, image2, flow_init))
        B, _, H, W = image1.shape
        k = len(self.lows)
        low = torch.stack([cc.gaussian(H // 8, W // 8, 2.0, seed=100 + 2 * k + b) for b in range(B)])
        up = torch.stack([cc.gaussian(H, W, 2.0, seed=500 + 2 * k + b) for b in range(B)])
        self.lows.append(low)
        self.ups.append(up)
        return low, up


@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(0)
    return [(rng.rand(128, 160, 3) * 255).astype(np.uint8) for _ in range(3)]


def _to_t(x):
    return torch.from_numpy(x).permute(2, 0, 1).float()[None]


def _stub_inference(**kw):
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, consistency=True, **kw)
    inf.runner = RecordingRunner()
    return inf


def test_flow_checked_stacks_and_swaps_the_pair(frames):
    a, b, _ = frames
    inf = _stub_inference()
    flow_fw, occ, err2, counts = inf.flow_checked(a, b)
    image1, image2, init = inf.runner.calls[-1]
    assert init is None
    assert torch.equal(image1, torch.cat([_to_t(a), _to_t(b)])) and torch.equal(image2, torch.cat([_to_t(b), _to_t(a)]))
    up = inf.runner.ups[-1]
    assert torch.equal(flow_fw, up[0:1])
    want = fb_consistency(up[0:1], up[1:2])
    assert torch.equal(occ, want[0]) and cc.same(err2, want[1]) and torch.equal(counts, want[2])
    assert occ.shape == (1, 128, 160) and counts.shape == (1, 2)


def test_flow_checked_warm_init_and_cold_on_a_stamp_gap(frames):
    a, b, c = frames
    inf = _stub_inference(warm_start=True)
    r = inf.runner
    inf.flow_checked(a, b, prev_stamp=1.0, curr_stamp=2.0)
    assert r.calls[-1][2] is None  # first pair
    inf.flow_checked(b, c, prev_stamp=2.0, curr_stamp=3.0)
    kept = forward_splat_nearest(r.lows[0][0:1])  # the forward direction only
    assert torch.equal(r.calls[-1][2], torch.cat([kept, torch.zeros_like(kept)]))
    assert r.calls[-1][0].shape[0] == 2
    inf.flow_checked(a, b, prev_stamp=3.5, curr_stamp=4.0)
    assert r.calls[-1][2] is None  # stamp gap
    inf.flow_checked(b, c, prev_stamp=4.0, curr_stamp=5.0)
    assert r.calls[-1][2] is not None  # and warm again after it
    inf.flow_checked(a, b)
    assert r.calls[-1][2] is None  # no stamps: never warm
    # flow() shares the kept state and still makes batch-1 calls
    inf.flow_checked(a, b, prev_stamp=6.0, curr_stamp=7.0)
    inf.flow(b, c, prev_stamp=7.0, curr_stamp=8.0)
    image1, _, init = r.calls[-1]
    assert image1.shape[0] == 1 and init.shape[0] == 1
    assert torch.equal(init, forward_splat_nearest(r.lows[-2][0:1]))


def test_flow_stays_batch_one_and_checked_needs_the_option(frames):
    a, b, _ = frames
    inf = _stub_inference()
    inf.flow(a, b)
    image1, image2, init = inf.runner.calls[-1]
    assert image1.shape == (1, 3, 128, 160) and image2.shape == (1, 3, 128, 160) and init is None
    off = FlowInference(None, small=True, device="cpu", iters=2)
    assert off.consistency is False
    with pytest.raises(RuntimeError):
        off.flow_checked(a, b)
    with pytest.raises(RuntimeError):
        off.visualize_checked(a, b)


def test_checked_runs_the_model_on_the_cpu(frames):
    """The real runner: the forward direction of the batch is the model on the stacked pair, the
    image is visualize()'s colour coding of it, the mask codes the classes."""
    a, b, _ = frames
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, consistency=True)
    with torch.no_grad():
        _, up = inf.model(torch.cat([_to_t(a), _to_t(b)]), torch.cat([_to_t(b), _to_t(a)]), iters=2, test_mode=True)
    flow_fw, occ, err2, counts = inf.flow_checked(a, b)
    assert torch.equal(flow_fw, up[0:1])
    want = fb_consistency_ref(up[0:1], up[1:2])
    assert torch.equal(occ, want[0]) and cc.same(err2, want[1]) and torch.equal(counts, want[2])
    img, mask = inf.visualize_checked(a, b)
    assert img.shape == (128, 160, 3) and img.dtype == np.uint8
    assert mask.shape == (128, 160) and mask.dtype == np.uint8 and mask.flags.owndata and mask.flags.c_contiguous
    assert np.array_equal(mask, np.array([0, 128, 255], np.uint8)[occ[0].numpy()])
    assert inf.last_counts.shape == (2,)
    assert inf.last_counts.tolist() == [int((mask == 128).sum()), int((mask == 255).sum())]


# ---------------------------------------------------------------------------- ROS node
class CheckedRecorder:
    def __init__(self):
        self.calls = []

    def visualize(self, prev, curr, prev_stamp=None, curr_stamp=None):
        self.calls.append(("visualize", prev_stamp, curr_stamp))
        return np.zeros(prev.shape, np.uint8)

    def visualize_checked(self, prev, curr, prev_stamp=None, curr_stamp=None):
        self.calls.append(("visualize_checked", prev_stamp, curr_stamp))
        mask = np.zeros(prev.shape[:2], np.uint8)
        mask[2:4], mask[5] = 128, 255
        return np.zeros(prev.shape, np.uint8), mask


BASE = {"/ROS/prev_img": "/p", "/ROS/curr_img": "/c"}


def test_node_without_the_parameter_has_one_publisher():
    rospy = FakeRospy(dict(BASE))
    rec = CheckedRecorder()
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=rec)
    assert node.occlusion is False and [p.topic for p in rospy.pubs] == ["/raft_result"]
    img = np.zeros((16, 24, 3), np.uint8)
    node.process_pair(Msg(1.0, img), Msg(2.0, img))
    assert rec.calls == [("visualize", None, None)] and len(rospy.pubs[0].sent) == 1


@pytest.mark.parametrize("warm", [False, True])
def test_node_publishes_the_mask(warm):
    rospy = FakeRospy(dict(BASE, **{"/RAFT/occlusion": True, "/RAFT/warm_start": warm}))
    rec = CheckedRecorder()
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=rec)
    assert node.occlusion is True
    assert [(p.topic, p.queue_size) for p in rospy.pubs] == [("/raft_result", 100), ("/raft_occlusion", 100)]
    img = np.zeros((16, 24, 3), np.uint8)
    out = node.process_pair(Msg(1.0, img), Msg(2.0, img))
    assert rec.calls == [("visualize_checked",) + ((1.0, 2.0) if warm else (None, None))]
    res, occ = rospy.pubs[0].sent, rospy.pubs[1].sent
    assert len(res) == 1 and len(occ) == 1 and res[0] is out and res[0].encoding == "passthrough"
    assert occ[0].encoding == "mono8" and occ[0].header is res[0].header
    assert occ[0].header.frame_id == "raft_image" and occ[0].header.stamp.t == 2.0
    assert occ[0].data.shape == (16, 24) and occ[0].data.dtype == np.uint8
    assert set(np.unique(occ[0].data).tolist()) == {0, 128, 255}


def test_node_builds_inference_with_consistency(monkeypatch):
    import raft_ros_amd.ros.node as node_mod

    seen = {}

    def fake_inference(weight_path, small, device, **kw):
        seen.update(kw)
        return CheckedRecorder()

    monkeypatch.setattr(node_mod, "FlowInference", fake_inference)
    base = dict(BASE, **{"/RAFT/weight_path": "", "/RAFT/is_small": True, "/RAFT/device": "cpu"})
    RaftRosNode(FakeRospy(dict(base)), image_msg=object, cv_bridge_cls=FakeBridge)
    assert seen["consistency"] is False
    RaftRosNode(FakeRospy(dict(base, **{"/RAFT/occlusion": True})), image_msg=object, cv_bridge_cls=FakeBridge)
    assert seen["consistency"] is True


def test_node_end_to_end_mask_coding():
    """The real inference on the CPU behind the node: a mono8 message of the padded size in the
    0 / 128 / 255 coding."""
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, consistency=True)
    rospy = FakeRospy(dict(BASE, **{"/RAFT/occlusion": True}))
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=inf)
    rng = np.random.RandomState(1)
    a, b = [(rng.rand(130, 150, 3) * 255).astype(np.uint8) for _ in range(2)]
    node.process_pair(Msg(1.0, a), Msg(2.0, b))
    res, occ = rospy.pubs[0].sent[0], rospy.pubs[1].sent[0]
    assert res.data.shape == (136, 152, 3) and occ.data.shape == (136, 152) and occ.encoding == "mono8"
    assert set(np.unique(occ.data).tolist()) <= {0, 128, 255}
    assert inf.last_counts.tolist() == [int((occ.data == 128).sum()), int((occ.data == 255).sum())]


def test_config_yaml_has_the_parameter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "ros", "config", "config.yaml")).read()
    assert "occlusion: false" in text


# ---------------------------------------------------------------------------- demo.py
def _write_frames(path, n=3):
    from raft_ros_amd.data.synthetic import demo_sequence

    os.makedirs(path)
    for k, fr in enumerate(demo_sequence(n, 128, 128)):
        Image.fromarray(fr.permute(1, 2, 0).numpy()).save(os.path.join(path, "frame_%04d.png" % k))


def test_demo_occlusion_flag(tmp_path):
    import demo

    frames_dir = str(tmp_path / "frames")
    _write_frames(frames_dir)
    common = ["--path", frames_dir, "--device", "cpu", "--small", "--iters", "2"]
    torch.manual_seed(0)
    outs = demo.main(common + ["--occlusion", "--output", str(tmp_path / "occ")])
    torch.manual_seed(0)
    plain = demo.main(common + ["--output", str(tmp_path / "plain")])
    # the return value is the flow images, as without the option
    assert [os.path.basename(f) for f in outs] == [os.path.basename(f) for f in plain] == ["flow_0000.png",
                                                                                           "flow_0001.png"]
    assert sorted(os.listdir(tmp_path / "plain")) == ["flow_0000.png", "flow_0001.png"]
    for k in range(2):
        mask = Image.open(str(tmp_path / "occ" / ("occ_%04d.png" % k)))
        assert mask.mode == "L" and mask.size == (128, 128)
        assert set(np.unique(np.array(mask)).tolist()) <= {0, 128, 255}
    # with --warm_start the option still runs (the backward direction starts cold)
    torch.manual_seed(0)
    warm = demo.main(common + ["--occlusion", "--warm_start", "--output", str(tmp_path / "warm")])
    assert len(warm) == 2 and os.path.exists(str(tmp_path / "warm" / "occ_0001.png"))
