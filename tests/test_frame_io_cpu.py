"""Frame path without a GPU: the Python layer's CPU fallbacks, argument checks, the fake kernels,
and the consumers (FlowInference, the ROS node with fakes, demo.py --device_viz), which on a CPU
device must produce exactly what they produce without the option."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import frame_io_cases as fc
from raft_ros_amd import ops
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops.frame_io import flow_to_image, ingest_frames
from raft_ros_amd.ros.node import FlowInference, RaftRosNode
from raft_ros_amd.utils.utils import InputPadder
from test_ros_cpu import FakeBridge, FakeRospy, Msg


def test_exported_from_ops():
    assert ops.flow_to_image is flow_to_image and ops.ingest_frames is ingest_frames


@pytest.mark.parametrize("bgr", [False, True])
def test_flow_to_image_cpu_is_numpy_flow_viz(bgr):
    f = fc.scaled_batch()
    out = flow_to_image(f, convert_to_bgr=bgr)
    assert out.shape == (3, 37, 41, 3) and out.dtype == torch.uint8 and out.device.type == "cpu"
    for b in range(3):  # a batch is the per-image results, each with its own maximum
        want = fc.host_image(f[b], bgr=bgr)
        assert np.array_equal(out[b].numpy(), want)
        one = flow_to_image(f[b], convert_to_bgr=bgr)  # (2, H, W) in, (H, W, 3) out
        assert one.shape == (37, 41, 3) and np.array_equal(one.numpy(), want)
    assert np.array_equal(flow_to_image(f[1], clip_flow=3.0).numpy(), fc.host_image(f[1], clip_flow=3.0))
    fix = np.load(os.path.join(fc.golden.GOLDEN, "flow_viz.npz"))
    assert np.array_equal(flow_to_image(fc.parity_flow(), convert_to_bgr=bgr).numpy(), fix["bgr" if bgr else "rgb"])


@pytest.mark.parametrize("mode", ["sintel", "kitti"])
def test_ingest_frames_cpu_is_input_padder(mode):
    fr = fc.frames(2, 13, 17)
    out, padder = ingest_frames(fr, mode=mode)
    chw = fr.permute(0, 3, 1, 2).float()
    want = InputPadder(chw.shape, mode=mode).pad(chw)[0]
    assert out.dtype == torch.float32 and out.shape == (2, 3, 16, 24) and torch.equal(out, want)
    assert torch.equal(padder.unpad(out), chw)  # a working padder
    # a list of (H, W, 3) arrays or tensors is the stacked tensor
    for items in ([x.numpy() for x in fr], list(fr)):
        got, p2 = ingest_frames(items, mode=mode)
        assert torch.equal(got, want) and p2._pad == padder._pad


def test_shape_and_dtype_errors():
    for bad in (torch.zeros(3, 16, 24), torch.zeros(2, 3, 16, 24), torch.zeros(16, 24),
                torch.zeros(2, 16, 24, dtype=torch.int32)):
        with pytest.raises(ValueError):
            flow_to_image(bad)
    for bad in (torch.zeros(2, 16, 24, 3), torch.zeros(2, 3, 16, 24, dtype=torch.uint8),
                torch.zeros(16, 24, 3, dtype=torch.uint8), [],
                [np.zeros((16, 24, 3), np.uint8), np.zeros((16, 25, 3), np.uint8)]):
        with pytest.raises(ValueError):
            ingest_frames(bad)


def test_fake_kernels_shape_and_dtype():
    assert _ext.is_loaded(), f"native library not built: {_ext.load_error()}"
    m = torch.device("meta")
    img = _ext.ops().flow_to_image(torch.empty(3, 2, 37, 41, device=m), None, True)
    assert img.shape == (3, 37, 41, 3) and img.dtype == torch.uint8 and img.device.type == "meta"
    out = _ext.ops().ingest_frames(torch.empty(2, 13, 17, 3, device=m, dtype=torch.uint8), 3, 4, 1, 2)
    assert out.shape == (2, 3, 16, 24) and out.dtype == torch.float32 and out.device.type == "meta"


# ---------------------------------------------------------------------------- consumers
@pytest.fixture(scope="module")
def pair():
    rng = np.random.RandomState(0)
    return [(rng.rand(130, 150, 3) * 255).astype(np.uint8) for _ in range(2)]


@pytest.fixture(scope="module")
def inferences():
    out = []
    for device_io in (False, True):
        torch.manual_seed(0)
        out.append(FlowInference(None, small=True, device="cpu", iters=2, device_io=device_io))
    return out


def test_flow_inference_cpu_flag_changes_nothing(pair, inferences):
    off, on = inferences
    assert on.device_io and not off.device_io
    assert on.visualize(*pair).tobytes() == off.visualize(*pair).tobytes()


def test_node_reads_device_io_and_publishes_the_same_image(monkeypatch, pair, inferences):
    import raft_ros_amd.ros.node as node_mod

    seen = []

    def fake_inference(weight_path, small, device, **kw):
        seen.append(kw["device_io"])
        return inferences[int(kw["device_io"])]

    monkeypatch.setattr(node_mod, "FlowInference", fake_inference)
    base = {"/ROS/prev_img": "/p", "/ROS/curr_img": "/c", "/RAFT/weight_path": "", "/RAFT/is_small": True,
            "/RAFT/device": "cpu"}
    sent = []
    for params in (base, dict(base, **{"/RAFT/device_io": True})):
        rospy = FakeRospy(dict(params))
        node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge)
        node.process_pair(Msg(1.0, pair[0]), Msg(2.0, pair[1]))
        sent.append(rospy.pubs[0].sent[0].data)
    assert seen == [False, True]  # missing parameter: off
    assert sent[0].shape == (136, 152, 3) and sent[0].tobytes() == sent[1].tobytes()


def test_config_yaml_documents_device_io():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "device_io: false" in open(os.path.join(root, "ros", "config", "config.yaml")).read()


def test_demo_device_viz_flag_on_cpu(tmp_path):
    import demo
    from raft_ros_amd.data.synthetic import demo_sequence

    frames_dir = str(tmp_path / "frames")
    os.makedirs(frames_dir)
    for k, fr in enumerate(demo_sequence(3, 130, 158)):  # padded to 136 x 160
        Image.fromarray(fr.permute(1, 2, 0).numpy()).save(os.path.join(frames_dir, "frame_%04d.png" % k))
    common = ["--path", frames_dir, "--device", "cpu", "--small", "--iters", "2"]
    torch.manual_seed(0)
    dev = demo.main(common + ["--device_viz", "--output", str(tmp_path / "dev")])
    torch.manual_seed(0)
    host = demo.main(common + ["--output", str(tmp_path / "host")])
    assert len(dev) == len(host) == 2
    for a, b in zip(dev, host):
        assert open(a, "rb").read() == open(b, "rb").read()
