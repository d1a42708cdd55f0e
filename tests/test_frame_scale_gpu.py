"""Working-resolution inference on the GPU: the two HIP ops bitwise against their torch references
on the host copy of the same input, the equalities with the existing frame path at D = 1, graph
capture, and ``FlowInference(scale=2)`` against the hand composition.

Bitwise means ``torch.equal`` with NaN at the same positions (frame_scale_cases.same): both sides
run the same fp32 steps, each rounded on its own, so there is no tolerance to set.
"""
import numpy as np
import pytest
import torch

import frame_io_cases as fc
import frame_scale_cases as sc
from raft_ros_amd.ops.frame_io import ingest_frames
from raft_ros_amd.ops.frame_scale import ingest_frames_scaled, scaled_shape, upscale_flow
from raft_ros_amd.ros.node import FlowInference
from raft_ros_amd.utils.utils import InputPadder

pytestmark = pytest.mark.gpu


def _down(fr, D, pads, dev):
    return torch.ops.raft_amd.ingest_frames_scaled(fr.to(dev), D, *pads)


def _up(flow, geo, dev):
    return torch.ops.raft_amd.upscale_flow(flow.to(dev), *geo)


# ---------------------------------------------------------------------------- bitwise against the references
@pytest.mark.parametrize("pads", sc.PADS)
@pytest.mark.parametrize("shape,D", sc.GPU_SHAPES)
def test_downscale_bitwise(cuda, shape, D, pads):
    """D in {1, 2, 3, 4, 5, 8}: the templated and the looping factors; padded widths that are and
    are not multiples of 4; N = 2 and 3 with odd plane sizes (unaligned bases)."""
    for n in (1, 2, 3):
        fr, want = sc.down_case(shape, D, n, pads)
        got = _down(fr, D, pads, cuda)
        assert got.dtype == torch.float32 and got.device.type == "cuda"
        assert torch.equal(got.cpu(), want), f"{shape} D={D} N={n} pads={pads}"
    assert torch.equal(got[1:2].cpu(), _down(fr[1:2], D, pads, cuda).cpu())  # an image of a batch is that image alone


@pytest.mark.parametrize("pads", sc.PADS)
@pytest.mark.parametrize("shape,D", sc.GPU_SHAPES)
def test_upscale_bitwise(cuda, shape, D, pads):
    """Output widths 41, 70, 5, 17 (W % 4 != 0: scalar stores with a tail) and 24, 36, 40 (float4);
    B = 2 with odd planes (unaligned bases)."""
    for b in (1, 2):
        flow, geo, want = sc.up_case(shape, D, b, pads)
        got = _up(flow, geo, cuda)
        assert got.dtype == torch.float32 and got.shape == (b, 2) + shape and got.is_contiguous()
        assert sc.same(got, want), f"{shape} D={D} B={b} pads={pads}"
    assert torch.equal(got[1:2].cpu(), _up(flow[1:2].contiguous(), geo, cuda).cpu())


def test_vector_and_scalar_store_paths_are_both_taken():
    """The shapes above reach both store paths of both kernels."""
    down = {(sc.ceil_div(s[1], D) + p[0] + p[1]) % 4 == 0 for s, D in sc.GPU_SHAPES for p in sc.PADS}
    up = {s[1] % 4 == 0 for s, D in sc.GPU_SHAPES}
    assert down == {True, False} and up == {True, False}
    assert {D for _, D in sc.GPU_SHAPES} == {1, 2, 3, 4, 5, 8}


def test_upscale_nonfinite(cuda):
    hp, wp, left, top, w, h = sc.low_geometry((9, 13), 3, (1, 2, 3, 0))
    flow = sc.gaussian_flow(2, hp, wp, seed=11)
    flow[0, 0, top, left], flow[0, 1, top + h - 1, left + w - 1] = float("nan"), float("inf")
    flow[1, 0, top + 1, left + 2], flow[1, 0, top + 1, left + 3] = float("-inf"), float("-inf")
    flow[:, :, :top] = float("nan")  # the padding is never read
    geo = (3, left, top, w, h, 9, 13)
    want = sc.upscale_flow_ref(flow, *geo)
    assert want.isnan().any() and want.isinf().any()
    assert sc.same(_up(flow, geo, cuda), want)


def test_workload_downscale(cuda):
    fr, D, pads, want = sc.workload_down()
    got = _down(fr, D, pads, cuda)
    assert got.shape == (1, 3, 544, 960) and torch.equal(got.cpu(), want)
    out, padder = ingest_frames_scaled(fr.to(cuda), D)  # the wrapper picks the same padding
    assert tuple(padder._pad) == pads and torch.equal(out, got)


def test_workload_upscale(cuda):
    flow, geo, want = sc.workload_up()
    got = _up(flow, geo, cuda)
    assert got.shape == (1, 2, 1080, 1920) and sc.same(got, want)
    padder = InputPadder((540, 960))
    assert torch.equal(upscale_flow(flow.to(cuda), padder, 2, (1080, 1920)), got)


# ---------------------------------------------------------------------------- equalities with existing code
@pytest.mark.parametrize("mode", ["sintel", "kitti"])
def test_scale_one_is_the_existing_frame_path(cuda, mode):
    fr = sc.frames(2, 13, 17, seed=5).to(cuda)
    out, padder = ingest_frames_scaled(fr, 1, mode=mode)
    want, _ = ingest_frames(fr, mode=mode)
    assert torch.equal(out, want)
    for pads in ((1, 0, 2, 0), (0, 3, 0, 7), (7, 9, 6, 8)):
        assert torch.equal(torch.ops.raft_amd.ingest_frames_scaled(fr, 1, *pads),
                           torch.ops.raft_amd.ingest_frames(fr, *pads))
    flow = sc.gaussian_flow(2, 16, 24, seed=3).to(cuda)
    assert torch.equal(upscale_flow(flow, padder, 1, (13, 17)), padder.unpad(flow))


def test_op_argument_checks(cuda):
    down, up = torch.ops.raft_amd.ingest_frames_scaled, torch.ops.raft_amd.upscale_flow
    fr = torch.zeros(1, 8, 8, 3, device=cuda, dtype=torch.uint8)
    for args in ((fr.float(), 2, 0, 0, 0, 0), (fr, 0, 0, 0, 0, 0), (fr, 9, 0, 0, 0, 0), (fr, 2, -1, 0, 0, 0),
                 (fr[:, :, ::2], 2, 0, 0, 0, 0), (fr.cpu(), 2, 0, 0, 0, 0)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            down(*args)
    flow = torch.zeros(1, 2, 8, 8, device=cuda)
    up(flow, 2, 1, 1, 6, 6, 12, 12)
    for args in ((flow.half(), 2, 1, 1, 6, 6, 12, 12), (flow, 0, 1, 1, 6, 6, 12, 12), (flow, 9, 1, 1, 6, 6, 12, 12),
                 (flow, 2, 3, 1, 6, 6, 12, 12), (flow, 2, 1, 3, 6, 6, 12, 12), (flow, 2, -1, 1, 6, 6, 12, 12),
                 (flow, 2, 1, 1, 6, 6, 13, 12), (flow, 2, 1, 1, 6, 6, 12, 10), (flow, 2, 1, 1, 0, 6, 0, 12),
                 (flow[..., ::2], 2, 0, 0, 4, 6, 12, 8)):
        with pytest.raises(RuntimeError):
            up(*args)


# ---------------------------------------------------------------------------- graph capture
def test_graph_capture_and_two_replays(cuda):
    """Both ops in one captured graph, replayed twice on refilled inputs: each replay bitwise the
    reference of its own input."""
    shape, D, pads = (37, 41), 3, (1, 2, 3, 0)
    cases = [(sc.down_case(shape, D, n, pads), sc.up_case(shape, D, n, pads)) for n in (2, 3)]
    (fr0, _), (flow0, geo, _) = cases[0]
    s_fr = torch.zeros((2,) + tuple(fr0.shape[1:]), dtype=torch.uint8, device=cuda)
    s_flow = torch.zeros((2,) + tuple(flow0.shape[1:]), device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        torch.ops.raft_amd.ingest_frames_scaled(s_fr, D, *pads)
        torch.ops.raft_amd.upscale_flow(s_flow, *geo)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_down = torch.ops.raft_amd.ingest_frames_scaled(s_fr, D, *pads)
        c_up = torch.ops.raft_amd.upscale_flow(s_flow, *geo)
    for (fr, want_down), (flow, _, want_up) in cases:
        s_fr.copy_(fr[:2])
        s_flow.copy_(flow[:2])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c_down.cpu(), sc.ingest_frames_scaled_ref(fr[:2], D, pads))
        assert sc.same(c_up, sc.upscale_flow_ref(flow[:2], *geo))
    assert not torch.equal(cases[0][0][0][:2], cases[1][0][0][:2])  # the two replays saw different inputs


# ---------------------------------------------------------------------------- FlowInference
# The model refuses inputs below 128 x 128, so the frames are the smallest whose half is accepted:
# 249 x 299 -> 125 x 150 (both odd: partial last cells) -> padded to 128 x 152 (1 / 2 and 1 / 1).
HW = (249, 299)


def test_flow_inference_scale(cuda):
    """hip_graph on / off x device_io on / off: four flows, all equal and equal to the hand
    composition ingest -> runner -> upscale; with consistency and track the images are H x W and
    the points lie inside the frame."""
    rng = np.random.RandomState(0)
    a, b, c = [(rng.rand(*HW, 3) * 255).astype(np.uint8) for _ in range(3)]
    flows = []
    for hip_graph in (True, False):
        torch.manual_seed(0)
        inf = FlowInference(None, small=True, device="cuda", iters=2, hip_graph=hip_graph, scale=2,
                            consistency=True, track=True, track_cell=32)
        for device_io in (False, True):
            inf.device_io = device_io
            flow = inf.flow(a, b).clone()
            assert flow.shape == (1, 2) + HW and flow.device.type == "cuda"
            flows.append(flow)
            img = inf.visualize(a, b)
            assert img.shape == HW + (3,) and img.dtype == np.uint8
            fc.check_colors(img, fc.host_image(flow[0], bgr=True), f"graph {hip_graph} device_io {device_io}")
        images, padder = ingest_frames_scaled(torch.from_numpy(np.stack([a, b])).to(cuda), 2)
        assert images.shape == (2, 3, 128, 152) and scaled_shape(*HW, 2) == (125, 150)
        with torch.inference_mode():
            _, up = inf.runner(images[0:1], images[1:2])
            want = upscale_flow(up, padder, 2, HW)
        assert torch.equal(flows[-1], want)
        # consistency and tracks, device_io still on: everything on the camera frame
        img, mask, tr = inf.visualize_tracks(a, b, prev_stamp=1.0, curr_stamp=2.0)
        assert img.shape == HW + (3,) and mask.shape == HW and set(np.unique(mask).tolist()) <= {0, 128, 255}
        img2, mask2, tr2 = inf.visualize_tracks(b, c, prev_stamp=2.0, curr_stamp=3.0)
        assert img2.shape == HW + (3,) and inf._tracker.resets == 1 and tr2["age"].max() == 2
        for t in (tr, tr2):
            kept = t["status"] == 0
            assert t["points"].shape == (8 * 10, 2) and kept.any()
            for key in ("points", "prev"):
                x, y = t[key][kept, 0], t[key][kept, 1]
                assert (x >= 0).all() and (x <= HW[1] - 1).all() and (y >= 0).all() and (y <= HW[0] - 1).all()
    for f in flows[1:]:
        assert torch.equal(f, flows[0])
