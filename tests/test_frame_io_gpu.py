"""Device-side frame path on the GPU: the HIP colour coding against numpy ``flow_viz`` on the host
copy of the same flow, the HIP frame ingest bitwise against ``F.pad``, and ``FlowInference`` with
``device_io``.

The colour rule (frame_io_cases.check_colors): every channel within 1 level and at most
max(1, 1e-3 * H * W) pixels of an image differ at all.  The op rounds like numpy up to the last
bit of ``arctan2``, which moves ``floor(255 * col)`` by one level on rare pixels; a wrong hue end,
a wrong per-image maximum or a wrong channel order changes tens of levels on most pixels.
"""
import os

import numpy as np
import pytest
import torch

import frame_io_cases as fc
from raft_ros_amd.ops.frame_io import flow_to_image, ingest_frames
from raft_ros_amd.ros.node import FlowInference

pytestmark = pytest.mark.gpu


def _check_batch(flow, dev, clip_flow=None, bgr=False, what=""):
    """flow (B, 2, H, W) on the host -> the op's images, each checked against its own host image."""
    out = flow_to_image(flow.to(dev), clip_flow=clip_flow, convert_to_bgr=bgr)
    assert out.device.type == "cuda" and out.dtype == torch.uint8
    assert out.shape == (flow.shape[0],) + tuple(flow.shape[2:]) + (3,)
    out = out.cpu()
    for b in range(flow.shape[0]):
        fc.check_colors(out[b], fc.host_image(flow[b], clip_flow, bgr), f"{what}[{b}]")
    return out


# ---------------------------------------------------------------------------- colour coding
@pytest.mark.parametrize("bgr", [False, True])
def test_parity_field_and_recorded_reference(cuda, bgr):
    f = fc.parity_flow()
    out = _check_batch(f[None], cuda, bgr=bgr, what="37x41")
    fix = np.load(os.path.join(fc.golden.GOLDEN, "flow_viz.npz"))
    fc.check_colors(out[0], fix["bgr" if bgr else "rgb"], "37x41 vs recorded reference")
    one = flow_to_image(f.to(cuda), convert_to_bgr=bgr)  # (2, H, W) in, (H, W, 3) out
    assert one.shape == (37, 41, 3) and torch.equal(one.cpu(), out[0])


def test_batch_has_per_image_maxima_and_unaligned_bases(cuda):
    f = fc.scaled_batch()
    assert (37 * 41 * 3) % 4 != 0
    out = _check_batch(f, cuda, what="B=3 scales 1/5/40")
    for b in range(3):  # an image of a batch is that image alone
        assert torch.equal(flow_to_image(f[b].to(cuda)).cpu(), out[b])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 3)])
def test_packed_store_tails(cuda, shape):
    _check_batch(fc.gaussian(*shape, 3.0, seed=2)[None], cuda, what=f"{shape}")
    _check_batch(torch.stack([fc.gaussian(*shape, s, seed=5) for s in (1.0, 9.0)]), cuda, what=f"B=2 {shape}")


@pytest.mark.parametrize("shape", [(1, 1, 5, 7), (2, 1, 16, 16)])
def test_zero_flow_is_white(cuda, shape):
    B, _, H, W = shape
    out = flow_to_image(torch.zeros(B, 2, H, W, device=cuda))
    assert (out == 255).all()


def test_axes_wrap_and_signed_zeros(cuda):
    f = fc.axes_field()
    want = fc.host_image(f)
    # numpy tells v = +0.0 (row 8) from v = -0.0 (row 15) at u > 0: the two ends of the wheel, 43
    # levels apart in blue at full saturation, 43 * 4 / sqrt(128) = 15 at u = 4 of this field
    assert abs(int(want[8, 12, 2]) - int(want[15, 12, 2])) >= 14
    out = _check_batch(f[None], cuda, what="axes 16x16")
    assert np.array_equal(out[0, 8].numpy(), want[8]) and np.array_equal(out[0, 15].numpy(), want[15])
    _check_batch(f[None], cuda, bgr=True, what="axes 16x16 bgr")


def test_single_outlier(cuda):
    out = _check_batch(fc.outlier_field()[None], cuda, what="outlier 64x64")
    assert (out[0].float().mean() > 250) and out[0].min() < 200  # near white, except the outlier itself


def test_clip_flow(cuda):
    f = fc.parity_flow()[None]
    _check_batch(f, cuda, clip_flow=3.0, what="clip 3.0")
    _check_batch(f, cuda, clip_flow=3.0, bgr=True, what="clip 3.0 bgr")


def test_workload_shape_determinism_and_graph(cuda):
    """440 x 1024 once: the colour rule, two calls bitwise equal, and a captured graph replayed on a
    refilled input equal to the eager result."""
    f, want = fc.workload()
    d = f.to(cuda)[None]
    out = flow_to_image(d)
    fc.check_colors(out[0], want, "440x1024 sigma=8")
    assert torch.equal(flow_to_image(d), out)

    static = torch.zeros_like(d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flow_to_image(static)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = flow_to_image(static)
    static.copy_(d)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, out)


def test_determinism_small_unaligned(cuda):
    d = fc.scaled_batch().to(cuda)
    assert torch.equal(flow_to_image(d), flow_to_image(d))


def test_nonfinite_flow_returns(cuda):
    f = fc.nonfinite_field()
    out = flow_to_image(torch.stack([f, fc.gaussian(9, 13, 4.0, seed=6)]).to(cuda))
    torch.cuda.synchronize()
    assert out.shape == (2, 9, 13, 3)
    # the other image of the batch does not see them
    fc.check_colors(out[1], fc.host_image(fc.gaussian(9, 13, 4.0, seed=6)), "beside a non-finite image")


def test_op_argument_checks(cuda):
    op = torch.ops.raft_amd.flow_to_image
    with pytest.raises(RuntimeError):
        op(torch.zeros(1, 2, 4, 4, device=cuda, dtype=torch.float16), None, False)
    with pytest.raises(RuntimeError):
        op(torch.zeros(1, 2, 4, 8, device=cuda)[..., ::2], None, False)
    with pytest.raises(RuntimeError):
        torch.ops.raft_amd.ingest_frames(torch.zeros(1, 4, 4, 3, device=cuda), 0, 0, 0, 0)
    with pytest.raises(RuntimeError):
        torch.ops.raft_amd.ingest_frames(torch.zeros(1, 4, 4, 3, device=cuda, dtype=torch.uint8), -1, 0, 0, 0)
    # non-contiguous or half-precision flow goes through the Python layer's conversion
    f = fc.gaussian(6, 10, 3.0)
    fc.check_colors(flow_to_image(f.to(cuda).half()).cpu(), fc.host_image(f.half().float()), "fp16 flow")


# ---------------------------------------------------------------------------- ingest
@pytest.mark.parametrize("n,h,w,mode,pads", [
    (1, 13, 17, "sintel", (3, 4, 1, 2)),
    (1, 13, 17, "kitti", (3, 4, 0, 3)),
    (1, 16, 24, "sintel", (0, 0, 0, 0)),
    (1, 1, 1, "sintel", (3, 4, 3, 4)),
    (2, 13, 17, "sintel", (3, 4, 1, 2)),
])
def test_ingest_bitwise(cuda, n, h, w, mode, pads):
    fr = fc.frames(n, h, w, seed=h * w + n)
    out, padder = ingest_frames(fr.to(cuda), mode=mode)
    assert tuple(padder._pad) == pads and out.device.type == "cuda" and out.dtype == torch.float32
    assert torch.equal(out.cpu(), fc.pad_ref(fr, pads))
    assert torch.equal(padder.unpad(out).cpu(), fr.permute(0, 3, 1, 2).float())


def test_ingest_op_any_padding(cuda):
    """The op itself: a padded width that is no multiple of 4 (scalar stores) and pads beyond the frame."""
    fr = fc.frames(2, 5, 6, seed=9)
    for pads in ((1, 0, 2, 0), (0, 3, 0, 7), (7, 9, 6, 8)):
        out = torch.ops.raft_amd.ingest_frames(fr.to(cuda), *pads)
        assert torch.equal(out.cpu(), fc.pad_ref(fr, pads))


# ---------------------------------------------------------------------------- FlowInference
def test_flow_inference_device_io(cuda):
    """Random-weight RAFT-small; 124 x 150 frames (padded to 128 x 152: 2/2 and 1/1), the smallest
    the model accepts (it refuses inputs below 128 x 128).  One instance, the option switched: the
    same weights and the same captured graph."""
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cuda", iters=2)
    rng = np.random.RandomState(0)
    a, b, c = [(rng.rand(124, 150, 3) * 255).astype(np.uint8) for _ in range(3)]
    for k, (p, q) in enumerate(((a, b), (b, c), (c, a))):  # later calls reuse the pinned buffers
        inf.device_io = False
        want_flow = inf.flow(p, q).clone()
        want_img = inf.visualize(p, q)
        inf.device_io = True
        got_flow = inf.flow(p, q).clone()
        assert got_flow.shape == (1, 2, 128, 152) and torch.equal(got_flow, want_flow)
        got_img = inf.visualize(p, q)
        assert got_img.flags.owndata and got_img.flags.c_contiguous
        fc.check_colors(got_img, want_img, f"visualize, pair {k}")
        # against numpy on the very same flow, BGR
        fc.check_colors(got_img, fc.host_image(want_flow[0], bgr=True), f"visualize vs host, pair {k}")
    first = inf.visualize(a, b)
    second = inf.visualize(b, c)  # the returned image owns its memory: the next call does not change it
    assert first.tobytes() == inf.visualize(a, b).tobytes() and second.tobytes() != first.tobytes()
