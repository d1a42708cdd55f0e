"""HIP forward splat (csrc/forward_splat.hip) against the brute-force fp64 oracle, bitwise: the op
only selects input values.  Inputs: tests/warm_start_cases.py."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import warm_start_cases as wc
from raft_ros_amd.ops.warm_start import forward_splat_nearest

pytestmark = pytest.mark.gpu

MAX_EXCLUDED = 0.01


def _check(cuda, name, shape):
    f = wc.case(name, shape)
    got = forward_splat_nearest(f.to(cuda))
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == f.shape
    got = got.cpu()
    want = wc.oracle(name, shape)[0]
    assert torch.equal(got, want), (name, shape, int((got != want).any(1).sum()), "pixels differ")
    return got


@pytest.mark.parametrize("shape", wc.SHAPES)
@pytest.mark.parametrize("name", wc.RANDOM)
def test_random_flows(cuda, name, shape):  # (a)
    _check(cuda, name, shape)


@pytest.mark.parametrize("shape", wc.SHAPES)
def test_no_valid_point_gives_zeros(cuda, shape):  # (b)
    assert not _check(cuda, "all_out", shape).any()
    got = _check(cuda, "out_and_normal", shape)
    assert not got[0].any() and got[1].any()


@pytest.mark.parametrize("shape", wc.SHAPES)
def test_single_valid_point_fills_the_image(cuda, shape):  # (c)
    got = _check(cuda, "one_point", shape)
    assert (got[0, 0] == 0.5).all() and (got[0, 1] == -0.25).all()
    assert (got[1, 0] == -0.5).all() and (got[1, 1] == 0.25).all()


@pytest.mark.parametrize("shape", wc.SHAPES)
@pytest.mark.parametrize("name", sorted(wc.RING_TIES))
def test_ring_boundary_tie_goes_to_the_lower_index(cuda, name, shape):  # (d)
    _, (xt, yt), expect = wc.RING_TIES[name]
    got = _check(cuda, "ring_" + name, shape)
    assert tuple(got[0, :, yt, xt].tolist()) == expect


@pytest.mark.parametrize("shape", wc.SHAPES)
@pytest.mark.parametrize("name", ["half_steps", "constant", "zero_with_block"])
def test_tie_heavy_inputs(cuda, name, shape):  # (e)
    _check(cuda, name, shape)


@pytest.mark.parametrize("shape", wc.SHAPES)
def test_collapse_into_one_cell(cuda, shape):  # (f)
    f = wc.case("collapse", shape)[0]
    H, W = shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cells = (ys + f[1]).floor().long() * W + (xs + f[0]).floor().long()
    assert cells.reshape(-1).bincount().max() > 64
    _check(cuda, "collapse", shape)


@pytest.mark.parametrize("shape", wc.SHAPES)
def test_non_finite_flows_are_invalid(cuda, shape):  # (g)
    assert torch.isfinite(_check(cuda, "non_finite", shape)).all()


def test_deterministic(cuda):  # (h)
    f = wc.case("half_steps", (17, 23)).to(cuda)
    outs = [forward_splat_nearest(f) for _ in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_graph_capture_has_no_host_dependence(cuda):  # (i)
    shape = (17, 23)
    static = wc.case("all_out", shape).to(cuda)  # captured with no valid point at all
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        forward_splat_nearest(static)  # allocator warm-up outside the capture
    torch.cuda.current_stream(cuda).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = forward_splat_nearest(static)
    for name in ("random12", "out_and_normal", "one_point"):  # the number of valid points changes
        static.copy_(wc.case(name, shape))
        graph.replay()
        assert torch.equal(out.cpu(), wc.oracle(name, shape)[0]), name


@pytest.mark.parametrize("shape", wc.SHAPES)
@pytest.mark.parametrize("name", wc.RANDOM)
def test_matches_scipy_forward_interpolate(cuda, name, shape):  # (j)
    got = forward_splat_nearest(wc.case(name, shape).to(cuda)).cpu()
    keep = wc.oracle(name, shape)[1] >= 1e-9
    excluded = 1.0 - keep.double().mean().item()
    print(f"{name} {shape}: excluded {excluded:.4f}")
    assert excluded <= MAX_EXCLUDED
    keep = keep[:, None].expand_as(got)
    assert torch.equal(got[keep], wc.scipy_result(name, shape)[keep])


def test_sintel_submission_warm_start_stays_on_the_device(cuda, tmp_path, monkeypatch):
    """create_sintel_submission(warm_start=True) on a GPU: the HIP splat, not the CPU round trip."""
    from raft_ros_amd.data.synthetic import demo_sequence
    from raft_ros_amd.eval import validate
    from raft_ros_amd.models import RAFT

    frames = [f.float() for f in demo_sequence(3, 128, 160)]

    class FakeSintel:
        def __init__(self, split, aug_params, dstype):
            pass

        def __len__(self):
            return 2

        def __getitem__(self, i):
            return frames[i], frames[i + 1], ("seq", i)

    seen = []

    def splat(flow):
        seen.append(flow.device.type)
        return forward_splat_nearest(flow)

    def no_scipy(flow):
        raise AssertionError("forward_interpolate called on the GPU path")

    monkeypatch.setattr(validate.datasets, "MpiSintel", FakeSintel)
    monkeypatch.setattr(validate, "forward_splat_nearest", splat)
    monkeypatch.setattr(validate, "forward_interpolate", no_scipy)
    torch.manual_seed(0)
    model = RAFT(Namespace(small=True, mixed_precision=False, alternate_corr=False)).to(cuda)
    validate.create_sintel_submission(model, iters=2, warm_start=True, output_path=str(tmp_path))
    assert seen == ["cuda"] * 4  # 2 pairs x (clean, final)
    assert sorted(p.name for p in (tmp_path / "clean" / "seq").iterdir()) == ["frame0001.flo", "frame0002.flo"]


@pytest.mark.parametrize("small", [True, False])
def test_flow_inference_warm_start_end_to_end(cuda, small):  # (k)
    from raft_ros_amd.data.synthetic import demo_sequence
    from raft_ros_amd.ros.node import FlowInference

    torch.manual_seed(0)
    inf = FlowInference(None, small=small, device="cuda", iters=4, warm_start=True, hip_graph=True)
    frames = [np.ascontiguousarray(f.permute(1, 2, 0).numpy()) for f in demo_sequence(3, 128, 160)]
    to_t = lambda x: torch.from_numpy(x).permute(2, 0, 1).float()[None].to(cuda)  # noqa: E731
    i0, i1, i2 = map(to_t, frames)
    with torch.no_grad():
        low_prev, _ = inf.model(i0, i1, iters=4, test_mode=True)
        init = forward_splat_nearest(low_prev)
        _, want = inf.model(i1, i2, iters=4, flow_init=init, test_mode=True)
    inf.flow(frames[0], frames[1], prev_stamp=0.0, curr_stamp=1.0)
    got = inf.flow(frames[1], frames[2], prev_stamp=1.0, curr_stamp=2.0)
    torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-3)
    assert inf.runner.num_graphs == 2  # one cold, one warm
