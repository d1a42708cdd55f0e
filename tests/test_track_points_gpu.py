"""Point tracks on the GPU: the HIP op bitwise against the torch reference on the host copy of the
same inputs, chained over several steps on its own outputs; unaligned bases, batch independence,
the workload shape (determinism, graph capture), the argument checks and ``FlowInference.tracks``.

The specification fixes every rounding step, so no tolerance applies (track_cases.same: bitwise,
with a NaN equal to a NaN at the same place).
"""
import numpy as np
import pytest
import torch

import track_cases as tc
from raft_ros_amd.ops.track import seed_points, track_points, track_points_ref
from raft_ros_amd.ros.node import FlowInference

pytestmark = pytest.mark.gpu


def _host(inp):
    return tuple(t.cpu() if isinstance(t, torch.Tensor) else t for t in inp)


@pytest.mark.parametrize("use_bw", [True, False], ids=["bw", "no_bw"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_chain_against_the_reference(cuda, name, use_bw):
    """The kernel's own outputs feed the next step; every step is compared with the reference fed
    the same inputs."""
    log = tc.chain(track_points, name, use_bw, device=cuda)
    assert len(log) == tc.STEPS
    for k, (inp, out) in enumerate(log):
        assert all(o.device.type == "cuda" for o in out)
        tc.check(out, track_points_ref(*_host(inp)), f"{name} step {k}")
    if use_bw:  # the chain is the reference's own chain
        tc.check(log[-1][1], tc.reference_chain(name)[-1][1], f"{name} last step")


def test_unaligned_base_pointers(cuda):
    """Every input a slice of a larger tensor at an odd element offset."""
    (pos, ids, age, epoch, fw, bw, roi, S), want = tc.reference_chain("37x53_S8")[1]

    def odd(t):
        big = torch.zeros(t.numel() + 3, dtype=t.dtype, device=cuda)
        view = big[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view

    got = track_points(odd(pos), odd(ids), odd(age), odd(epoch), odd(fw), odd(bw), roi, S)
    tc.check(got, want, "odd offsets")


@pytest.mark.parametrize("name", ["37x53_S8", "64x96_S2"])
def test_a_batch_is_its_images_one_at_a_time(cuda, name):
    (pos, ids, age, epoch, fw, bw, roi, S), _ = tc.reference_chain(name)[2]
    dev = [t.to(cuda) for t in (pos, ids, age, epoch, fw, bw)]
    whole = track_points(*dev, roi, S)
    for b in range(pos.shape[0]):
        one = track_points(*[t[b:b + 1].contiguous() for t in dev[:3]], dev[3], dev[4][b:b + 1].contiguous(),
                           dev[5][b:b + 1].contiguous(), roi, S)
        for name_, o, w in zip(tc.NAMES, one, whole):
            assert tc.same(o, w if name_ == "epoch_out" else w[b:b + 1]), (b, name_)


def test_workload_shape_determinism_and_graph(cuda):
    """440 x 1024, S = 8, B = 2 once: two runs bitwise equal, the first step equal to the
    reference, and a captured graph that copies its outputs back into the state, replayed 3 times,
    equal to 3 eager steps."""
    B, H, W, roi, S, state, flows = tc.workload()
    flows = [(fw.to(cuda), bw.to(cuda)) for fw, bw in flows]
    s0 = [t.to(cuda) for t in state]
    first = track_points(*s0, *flows[0], roi, S)
    again = track_points(*s0, *flows[0], roi, S)
    assert all(tc.same(a, b) for a, b in zip(first, again))
    tc.check(first, track_points_ref(*state, flows[0][0].cpu(), flows[0][1].cpu(), roi, S), "440x1024 step 0")
    assert first[7].sum().item() == B * first[2].shape[1] and (first[7][:, :3] > 0).all()

    eager, st = [], s0
    for fw, bw in flows:
        out = track_points(*st, fw, bw, roi, S)
        eager.append(out)
        st = [out[0], out[2], out[3], out[4]]

    g_state = [t.clone() for t in s0]
    g_fw, g_bw = torch.zeros_like(flows[0][0]), torch.zeros_like(flows[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        track_points(*g_state, g_fw, g_bw, roi, S)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = track_points(*g_state, g_fw, g_bw, roi, S)
        for dst, src in zip(g_state, (captured[0], captured[2], captured[3], captured[4])):
            dst.copy_(src)
    for t, s in zip(g_state, s0):
        t.copy_(s)
    for k, (fw, bw) in enumerate(flows):
        g_fw.copy_(fw)
        g_bw.copy_(bw)
        graph.replay()
        torch.cuda.synchronize()
        tc.check(captured, eager[k], f"replay {k}")
        assert tc.same(g_state[0], eager[k][0]) and tc.same(g_state[3], eager[k][4])


def test_op_argument_checks(cuda):
    op = torch.ops.raft_amd.track_points
    roi, S = (0, 0, 16, 8), 4
    pos, ids, age, epoch = [t.to(cuda) for t in seed_points(1, roi, S)]
    f = torch.zeros(1, 2, 8, 16, device=cuda)
    good = (pos, ids, age, epoch, f, f, 0, 0, 16, 8, 4, 0.01, 0.5)
    out = op(*good)
    assert out[0].shape == (1, 8, 2) and out[5].dtype == torch.uint8 and out[7].tolist() == [[8, 0, 0, 0]]
    assert op(pos, ids, age, epoch, f, None, 0, 0, 16, 8, 4, 0.01, 0.5)[6].abs().sum() == 0

    def bad(**kw):
        names = ("pos", "ids", "age", "epoch", "flow_fw", "flow_bw", "left", "top", "w", "h", "S", "alpha1", "alpha2")
        args = [kw.get(n, g) for n, g in zip(names, good)]
        with pytest.raises(RuntimeError):
            op(*args)

    bad(pos=pos.double())
    bad(pos=pos[:, :7].contiguous())                  # N is not the grid's cell count
    bad(pos=torch.zeros(1, 8, 4, device=cuda)[..., ::2])  # not contiguous
    bad(ids=ids.int())
    bad(age=age.long())
    bad(epoch=epoch.int())
    bad(epoch=torch.ones(2, dtype=torch.int64, device=cuda))
    bad(flow_fw=f.half())
    bad(flow_bw=f.half())
    bad(flow_bw=torch.zeros(1, 2, 16, 8, device=cuda))
    bad(flow_fw=torch.zeros(1, 2, 8, 32, device=cuda)[..., ::2])
    bad(flow_bw=f.cpu())
    bad(pos=pos.cpu())
    bad(ids=ids.cpu())
    bad(w=17)            # the roi leaves the frame
    bad(left=1)
    bad(top=-1)
    bad(h=0)
    bad(w=0)
    bad(S=0)
    bad(S=8)             # another grid: 2 cells, not 8
    # B = 0: empty outputs, the epoch still advances
    e = op(torch.zeros(0, 8, 2, device=cuda), torch.zeros(0, 8, dtype=torch.int64, device=cuda),
           torch.zeros(0, 8, dtype=torch.int32, device=cuda), epoch, torch.zeros(0, 2, 8, 16, device=cuda), None,
           0, 0, 16, 8, 4, 0.01, 0.5)
    assert e[0].shape == (0, 8, 2) and e[5].shape == (0, 8) and e[7].shape == (0, 4) and e[4].item() == 2
    # the Python layer raises ValueError before the op is reached
    with pytest.raises(ValueError):
        track_points(pos, ids, age, epoch, f, f, (0, 0, 17, 8), 4)
    with pytest.raises(ValueError):
        track_points(pos, ids, age, epoch.cpu(), f, f, roi, 4)


def test_flow_inference_tracks_device_io(cuda):
    """Random-weight RAFT-small, 124 x 150 frames (padded to 128 x 152): the same instance with
    ``device_io`` on and off gives the same flow and the same tracks, bitwise."""
    rng = np.random.RandomState(0)
    frames = [(rng.rand(124, 150, 3) * 255).astype(np.uint8) for _ in range(3)]
    results = []
    for device_io in (True, False):
        torch.manual_seed(0)
        inf = FlowInference(None, small=True, device="cuda", iters=2, consistency=True, track=True, track_cell=16,
                            device_io=device_io)
        run = []
        for k in range(2):
            flow, tr = inf.tracks(frames[k], frames[k + 1], prev_stamp=float(k), curr_stamp=float(k + 1))
            run.append((flow.clone(), tr))
        results.append(run)
        assert inf._tracker.resets == 1  # the second pair continued the first
    for (flow_a, a), (flow_b, b) in zip(*results):
        assert flow_a.shape == (1, 2, 128, 152) and torch.equal(flow_a, flow_b)
        assert set(a) == {"points", "prev", "ids", "age", "status"}
        N = 8 * 10
        assert a["points"].shape == (N, 2) and a["ids"].shape == (N,) and a["status"].dtype == np.uint8
        for key in a:
            assert a[key].dtype == b[key].dtype and a[key].flags.owndata
            assert tc.same(torch.from_numpy(a[key]), torch.from_numpy(b[key])), key
        keep = a["status"] == 0
        pts = a["points"][keep]  # image coordinates: inside the unpadded image
        assert (pts[:, 0] >= 0).all() and (pts[:, 0] <= 149).all() and (pts[:, 1] >= 0).all() and (pts[:, 1] <= 123).all()
        assert np.isnan(a["prev"][~keep]).all() and not np.isnan(a["prev"][keep]).any()
    assert len(set(results[0][1][1]["ids"].tolist())) == 80
