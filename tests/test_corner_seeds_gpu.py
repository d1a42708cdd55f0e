"""Corner seeds on the GPU: the HIP op bitwise against the torch reference on the host copy of the
same frames (every case of the CPU tests, every row alignment, frames smaller than the footprint),
unaligned bases, batch independence, the seeded tracker chained on its own outputs, the workload
shape (determinism, graph capture with the tracker), the argument checks of both new ops and
``FlowInference(track_seeds="corners")``.

The specification is in integers, so no tolerance applies: every comparison is bitwise."""
import numpy as np
import pytest
import torch

import corner_cases as cc
import track_cases as tc
from raft_ros_amd.ops.corners import corner_seeds, corner_seeds_ref
from raft_ros_amd.ops.track import seed_points, track_points, track_points_ref
from raft_ros_amd.ros.node import FlowInference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S", cc.CELLS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_op_against_the_reference(cuda, shape, S):
    H, W = shape
    f = cc.frames(H, W)
    dev = f.to(cuda)
    for kw in cc.variants(H, W, S):
        for B in (1, 3):
            got = corner_seeds(dev[:B], S, **kw)
            assert all(t.device.type == "cuda" for t in got)
            cc.same_pair(got, corner_seeds_ref(f[:B], S, **kw), f"{kw} B={B}")
        empty = corner_seeds(dev[:0], S, **kw)
        assert empty[0].shape[0] == 0 and empty[0].shape[1:] == got[0].shape[1:] and empty[1].shape[0] == 0


# widths whose rows of 3 W bytes start at every alignment, sizes around the 64 x 16 tile and
# frames smaller than the 5 x 5 footprint
ODD_SHAPES = [(9, 50), (9, 51), (9, 53), (9, 64), (17, 65), (33, 131), (16, 64), (15, 63), (97, 131), (1, 7), (3, 3),
              (4, 2), (2, 1), (70, 1), (1, 130)]


@pytest.mark.parametrize("shape", ODD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_row_alignments_tile_edges_and_tiny_frames(cuda, shape):
    H, W = shape
    f = cc.frames(H, W)
    assert len({(3 * w) % 4 for _, w in ODD_SHAPES[:4]}) == 4
    dev = f.to(cuda)
    for S in (1, 5, 8, 32, 200):
        for margin in cc.margins(S):
            cc.same_pair(corner_seeds(dev, S, margin=margin), corner_seeds_ref(f, S, margin=margin), f"S={S} m={margin}")
    if H > 2 and W > 3:
        kw = dict(roi_size=(W - 3, H - 2), origin=(4, 1), margin=0)
        cc.same_pair(corner_seeds(dev, 7, **kw), corner_seeds_ref(f, 7, **kw), "roi")


def test_patterns(cuda):
    """Extremes and ties: checkerboards (equal maxima: the lowest index), stripes and constants
    (score 0: every seed a centre), one square per cell, the largest contrast."""
    g = torch.Generator().manual_seed(3)
    pats = [cc.checkerboard(24, 40, 1), cc.checkerboard(24, 40, 2), cc.stripes(24, 40, 1), cc.stripes(24, 40, 2, False),
            cc.gray_frame(torch.full((24, 40), 131)), cc.squares(48, 64, 16),
            cc.gray_frame(torch.randint(0, 2, (31, 33), generator=g) * 255)]
    for k, f in enumerate(pats):
        for S in (8, 16):
            for margin in (0, None):
                cc.same_pair(corner_seeds(f.to(cuda), S, margin=margin), corner_seeds_ref(f, S, margin=margin),
                             f"pattern {k} S={S}")
    f = cc.frames(37, 53)
    cc.same_pair(corner_seeds(f.flip(-1).contiguous().to(cuda), 8), corner_seeds_ref(f, 8), "BGR")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_base(cuda, offset):
    """The frames a slice of a larger byte buffer."""
    for H, W in ((37, 53), (9, 50), (33, 131)):
        f = cc.frames(H, W)
        big = torch.zeros(f.numel() + 8, dtype=torch.uint8, device=cuda)
        view = big[offset:offset + f.numel()].view(f.shape)
        view.copy_(f)
        assert view.is_contiguous() and view.data_ptr() % 4 == offset
        cc.same_pair(corner_seeds(view, 8), corner_seeds_ref(f, 8), f"offset {offset}")


def test_a_batch_is_its_images_one_at_a_time(cuda):
    for (H, W), S in (((37, 53), 8), ((64, 96), 4), ((97, 131), 16)):
        dev = cc.frames(H, W).to(cuda)
        whole = corner_seeds(dev, S)
        for b in range(3):
            one = corner_seeds(dev[b:b + 1].contiguous(), S)
            assert tc.same(one[0], whole[0][b:b + 1]) and tc.same(one[1], whole[1][b:b + 1])


def test_seeded_tracker_chain(cuda):
    """``track_points(seeds=...)`` chained on its own outputs against the reference fed the same
    inputs; the seeds are the corners of a moving texture, found on the device."""
    name = "37x53_S8"
    B, H, W, roi, S = tc.CASES[name]
    tex = cc.moving_texture()
    assert cc.fallback_share(tex[0], S, None) < 0.05  # the condition: corners exist
    seeds = [corner_seeds(t.to(cuda), S)[0] for t in tex]
    for t, s in zip(tex, seeds):
        assert tc.same(s, corner_seeds_ref(t, S)[0])
    _, _, _, _, _, _, flows = tc.case(name)
    state = [t.to(cuda) for t in seed_points(B, roi, S, seeds=seeds[0].cpu())]
    fresh = moved = 0
    for k, (fw, bw) in enumerate(flows):
        fw, bw = fw.to(cuda), bw.to(cuda)
        out = track_points(*state, fw, bw, roi, S, seeds=seeds[k + 1])
        want = track_points_ref(*[t.cpu() for t in state], fw.cpu(), bw.cpu(), roi, S, seeds=seeds[k + 1].cpu())
        tc.check(out, want, f"step {k}")
        plain = track_points(*state, fw, bw, roi, S)
        for name_, o, p in zip(tc.NAMES[1:], out[1:], plain[1:]):
            assert tc.same(o, p), name_  # the seeds move the fresh points and nothing else
        fresh += int((out[3] == 0).sum())
        moved += int((out[0] != plain[0]).any(dim=-1).sum())
        state = [out[0], out[2], out[3], out[4]]
    assert fresh > 0 and moved > 0


def test_workload_shape_determinism_and_graph(cuda):
    """440 x 1024, B = 2, S = 8: two runs bitwise equal and equal to the reference; a captured graph
    of ``corner_seeds`` followed by ``track_points``, replayed 3 times with new frames and flows
    copied into static buffers, equals the eager steps."""
    B, H, W, roi, S, state, flows = tc.workload()
    g = torch.Generator().manual_seed(7)
    low = torch.randint(0, 256, (3, B, H // 4, W // 4, 3), generator=g, dtype=torch.uint8)
    frames = [f.repeat_interleave(4, dim=1).repeat_interleave(4, dim=2).contiguous() for f in low]
    frames[0][:, :, : W // 2] = torch.randint(0, 256, (B, H, W // 2, 3), generator=g, dtype=torch.uint8)
    dev_frames = [f.to(cuda) for f in frames]
    first, again = corner_seeds(dev_frames[0], S), corner_seeds(dev_frames[0], S)
    assert tc.same(first[0], again[0]) and tc.same(first[1], again[1])
    want = corner_seeds_ref(frames[0], S)
    cc.same_pair(first, want, "440x1024")
    assert float((want[1] <= 0).sum()) / want[1].numel() < 0.5 and (want[1] > 0).any()

    flows = [(fw.to(cuda), bw.to(cuda)) for fw, bw in flows]
    s0 = [t.to(cuda) for t in state]

    def step(st, frm, fw, bw):
        seeds, score = corner_seeds(frm, S)
        return track_points(*st, fw, bw, roi, S, seeds=seeds) + (seeds, score)

    eager, st = [], s0
    for frm, (fw, bw) in zip(dev_frames, flows):
        out = step(st, frm, fw, bw)
        eager.append(out)
        st = [out[0], out[2], out[3], out[4]]
    assert sum(int((o[3] == 0).sum()) for o in eager) > 0

    g_state = [t.clone() for t in s0]
    g_frm, g_fw, g_bw = torch.zeros_like(dev_frames[0]), torch.zeros_like(flows[0][0]), torch.zeros_like(flows[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(g_state, g_frm, g_fw, g_bw)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(g_state, g_frm, g_fw, g_bw)
        for dst, src in zip(g_state, (captured[0], captured[2], captured[3], captured[4])):
            dst.copy_(src)
    for t, s in zip(g_state, s0):
        t.copy_(s)
    for k, (frm, (fw, bw)) in enumerate(zip(dev_frames, flows)):
        g_frm.copy_(frm)
        g_fw.copy_(fw)
        g_bw.copy_(bw)
        graph.replay()
        torch.cuda.synchronize()
        tc.check(captured[:8], eager[k][:8], f"replay {k}")
        assert tc.same(captured[8], eager[k][8]) and tc.same(captured[9], eager[k][9])


def test_argument_checks_of_both_ops(cuda):
    op = torch.ops.raft_amd.corner_seeds
    f = cc.frames(37, 53).to(cuda)
    good = (f, 8, 53, 37, 0, 0, 2, 0)
    seeds, score = op(*good)
    assert seeds.shape == (3, 35, 2) and seeds.dtype == torch.float32 and score.shape == (3, 35) and score.dtype == torch.int32

    def bad(**kw):
        names = ("frames", "S", "w", "h", "left", "top", "margin", "min_score")
        with pytest.raises(RuntimeError):
            op(*[kw.get(n, g) for n, g in zip(names, good)])

    bad(frames=f.float())
    bad(frames=f.cpu())
    bad(frames=f[..., :2])
    bad(frames=f[:, :, ::2])
    bad(frames=f[0])
    bad(S=0)
    bad(S=-1)
    bad(margin=4)        # 2 * margin > S - 1
    bad(margin=-1)
    bad(S=1, margin=1)
    bad(w=54)
    bad(h=38)
    bad(w=0)
    bad(left=1 << 24)
    e = op(f[:0], 8, 53, 37, 0, 0, 2, 0)
    assert e[0].shape == (0, 35, 2) and e[1].shape == (0, 35)
    with pytest.raises(ValueError):  # the Python layer raises before the op is reached
        corner_seeds(f, 8, margin=4)
    with pytest.raises(ValueError):
        corner_seeds(f, 0)
    with pytest.raises(ValueError):
        corner_seeds(f.float(), 8)

    top = torch.ops.raft_amd.track_points_seeded
    roi, S = (0, 0, 16, 8), 4
    pos, ids, age, epoch = [t.to(cuda) for t in seed_points(1, roi, S)]
    fl = torch.zeros(1, 2, 8, 16, device=cuda)
    sd = pos.clone()
    good_t = (pos, ids, age, epoch, fl, fl, sd, 0, 0, 16, 8, 4, 0.01, 0.5)
    out = top(*good_t)
    assert out[0].shape == (1, 8, 2) and out[7].tolist() == [[8, 0, 0, 0]]
    assert top(pos, ids, age, epoch, fl, None, sd, 0, 0, 16, 8, 4, 0.01, 0.5)[6].abs().sum() == 0

    def bad_t(**kw):
        names = ("pos", "ids", "age", "epoch", "flow_fw", "flow_bw", "seeds", "left", "top", "w", "h", "S", "alpha1",
                 "alpha2")
        with pytest.raises(RuntimeError):
            top(*[kw.get(n, g) for n, g in zip(names, good_t)])

    bad_t(seeds=sd.double())
    bad_t(seeds=sd.cpu())
    bad_t(seeds=sd[:, :7].contiguous())                      # not the grid's cell count
    bad_t(seeds=torch.zeros(1, 8, 3, device=cuda))
    bad_t(seeds=torch.zeros(1, 8, 4, device=cuda)[..., ::2])  # not contiguous
    bad_t(seeds=torch.zeros(2, 8, 2, device=cuda))
    bad_t(pos=pos.double())
    bad_t(S=0)
    bad_t(S=8)
    bad_t(w=17)
    with pytest.raises(ValueError):
        track_points(pos, ids, age, epoch, fl, fl, roi, S, seeds=sd[:, :7].contiguous())
    with pytest.raises(ValueError):
        track_points(pos, ids, age, epoch, fl, fl, roi, S, seeds=sd.cpu())


@pytest.mark.parametrize("scale", [1, 2])
def test_flow_inference_corner_seeds_device_io(cuda, scale):
    """Random-weight RAFT-small; ``device_io`` on and off give the same flow and the same tracks,
    bitwise: 124 x 150 frames (padded to 128 x 152), and 250 x 300 frames with ``scale = 2``."""
    rng = np.random.RandomState(0)
    H, W = (124, 150) if scale == 1 else (250, 300)
    frames = [(rng.rand(H, W, 3) * 255).astype(np.uint8) for _ in range(3)]
    ref_seeds, ref_score = corner_seeds_ref(torch.from_numpy(np.stack(frames[:2])), 16)
    assert float((ref_score <= 0).sum()) / ref_score.numel() < 0.05  # the condition: corners exist
    results = []
    for device_io in (True, False):
        torch.manual_seed(0)
        inf = FlowInference(None, small=True, device="cuda", iters=2, consistency=True, track=True, track_cell=16,
                            device_io=device_io, track_seeds="corners", **(dict(scale=2) if scale == 2 else {}))
        run = []
        for k in range(2):
            flow, tr = inf.tracks(frames[k], frames[k + 1], prev_stamp=float(k), curr_stamp=float(k + 1))
            run.append((flow.clone(), tr))
        results.append(run)
        assert inf._tracker.resets == 1
    for (flow_a, a), (flow_b, b) in zip(*results):
        assert torch.equal(flow_a, flow_b)
        assert list(a) == ["points", "prev", "ids", "age", "status", "score"]
        for key in a:
            assert a[key].dtype == b[key].dtype and a[key].flags.owndata
            assert tc.same(torch.from_numpy(a[key]), torch.from_numpy(b[key])), key
    # the first pair's survivors started on the first frame's corners, with their scores
    tr = results[0][0][1]
    keep = tr["status"] == 0
    assert keep.any() and np.array_equal(tr["prev"][keep], ref_seeds[0].numpy()[keep])
    assert np.array_equal(tr["score"][keep], ref_score[0].numpy()[keep])
