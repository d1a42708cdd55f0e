"""Corner seeds on the CPU: the torch reference against a per-pixel loop on Python ints, the extremes
and ties of the score, the tracker with seeds against a per-slot loop, and the consumers
(PointTracker, FlowInference, the ROS node with fakes, demo.py --track_seeds corners).

Everything is in integers (or moves fp32 values unchanged), so every comparison is bitwise."""
import csv
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

import corner_cases as cc
import track_cases as tc
from raft_ros_amd.ops.corners import corner_score_ref, corner_seeds, corner_seeds_ref, slot_scores
from raft_ros_amd.ops.track import PointTracker, _seed_xy, grid_shape, seed_points, track_points, track_points_ref
from raft_ros_amd.ros.node import FlowInference, RaftRosNode


# ---------------------------------------------------------------------------- reference against the loop
@pytest.mark.parametrize("S", cc.CELLS)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_reference_is_the_per_pixel_loop(shape, S):
    H, W = shape
    f = cc.frames(H, W)
    for kw in cc.variants(H, W, S):
        for B in (1, 3):
            got = corner_seeds_ref(f[:B], S, **kw)
            want = [cc.loop_seeds(cc.loop_scores_of_case(H, W, b), S, kw.get("roi_size"), kw.get("origin", (0, 0)),
                                  kw["margin"], kw["min_score"]) for b in range(B)]
            cc.same_pair(got, (torch.stack([w[0] for w in want]), torch.stack([w[1] for w in want])), f"{kw} B={B}")
        Gy, Gx = grid_shape((0, 0) + tuple(kw.get("roi_size") or (W, H)), S)
        empty = corner_seeds_ref(f[:0], S, **kw)
        assert empty[0].shape == (0, Gy * Gx, 2) and empty[1].shape == (0, Gy * Gx)
        assert empty[0].dtype == torch.float32 and empty[1].dtype == torch.int32


def test_the_median_min_score_sends_about_half_the_cells_back():
    """A condition on the cases: the second min_score of ``variants`` does what it is there for."""
    H, W, S = 64, 96, 8
    kw = cc.variants(H, W, S)[1]
    assert kw["margin"] == 0 and kw["min_score"] > 0
    _, _, fallback = cc.loop_seeds(cc.loop_scores_of_case(H, W, 0), S, None, (0, 0), 0, kw["min_score"])
    assert 0.3 <= fallback / (8 * 12) <= 0.7
    # and with min_score 0 the flat rectangle falls back, the noise does not
    seeds, score, fallback0 = cc.loop_seeds(cc.loop_scores_of_case(H, W, 0), S, None, (0, 0), 0, 0)
    assert 0 < fallback0 < 0.3 * 8 * 12 and int(score.min()) == 0


def test_score_map_is_the_loop_and_the_root_is_exact():
    f = cc.frames(37, 53)
    got = corner_score_ref(f)
    assert got.dtype == torch.int64
    for b in range(3):
        assert got[b].tolist() == cc.loop_scores_of_case(37, 53, b)
    assert int(got.min()) >= 0 and int(got.max()) <= cc.SCORE_MAX


# ---------------------------------------------------------------------------- extremes and ties
def test_stripes_and_constant_frames_score_zero_everywhere():
    """Straight edges are the aperture case: the smaller eigenvalue is 0, every seed a centre."""
    H, W, S = 24, 40, 8
    centre = _seed_xy((0, 0, W, H), S, None)
    for f in (cc.stripes(H, W, 1), cc.stripes(H, W, 2), cc.stripes(H, W, 1, False), cc.stripes(H, W, 2, False),
              cc.gray_frame(torch.full((H, W), 131)), cc.checkerboard(H, W, 1)):
        assert int(corner_score_ref(f).abs().max()) == 0
        seeds, score = corner_seeds_ref(f, S)
        assert tc.same(seeds[0], centre) and (score == 0).all()
        assert score.tolist() == [cc.loop_seeds(cc.loop_scores(f[0]), S)[1].tolist()]


def test_checkerboards_bounds_and_ties():
    H, W, S = 24, 40, 8
    f = cc.checkerboard(H, W, 2)
    smap = corner_score_ref(f)
    assert smap[0].tolist() == cc.loop_scores(f[0])
    assert int(smap.max()) == 6242400 and int(smap.min()) >= 0  # 6 * 1020^2, reached at the replicated border
    inner = smap[0, 2:-2, 2:-2]
    assert int(inner.min()) == int(inner.max()) > 0  # equal maxima away from the border
    # ... so that inside a cell away from the border the lowest index wins: the cell's first candidate
    for margin in (0, 2, 3):
        seeds, score = corner_seeds_ref(f, S, margin=margin)
        want = cc.loop_seeds(cc.loop_scores(f[0]), S, margin=margin)
        cc.same_pair((seeds, score), (want[0][None], want[1][None]))
        assert seeds[0].reshape(3, 5, 2)[1, 1].tolist() == [8 + margin, 8 + margin]
        assert int(score[0].reshape(3, 5)[1, 1]) == int(inner.max())
    # the largest possible contrast keeps every intermediate in range (loop_scores asserts the rest)
    g = torch.Generator().manual_seed(3)
    hard = cc.gray_frame(torch.randint(0, 2, (31, 33), generator=g) * 255)
    smap = corner_score_ref(hard)
    assert smap[0].tolist() == cc.loop_scores(hard[0]) and int(smap.max()) <= cc.SCORE_MAX and int(smap.min()) >= 0


def test_a_square_per_cell_is_found_at_one_of_its_corners():
    H, W, S = 48, 64, 16
    f = cc.squares(H, W, S, 4, 11)
    seeds, score = corner_seeds_ref(f, S)
    assert (score > 0).all()
    sx, sy = seeds[0, :, 0].long() % S, seeds[0, :, 1].long() % S
    near = lambda v: ((v - 4).abs() <= 1) | ((v - 10).abs() <= 1)  # noqa: E731
    assert (near(sx) & near(sy)).all()
    want = cc.loop_seeds(cc.loop_scores(f[0]), S)
    cc.same_pair((seeds, score), (want[0][None], want[1][None]))


def test_channel_order_does_not_matter():
    f = cc.frames(37, 53)
    assert not torch.equal(f, f.flip(-1))
    for S in (4, 8):
        cc.same_pair(corner_seeds_ref(f.flip(-1).contiguous(), S), corner_seeds_ref(f, S))


def test_corners_are_actually_used_on_real_and_noise_frames():
    """The reference alone must send fewer than 5 % of the cells to the centre on these inputs,
    else the tests that compare seeds would compare centres."""
    demo = cc.demo_frame()
    assert demo.shape == (1, 436, 1024, 3) and demo.dtype == torch.uint8
    for S, cells in ((8, 7040), (16, 1792), (32, 448)):
        score = corner_seeds_ref(demo, S, margin=0)[1]
        assert score.numel() == cells and cc.fallback_share(demo, S) < 0.05
    noise = cc.noise_frame()
    assert cc.fallback_share(noise, 8) < 0.05 and cc.fallback_share(noise, 8, None) < 0.05
    seeds, score = corner_seeds_ref(noise, 8)
    centre = _seed_xy((0, 0, 53, 37), 8, None)
    assert (seeds[0] != centre).any(dim=1).float().mean() > 0.5  # most seeds are off their centre


# ---------------------------------------------------------------------------- wrapper
def test_wrapper_cpu_path_and_errors():
    f = cc.frames(37, 53)
    cc.same_pair(corner_seeds(f, 8), corner_seeds_ref(f, 8))
    cc.same_pair(corner_seeds(f, 8, (50, 30), (2, 3), 1, 1000), corner_seeds_ref(f, 8, (50, 30), (2, 3), 1, 1000))
    e = corner_seeds(f[:0], 8)
    assert e[0].shape == (0, 35, 2) and e[1].shape == (0, 35)
    for bad in (dict(frames=f.float()), dict(frames=f[..., :2]), dict(frames=f[0]), dict(frames=f[:, :, ::2]),
                dict(frames=f.numpy()), dict(S=0), dict(S=-3), dict(S=2.5), dict(S=8, margin=4), dict(S=7, margin=4),
                dict(S=8, margin=-1), dict(S=1, margin=1), dict(roi_size=(54, 37)), dict(roi_size=(53, 0)),
                dict(min_score=0.5), dict(origin=(2 ** 24, 0))):
        kw = dict(dict(frames=f, S=8), **bad)
        with pytest.raises(ValueError):
            corner_seeds(**kw)
        with pytest.raises(ValueError):
            corner_seeds_ref(**kw)
    corner_seeds(f, 7, margin=3)  # the largest legal margin: one candidate per cell
    corner_seeds(f, 8, margin=3)


def test_fake_kernels_shapes_and_dtypes():
    from raft_ros_amd.ops import _ext

    if not _ext.is_loaded():
        pytest.skip("the native extension is not built")
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        f = torch.empty((2, 37, 53, 3), dtype=torch.uint8, device="cuda")
        seeds, score = torch.ops.raft_amd.corner_seeds(f, 8, 53, 37, 0, 0, 2, 0)
        assert seeds.shape == (2, 35, 2) and seeds.dtype == torch.float32 and score.shape == (2, 35)
        assert score.dtype == torch.int32
        pos = torch.empty((2, 35, 2), device="cuda")
        ids = torch.empty((2, 35), dtype=torch.int64, device="cuda")
        age = torch.empty((2, 35), dtype=torch.int32, device="cuda")
        epoch = torch.empty((1,), dtype=torch.int64, device="cuda")
        fw = torch.empty((2, 2, 37, 53), device="cuda")
        out = torch.ops.raft_amd.track_points_seeded(pos, ids, age, epoch, fw, None, seeds, 0, 0, 53, 37, 8, 0.01, 0.5)
        assert len(out) == 8 and out[0].shape == (2, 35, 2) and out[5].dtype == torch.uint8


# ---------------------------------------------------------------------------- the tracker with seeds
def _case_seeds(name, k):
    """Seeds of a chain case for step k: integer positions inside each cell, different per step."""
    B, H, W, roi, S = tc.CASES[name]
    left, top, w, h = roi
    Gy, Gx = grid_shape(roi, S)
    g = torch.Generator().manual_seed(31 * k + len(name))
    gy, gx = torch.meshgrid(torch.arange(Gy), torch.arange(Gx), indexing="ij")
    ox = torch.randint(0, S, (B, Gy, Gx), generator=g)
    oy = torch.randint(0, S, (B, Gy, Gx), generator=g)
    x = left + torch.minimum(gx[None] * S + ox, torch.tensor(w - 1))
    y = top + torch.minimum(gy[None] * S + oy, torch.tensor(h - 1))
    return torch.stack([x, y], dim=-1).reshape(B, Gy * Gx, 2).float().contiguous()


def _loop_with_seeds(inp, seeds):
    """``tc.loop_oracle`` decides every fate; the fresh slots (in slot order) then take the seeds of
    the unowned cells (in cell order), cell by cell in a Python loop."""
    out, claims = tc.loop_oracle(*inp)
    pos_out = out[0].clone()
    B, N = out[2].shape
    for b in range(B):
        fresh = [j for j in range(N) if int(out[3][b, j]) == 0]
        free = [c for c in range(N) if c not in claims[b]]
        assert len(fresh) == len(free)
        for j, c in zip(fresh, free):
            pos_out[b, j] = seeds[b, c]
    return (pos_out,) + tuple(out[1:])


@pytest.mark.parametrize("name", list(tc.CASES))
def test_seeded_reference_is_the_per_slot_loop(name):
    used = 0
    for k, (inp, old) in enumerate(tc.reference_chain(name)):
        seeds = _case_seeds(name, k)
        got = track_points_ref(*inp, seeds=seeds)
        tc.check(got, _loop_with_seeds(inp, seeds), f"{name} step {k}")
        tc.check(track_points(*inp, seeds=seeds), got, f"{name} step {k}: wrapper")
        # everything but the position of the fresh points is the old result
        for name_, g, o in zip(tc.NAMES[1:], got[1:], old[1:]):
            assert tc.same(g, o), name_
        used += int((got[0] != old[0]).any(dim=-1).sum())
        # no seeds, and the centres given as seeds, are bitwise the old result
        B, _, _, roi, S = tc.CASES[name]
        tc.check(track_points_ref(*inp, seeds=None), old, "seeds=None")
        centres = _seed_xy(roi, S, None)[None].expand(B, -1, 2).contiguous()
        tc.check(track_points_ref(*inp, seeds=centres), old, "seeds = centres")
    assert used > 0 or name in ("5x7_S1", "one_cell")  # S = 1: the one pixel of a cell is its centre


def test_seed_points_and_point_tracker_with_seeds():
    roi, S, B = (1, 2, 53, 37), 8, 2
    N = 35
    first = _case_seeds("roi_in_40x56", 0)
    later = _case_seeds("roi_in_40x56", 1)
    pos, ids, age, epoch = seed_points(B, roi, S, seeds=first)
    old = seed_points(B, roi, S)
    assert tc.same(pos, first) and pos.data_ptr() != first.data_ptr()
    assert all(tc.same(a, b) for a, b in zip((ids, age, epoch), old[1:]))
    for bad in (first[:, :34].contiguous(), first.double(), first[:1], first.transpose(0, 1)):
        with pytest.raises(ValueError):
            seed_points(B, roi, S, seeds=bad)
    fw, bw = tc.fields(B, 40, 56, roi, S, 0)
    for bad in (first[:, :34].contiguous(), first.double(), torch.zeros(B, N, 3)[..., :2]):
        with pytest.raises(ValueError):
            track_points(pos, ids, age, epoch, fw, bw, roi, S, seeds=bad)
    # a reseed starts at first_seeds and takes seeds for the points born in its step; a continued
    # pair does not read first_seeds
    tr = PointTracker(S=S, roi=roi)
    out1 = tr.update(fw, bw, seeds=later, first_seeds=first)
    tc.check(out1, track_points_ref(first, ids, age, epoch, fw, bw, roi, S, seeds=later), "first pair")
    kept = out1[5] == 0
    assert kept.any() and tc.same(out1[1][kept], first[kept])
    fresh = out1[3] == 0
    cells = later.reshape(B * N, 2).tolist()
    assert fresh.any() and all(p in cells for p in out1[0][fresh].tolist())
    fw2, bw2 = tc.fields(B, 40, 56, roi, S, 1)
    poison = torch.full_like(first, float("nan"))
    out2 = tr.update(fw2, bw2, seeds=first, first_seeds=poison)
    assert tr.resets == 1
    tc.check(out2, track_points_ref(out1[0], out1[2], out1[3], out1[4], fw2, bw2, roi, S, seeds=first), "second pair")
    out3 = tr.update(fw2, bw2, continuous=False, seeds=later, first_seeds=first)
    assert tr.resets == 2 and tc.same(out3[1][out3[5] == 0], first[out3[5] == 0])
    # without seeds the tracker is the old one
    a, b = PointTracker(S=S, roi=roi), PointTracker(S=S, roi=roi)
    tc.check(a.update(fw, bw), b.update(fw, bw, seeds=None, first_seeds=None), "no seeds")


def test_slot_scores():
    roi, S = (1, 2, 20, 12), 8  # 2 x 3 cells
    cell_score = torch.tensor([[10, 11, 12, 13, 14, -1]], dtype=torch.int32)
    pos = torch.tensor([[[1.0, 2.0], [9.5, 3.25], [20.0, 13.0], [17.0, 9.0], [2.0, 11.0], [12.0, 12.0]]])
    age = torch.tensor([[0, 3, 0, 0, 1, 0]], dtype=torch.int32)
    kept = torch.tensor([[1, 2, 3, 4, 5, 6]], dtype=torch.int32)
    assert slot_scores(pos, age, kept, cell_score, roi, S).tolist() == [[10, 2, -1, 12, 5, 14]]
    assert slot_scores(pos, age, None, cell_score, roi, S).tolist() == [[10, 11, -1, 12, 13, 14]]


# ---------------------------------------------------------------------------- FlowInference
@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(0)
    return [(rng.rand(124, 150, 3) * 255).astype(np.uint8) for _ in range(3)]


@pytest.mark.parametrize("median", [False, True], ids=["min_score_0", "min_score_median"])
def test_flow_inference_corner_seeds_on_the_cpu(frames, median):
    a, b, c = frames
    S, roi = 16, (1, 2, 150, 124)
    # the condition first: on these frames the reference alone uses corners
    pair = torch.stack([torch.from_numpy(a), torch.from_numpy(b)])
    min_score = int(corner_seeds_ref(pair, S)[1].median()) if median else 0
    ref_seeds, ref_score = corner_seeds_ref(pair, S, min_score=min_score)
    share = float((ref_score <= min_score).sum()) / ref_score.numel()
    assert 0.3 < share < 0.7 if median else share < 0.05
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, track=True, track_cell=S, track_seeds="corners",
                        track_min_score=min_score)
    flow, tr = inf.tracks(a, b, prev_stamp=1.0, curr_stamp=2.0)
    assert list(tr) == ["points", "prev", "ids", "age", "status", "score"]
    assert tr["score"].dtype == np.int32 and tr["score"].shape == (80,)
    # the step itself: the grid starts on the first frame's corners, fresh points on the second's
    shift = torch.tensor([1.0, 2.0])
    first, later = (ref_seeds + shift)[0:1].contiguous(), (ref_seeds + shift)[1:2].contiguous()
    pos0, ids0, age0, epoch0 = seed_points(1, roi, S, seeds=first)
    want = track_points_ref(pos0, ids0, age0, epoch0, flow.contiguous(), None, roi, S, seeds=later)
    assert tc.same(torch.from_numpy(tr["points"]), (want[0] - shift)[0])
    assert tc.same(torch.from_numpy(tr["prev"]), (want[1] - shift)[0])
    assert tr["ids"].tolist() == want[2][0].tolist() and tr["status"].tolist() == want[5][0].tolist()
    kept = tr["status"] == 0
    assert kept.any()
    assert np.array_equal(tr["score"][kept], ref_score[0].numpy()[kept])  # slot j was born in cell j of frame 1
    smap_a = corner_score_ref(torch.from_numpy(a)[None])[0]
    on_corner = kept & (tr["score"] > min_score)
    assert on_corner.any()
    for (x, y), sc in zip(tr["prev"][on_corner], tr["score"][on_corner]):
        assert x == int(x) and y == int(y) and int(smap_a[int(y), int(x)]) == sc

    def check_fresh(t, frame_scores):
        """Every slot of age 0 sits on an integer pixel with the reported score, or on the centre
        of its cell with a score <= min_score."""
        smap = corner_score_ref(torch.from_numpy(frame_scores)[None])[0]
        centre = _seed_xy((0, 0, 150, 124), S, None)
        n_corner = 0
        for j in np.flatnonzero(t["age"] == 0):
            x, y = t["points"][j]
            assert x == int(x) and y == int(y)
            cell = (int(y) // S) * 10 + int(x) // S
            if t["score"][j] > min_score:
                assert int(smap[int(y), int(x)]) == t["score"][j]
                n_corner += 1
            else:
                assert [x, y] == centre[cell].tolist()
        return n_corner

    check_fresh(tr, b)
    _, tr2 = inf.tracks(b, c, prev_stamp=2.0, curr_stamp=3.0)
    assert inf._tracker.resets == 1
    both = (tr2["status"] == 0) & kept
    assert both.any() and np.array_equal(tr2["score"][tr2["status"] == 0], tr["score"][tr2["status"] == 0])
    check_fresh(tr2, c)
    img, mask, tr3 = inf.visualize_tracks(a, b)
    assert mask is None and img.shape == (128, 152, 3) and list(tr3) == list(tr)
    # a pair without stamps seeds anew: everything but the ids is the first result
    assert all(np.array_equal(tr3[k], tr[k], equal_nan=True) for k in tr if k != "ids")


def test_flow_inference_grid_is_todays(frames):
    a, b, c = frames
    results = []
    for kw in (dict(), dict(track_seeds="grid", track_min_score=5)):
        torch.manual_seed(0)
        inf = FlowInference(None, small=True, device="cpu", iters=2, track=True, track_cell=16, **kw)
        results.append([inf.tracks(a, b, 1.0, 2.0), inf.tracks(b, c, 2.0, 3.0)])
    for (fa, ta), (fb, tb) in zip(*results):
        assert torch.equal(fa, fb) and list(ta) == list(tb) == ["points", "prev", "ids", "age", "status"]
        assert all(tc.same(torch.from_numpy(ta[k]), torch.from_numpy(tb[k])) for k in ta)
    roi = (1, 2, 150, 124)
    want = track_points_ref(*seed_points(1, roi, 16), results[1][0][0].contiguous(), None, roi, 16)
    assert tc.same(torch.from_numpy(results[1][0][1]["points"]), (want[0] - torch.tensor([1.0, 2.0]))[0])
    with pytest.raises(ValueError):
        FlowInference(None, small=True, device="cpu", iters=2, track=True, track_seeds="harris")


def test_flow_inference_corner_seeds_with_scale():
    """scale = 2: the corners come from the full-resolution frame and have no pad shift."""
    rng = np.random.RandomState(2)
    a, b = [(rng.rand(250, 300, 3) * 255).astype(np.uint8) for _ in range(2)]
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, track=True, track_cell=16, track_seeds="corners",
                        scale=2)
    flow, tr = inf.tracks(a, b, prev_stamp=1.0, curr_stamp=2.0)
    assert flow.shape == (1, 2, 250, 300)
    ref_seeds, ref_score = corner_seeds_ref(torch.stack([torch.from_numpy(a), torch.from_numpy(b)]), 16)
    roi = (0, 0, 300, 250)
    assert (ref_score > 0).float().mean() > 0.95
    pos0, ids0, age0, epoch0 = seed_points(1, roi, 16, seeds=ref_seeds[0:1].contiguous())
    want = track_points_ref(pos0, ids0, age0, epoch0, flow.contiguous(), None, roi, 16,
                            seeds=ref_seeds[1:2].contiguous())
    assert tc.same(torch.from_numpy(tr["points"]), want[0][0]) and tc.same(torch.from_numpy(tr["prev"]), want[1][0])


# ---------------------------------------------------------------------------- ROS node
class FakeRospy:
    def __init__(self, params):
        self.params = params
        self.pubs = []

    def init_node(self, *a, **k):
        pass

    def get_param(self, name, default=None):
        return self.params.get(name, default)

    def Subscriber(self, *a, **k):
        return None

    def Publisher(self, topic, cls, queue_size=None):
        pub = types.SimpleNamespace(topic=topic, queue_size=queue_size, sent=[])
        pub.publish = pub.sent.append
        self.pubs.append(pub)
        return pub

    def is_shutdown(self):
        return False


class FakeBridge:
    def imgmsg_to_cv2(self, msg, desired_encoding="passthrough"):
        return msg.data

    def cv2_to_imgmsg(self, img, encoding="passthrough", header=None):
        return types.SimpleNamespace(data=img, encoding=encoding, header=header)


def Msg(t, img):
    stamp = types.SimpleNamespace(to_sec=lambda: t, t=t)
    return types.SimpleNamespace(data=img, header=types.SimpleNamespace(stamp=stamp, frame_id=""))


class Cloud(types.SimpleNamespace):
    def __init__(self):
        super().__init__(header=None, points=[], channels=[])


MSGS = (Cloud, lambda x=0.0, y=0.0, z=0.0: types.SimpleNamespace(x=x, y=y, z=z),
        lambda name="", values=(): types.SimpleNamespace(name=name, values=list(values)))
BASE = {"/ROS/prev_img": "/p", "/ROS/curr_img": "/c"}


def test_node_parameter_and_score_channel(monkeypatch):
    import raft_ros_amd.ros.node as node_mod

    seen = {}

    def fake_inference(weight_path, small, device, **kw):
        seen.clear()
        seen.update(kw)
        return object()

    monkeypatch.setattr(node_mod, "FlowInference", fake_inference)
    base = dict(BASE, **{"/RAFT/weight_path": "", "/RAFT/is_small": True, "/RAFT/device": "cpu", "/RAFT/track": True})
    node = RaftRosNode(FakeRospy(dict(base)), image_msg=object, cv_bridge_cls=FakeBridge, track_msgs=MSGS)
    assert node.track_seeds == "grid" and "track_seeds" not in seen
    node = RaftRosNode(FakeRospy(dict(base, **{"/RAFT/track_seeds": "corners", "/RAFT/track_min_score": 7})),
                       image_msg=object, cv_bridge_cls=FakeBridge, track_msgs=MSGS)
    assert seen["track_seeds"] == "corners" and seen["track_min_score"] == 7 and seen["track"] is True
    monkeypatch.undo()
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, track=True, track_cell=32, track_seeds="corners")
    rospy = FakeRospy(dict(BASE, **{"/RAFT/track": True, "/RAFT/track_seeds": "corners"}))
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=inf, track_msgs=MSGS)
    rng = np.random.RandomState(1)
    a, b = [(rng.rand(130, 150, 3) * 255).astype(np.uint8) for _ in range(2)]
    node.process_pair(Msg(1.0, a), Msg(2.0, b))
    cloud = rospy.pubs[1].sent[0]
    assert [ch.name for ch in cloud.channels] == ["id", "prev_x", "prev_y", "age", "score"]
    assert len(cloud.channels[4].values) == len(cloud.points) > 0 and min(cloud.channels[4].values) >= -1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "ros", "config", "config.yaml")).read()
    assert "track_seeds: grid" in text and "track_min_score: 0" in text


# ---------------------------------------------------------------------------- demo.py
def test_demo_track_seeds_flag(tmp_path):
    import demo
    from raft_ros_amd.data.synthetic import demo_sequence

    frames_dir = str(tmp_path / "frames")
    os.makedirs(frames_dir)
    seq = [fr.permute(1, 2, 0).contiguous() for fr in demo_sequence(4, 128, 128)]
    for k, fr in enumerate(seq):
        Image.fromarray(fr.numpy()).save(os.path.join(frames_dir, "frame_%04d.png" % k))
    assert all(cc.fallback_share(fr[None], 16, None) < 0.05 for fr in seq)  # the condition: corners exist
    common = ["--path", frames_dir, "--device", "cpu", "--small", "--iters", "2", "--tracks", "--track_cell", "16"]
    torch.manual_seed(0)
    demo.main(common + ["--output", str(tmp_path / "grid")])
    torch.manual_seed(0)
    demo.main(common + ["--track_seeds", "corners", "--track_min_score", "0", "--output", str(tmp_path / "corners")])
    with open(tmp_path / "grid" / "tracks.csv") as f:
        assert next(csv.reader(f)) == ["frame", "id", "x", "y", "prev_x", "prev_y", "age"]
    with open(tmp_path / "corners" / "tracks.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "id", "x", "y", "prev_x", "prev_y", "age", "score"] and len(rows) > 1
    smaps = [corner_score_ref(fr[None])[0] for fr in seq]
    young = 0
    for r in rows[1:]:
        frame, age, score = int(r[0]), int(r[6]), int(r[7])
        px, py = float(r[4]), float(r[5])
        if age == 1:  # born one pair ago, on a corner of that pair's first frame (pair 0) or of the
            #           frame the previous pair ended in: both are frame ``frame``
            assert px == int(px) and py == int(py)
            if score > 0:  # else: the centre of a cell without a corner
                assert int(smaps[frame][int(py), int(px)]) == score
                young += 1
    assert young > 0
