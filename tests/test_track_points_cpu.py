"""Point tracks without a GPU: the torch reference against a per-slot loop, the conditions on the
cases, the invariants, the cross-check with the consistency op, the Python layer, the fake kernel
and the consumers (PointTracker, FlowInference.tracks, the ROS node with fakes, demo.py --tracks)."""
import csv
import os
import types

import numpy as np
import pytest
import torch
from PIL import Image

import consistency_cases as cc
import track_cases as tc
from raft_ros_amd import ops
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops.consistency import fb_consistency_ref
from raft_ros_amd.ops.track import PointTracker, grid_shape, seed_points, track_points, track_points_ref
from raft_ros_amd.ros.node import FlowInference, RaftRosNode
from test_ros_cpu import FakeBridge, FakeRospy, Msg


# ---------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("use_bw", [True, False], ids=["bw", "no_bw"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_reference_is_the_per_slot_loop(name, use_bw):
    """Every step of the reference's chain against the loop on numpy.float32 scalars: bitwise."""
    for k, (inp, out) in enumerate(tc.reference_chain(name, use_bw)):
        want, _ = tc.loop_oracle(*inp)
        assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int64, torch.int32, torch.int64,
                                          torch.uint8, torch.float32, torch.int32]
        tc.check(out, want, f"{name} step {k}")


@pytest.mark.parametrize("name", list(tc.CASES))
def test_invariants_after_every_step(name):
    B, H, W, roi, S = tc.CASES[name]
    left, top, w, h = roi
    Gy, Gx = grid_shape(roi, S)
    N = Gy * Gx
    seen = [set(range(N)) for _ in range(B)]  # every id an image has ever held
    for use_bw in (True, False):
        for k, (inp, out) in enumerate(tc.reference_chain(name, use_bw)):
            pos_out, prev, ids_out, age_out, epoch_out, status, err2, counts = out
            epoch, ids, age = inp[3], inp[1], inp[2]
            assert epoch_out.item() == epoch.item() + 1 == k + 2
            assert torch.equal(counts.sum(1), torch.full((B,), N, dtype=torch.int64)) and counts.dtype == torch.int32
            assert counts.tolist() == [[int((status[b] == s).sum()) for s in range(4)] for b in range(B)]
            # exactly one point per cell
            cell = ((pos_out[..., 1].floor().long() - top) // S) * Gx + (pos_out[..., 0].floor().long() - left) // S
            assert torch.equal(cell.sort(1).values, torch.arange(N)[None].expand(B, N))
            kept = status == 0
            slots = torch.arange(N)[None].expand(B, N)
            assert torch.equal(ids_out[kept], ids[kept]) and torch.equal(age_out[kept], age[kept] + 1)
            assert torch.equal(ids_out[~kept], (epoch.item() * N + slots)[~kept]) and (age_out[~kept] == 0).all()
            assert prev[~kept].isnan().all() and torch.equal(prev[kept], inp[0][kept])
            assert (err2[status == 2] == float("inf")).all() and not err2[status == 0].isnan().any()
            for b in range(B):
                assert len(set(ids_out[b].tolist())) == N
                if use_bw:  # ids are unique for the life of the state: a new id was never seen before
                    fresh = set(ids_out[b][~kept[b]].tolist())
                    assert not (fresh & seen[b])
                    seen[b] |= fresh


def test_conditions_on_the_cases():
    """The case set reaches every fate, the tie rule, re-seeding into another cell, the edges of the
    roi and the non-finite values.  Counted on the reference's chains; the claims of a cell (which
    the op does not return) are the loop oracle's, equal to the reference by the test above."""
    totals = torch.zeros(4, dtype=torch.int64)
    ties = moved = on_right = on_bottom = integer = 0
    nonfinite = {"fw": set(), "bw": set(), "pos": set()}
    for name, (B, H, W, roi, S) in tc.CASES.items():
        left, top, w, h = roi
        seeds = seed_points(B, roi, S)[0]
        for inp, out in tc.reference_chain(name):
            pos, ids, age, epoch, fw, bw = inp[:6]
            totals += out[7].sum(0)
            for key, t in (("fw", fw), ("bw", bw), ("pos", pos)):
                nonfinite[key] |= {s for s, m in (("nan", t.isnan()), ("+inf", t == float("inf")),
                                                   ("-inf", t == float("-inf"))) if m.any()}
            on_right += int((pos[..., 0] == left + w - 1).sum())
            on_bottom += int((pos[..., 1] == top + h - 1).sum())
            integer += int(((pos == pos.floor()).all(-1)).sum())
            lost = out[5] != 0
            moved += int((out[0][lost] != seeds[lost]).any(-1).sum())  # re-seeded into a cell that is not its index
            _, claims = tc.loop_oracle(*inp)
            for b, per_image in enumerate(claims):
                for cell, claimants in per_image.items():
                    best = sorted(claimants, key=lambda t: (-t[0], t[1]))
                    if len(best) > 1 and best[0][0] == best[1][0]:  # the two oldest are equally old: the slot decides
                        ties += 1
                        assert out[5][b, best[0][1]] == 0 and out[5][b, best[1][1]] == 3
                        assert best[0][1] < best[1][1]
    print("status totals", totals.tolist(), "ties", ties, "moved", moved, "edges", on_right, on_bottom, integer)
    assert (totals >= 5).all()
    assert ties >= 1 and moved >= 1
    assert on_right >= 1 and on_bottom >= 1 and integer >= 1
    assert all(v == {"nan", "+inf", "-inf"} for v in nonfinite.values()), nonfinite


def test_ages_differ_along_a_chain():
    _, out = tc.reference_chain("37x53_S8")[-1]
    assert len(set(out[3].flatten().tolist())) >= 3 and out[3].max() == tc.STEPS


# ---------------------------------------------------------------------------- against fb_consistency
@pytest.mark.parametrize("pair", ["parity", "random"])
def test_every_pixel_agrees_with_fb_consistency(pair):
    """A point on every pixel (S = 1, the state of seed_points): err2 bitwise the consistency op's,
    status 1 or 2 exactly where its class is 1 or 2."""
    fw, bw = cc.parity_pair() if pair == "parity" else cc.random_pair(12, 20, seed=4)
    H, W = fw.shape[1:]
    occ, err2, _ = fb_consistency_ref(fw[None], bw[None])
    out = track_points_ref(*seed_points(1, (0, 0, W, H), 1), fw[None].contiguous(), bw[None].contiguous(), None, 1)
    status, e = out[5].reshape(1, H, W), out[6].reshape(1, H, W)
    assert tc.same(e, err2)
    for k in (1, 2):
        assert torch.equal(status == k, occ == k)
    assert (occ == 1).any() and (occ == 2).any() and (status == 0).any()
    if pair == "parity":  # the smooth field also crowds pixels: class 0 splits into status 0 and 3
        assert (status == 3).any()


# ---------------------------------------------------------------------------- the Python layer
def test_seed_points_values():
    pos, ids, age, epoch = seed_points(2, (1, 2, 53, 37), 8)
    assert pos.shape == (2, 35, 2) and pos.dtype == torch.float32 and pos.is_contiguous()
    assert ids.dtype == torch.int64 and age.dtype == torch.int32 and epoch.dtype == torch.int64
    assert ids.tolist() == [list(range(35))] * 2 and (age == 0).all() and epoch.tolist() == [1]
    want = [(1 + min(gx * 8 + 4, 52), 2 + min(gy * 8 + 4, 36)) for gy in range(5) for gx in range(7)]
    assert pos[0].tolist() == [[float(x), float(y)] for x, y in want] and torch.equal(pos[0], pos[1])
    assert pos[0, 6].tolist() == [53.0, 6.0] and pos[0, 34].tolist() == [53.0, 38.0]  # partial cells: clamped
    assert seed_points(1, (0, 0, 7, 5), 1)[0][0, 8].tolist() == [1.0, 1.0]
    assert seed_points(1, (0, 0, 9, 6), 16)[0].tolist() == [[[8.0, 5.0]]]
    assert grid_shape((0, 0, 53, 37), 8) == (5, 7)
    assert seed_points(0, (0, 0, 9, 6), 4)[0].shape == (0, 6, 2)


def test_wrapper_cpu_path_defaults_and_absent_bw():
    inp, want = tc.reference_chain("37x53_S8")[1]
    pos, ids, age, epoch, fw, bw, roi, S = inp
    tc.check(track_points(pos, ids, age, epoch, fw, bw, roi, S), want, "wrapper")
    tc.check(track_points(pos, ids, age, epoch, fw, bw, None, S, 0.01, 0.5), want, "defaults")  # roi: the whole frame
    no_bw = track_points(pos, ids, age, epoch, fw, None, roi, S)
    tc.check(no_bw, tc.loop_oracle(pos, ids, age, epoch, fw, None, roi, S)[0], "no bw")
    assert (no_bw[5] != 1).all() and (no_bw[6][no_bw[5] != 2] == 0).all() and (no_bw[6][no_bw[5] == 2] == float("inf")).all()
    tight = track_points(pos, ids, age, epoch, fw, bw, roi, S, alpha1=0.0, alpha2=1e-4)
    assert tight[7][:, 1].sum() > want[7][:, 1].sum()  # a tighter criterion: more inconsistent points
    assert ops.track_points is track_points and ops.track_points_ref is track_points_ref
    assert ops.seed_points is seed_points and ops.PointTracker is PointTracker


def test_batch_zero():
    pos, ids, age, epoch = seed_points(0, (0, 0, 16, 8), 4)
    out = track_points(pos, ids, age, epoch + 4, torch.zeros(0, 2, 8, 16), torch.zeros(0, 2, 8, 16), None, 4)
    assert [tuple(o.shape) for o in out] == [(0, 8, 2), (0, 8, 2), (0, 8), (0, 8), (1,), (0, 8), (0, 8), (0, 4)]
    assert out[4].item() == 6 and out[5].dtype == torch.uint8 and out[7].dtype == torch.int32


def test_wrapper_errors():
    roi, S = (0, 0, 16, 8), 4
    pos, ids, age, epoch = seed_points(1, roi, S)
    f = torch.zeros(1, 2, 8, 16)
    track_points(pos, ids, age, epoch, f, f, roi, S)
    bads = [dict(pos=pos.double()), dict(pos=pos[:, :7]), dict(pos=torch.zeros(1, 8, 4)[..., ::2]),
            dict(ids=ids.int()), dict(ids=ids - 1), dict(age=age.long()), dict(epoch=epoch.int()),
            dict(epoch=torch.ones(2, dtype=torch.int64)), dict(fw=f.half()), dict(fw=f[0]), dict(fw=torch.zeros(1, 3, 8, 16)),
            dict(bw=f.half()), dict(bw=torch.zeros(1, 2, 16, 8)), dict(bw=torch.zeros(1, 2, 8, 32)[..., ::2]),
            dict(roi=(0, 0, 17, 8)), dict(roi=(1, 0, 16, 8)), dict(roi=(0, -1, 16, 8)), dict(roi=(0, 0, 16, 0)),
            dict(roi=(0, 0, 0, 8)), dict(roi=(0, 0, 16)), dict(S=0), dict(S=8), dict(fw=f.numpy())]
    for kw in bads:
        a = dict(pos=pos, ids=ids, age=age, epoch=epoch, fw=f, bw=f, roi=roi, S=S)
        a.update(kw)
        with pytest.raises(ValueError):
            track_points(a["pos"], a["ids"], a["age"], a["epoch"], a["fw"], a["bw"], a["roi"], a["S"])
    with pytest.raises(ValueError):
        seed_points(1, (0, 0, 4, 4), 0)


@pytest.mark.skipif(not _ext.is_loaded(), reason=f"native library not built: {_ext.load_error()}")
def test_fake_kernel_shapes_and_dtypes():
    m = dict(device="meta")
    out = _ext.ops().track_points(torch.empty(3, 6, 2, **m), torch.empty(3, 6, dtype=torch.int64, **m),
                                  torch.empty(3, 6, dtype=torch.int32, **m), torch.empty(1, dtype=torch.int64, **m),
                                  torch.empty(3, 2, 17, 23, **m), None, 0, 0, 23, 17, 8, 0.01, 0.5)
    assert [tuple(o.shape) for o in out] == [(3, 6, 2), (3, 6, 2), (3, 6), (3, 6), (1,), (3, 6), (3, 6), (3, 4)]
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int64, torch.int32, torch.int64, torch.uint8,
                                      torch.float32, torch.int32]
    assert all(o.device.type == "meta" for o in out)


# ---------------------------------------------------------------------------- PointTracker
def test_point_tracker_reset_rules():
    fw = torch.zeros(1, 2, 16, 24)
    fw[:, 0] = 1.0
    tr = PointTracker(S=8)
    out = tr.update(fw, -fw)
    N = 6
    assert tr.resets == 1 and out[2].tolist() == [list(range(N))] and (out[3] == 1).all()
    assert torch.equal(out[1], seed_points(1, (0, 0, 24, 16), 8)[0])  # seeded in the first frame, then moved
    assert torch.equal(out[0], out[1] + torch.tensor([1.0, 0.0]))
    out = tr.update(fw, -fw)
    assert tr.resets == 1 and (out[3] == 2).all() and out[2].tolist() == [list(range(N))]
    ids_seen = set(range(N))
    out = tr.update(fw, -fw, continuous=False)  # a gap: fresh points, fresh ids
    assert tr.resets == 2 and (out[3] == 1).all() and not (set(out[2].flatten().tolist()) & ids_seen)
    ids_seen |= set(out[2].flatten().tolist())
    out = tr.update(fw)  # bw absent: no reset
    assert tr.resets == 2 and (out[3] == 2).all()
    for change in (dict(flow=torch.zeros(1, 2, 16, 32)), dict(flow=torch.zeros(2, 2, 16, 24)), dict(roi=(0, 0, 20, 16)),
                   dict(S=4)):
        if "S" in change:
            tr.S = change["S"]
        flow = change.get("flow", torch.zeros(1, 2, 16, 24))
        n_before = tr.resets
        out = tr.update(flow, roi=change.get("roi"))
        assert tr.resets == n_before + 1 and (out[3] == 1).all(), change
        new = set(out[2].flatten().tolist())
        assert not (new & ids_seen), change  # ids are never reused, whatever the grid
        ids_seen |= new
        out = tr.update(flow)
        assert tr.resets == n_before + 1
        ids_seen |= set(out[2].flatten().tolist())
    tr.reset()
    tr.update(flow)
    assert tr.resets == n_before + 2
    # a point that leaves gets a new id in the same slot; the epoch counts on across resets
    far = torch.zeros(1, 2, 16, 24)
    far[:, 0, :, 16:] = 100.0
    t2 = PointTracker(S=8)
    t2.update(torch.zeros(1, 2, 16, 24))
    out = t2.update(far)
    assert out[5].tolist() == [[0, 0, 2, 0, 0, 2]] and out[2].tolist() == [[0, 1, 2 * 6 + 2, 3, 4, 2 * 6 + 5]]
    assert out[4].item() == 3


# ---------------------------------------------------------------------------- FlowInference
@pytest.fixture(scope="module")
def frames():
    rng = np.random.RandomState(0)
    return [(rng.rand(124, 150, 3) * 255).astype(np.uint8) for _ in range(3)]


def test_flow_inference_tracks_on_the_cpu(frames):
    a, b, c = frames
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, track=True, track_cell=16)
    assert inf.track is True and inf.track_cell == 16
    flow, tr = inf.tracks(a, b, prev_stamp=1.0, curr_stamp=2.0)
    assert flow.shape == (1, 2, 128, 152) and torch.equal(flow, inf.flow(a, b))
    N = 8 * 10  # the grid tiles the unpadded 124 x 150 image
    assert set(tr) == {"points", "prev", "ids", "age", "status"}
    assert tr["points"].shape == (N, 2) and tr["points"].dtype == np.float32 and tr["prev"].shape == (N, 2)
    assert tr["ids"].dtype == np.int64 and tr["age"].dtype == np.int32 and tr["status"].dtype == np.uint8
    # the step itself, in frame coordinates: roi = the image inside the padded frame (left 1, top 2)
    roi = (1, 2, 150, 124)
    want = track_points_ref(*seed_points(1, roi, 16), flow.contiguous(), None, roi, 16)
    shift = torch.tensor([1.0, 2.0])
    assert tc.same(torch.from_numpy(tr["points"]), (want[0] - shift)[0])
    assert tc.same(torch.from_numpy(tr["prev"]), (want[1] - shift)[0])
    assert tr["ids"].tolist() == want[2][0].tolist() and tr["status"].tolist() == want[5][0].tolist()
    assert (tr["status"] != 1).all()  # without consistency only the frame test applies
    kept = tr["status"] == 0
    assert kept.any() and np.array_equal(tr["prev"][kept], seed_points(1, (0, 0, 150, 124), 16)[0][0].numpy()[kept])
    # continuity: the next pair starts where this one ended ...
    _, tr2 = inf.tracks(b, c, prev_stamp=2.0, curr_stamp=3.0)
    assert inf._tracker.resets == 1
    both = (tr2["status"] == 0) & kept
    assert both.any() and np.array_equal(tr2["prev"][both], tr["points"][both]) and (tr2["age"][both] == 2).all()
    assert np.array_equal(tr2["ids"][both], tr["ids"][both])
    # ... a stamp gap, a missing stamp or another frame size seeds anew, with new ids
    seen = set(tr["ids"].tolist()) | set(tr2["ids"].tolist())
    for kw in (dict(prev_stamp=3.5, curr_stamp=4.0), dict(), dict(prev_stamp=None, curr_stamp=5.0)):
        n = inf._tracker.resets
        _, t3 = inf.tracks(a, b, **kw)
        assert inf._tracker.resets == n + 1 and t3["age"].max() == 1 and not (set(t3["ids"].tolist()) & seen)
        seen |= set(t3["ids"].tolist())
    _, t4 = inf.tracks(b[:, :140], c[:, :140], prev_stamp=5.0, curr_stamp=6.0)
    assert inf._tracker.resets == n + 2 and t4["points"].shape == (8 * 9, 2) and t4["age"].max() == 1
    off = FlowInference(None, small=True, device="cpu", iters=2)
    assert off.track is False
    with pytest.raises(RuntimeError):
        off.tracks(a, b)


def test_flow_inference_tracks_with_consistency(frames):
    a, b, _ = frames
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, consistency=True, track=True, track_cell=16)
    flow, tr = inf.tracks(a, b)
    with torch.no_grad():
        t = [torch.from_numpy(x).permute(2, 0, 1).float()[None] for x in (a, b)]
        i1, i2 = inf._padded_pair(a, b)
        _, up = inf.model(torch.cat([i1, i2]), torch.cat([i2, i1]), iters=2, test_mode=True)
    assert t[0].shape[-2:] == (124, 150) and torch.equal(flow, up[0:1])
    roi = (1, 2, 150, 124)
    want = track_points_ref(*seed_points(1, roi, 16), up[0:1].contiguous(), up[1:2].contiguous(), roi, 16)
    assert tr["status"].tolist() == want[5][0].tolist() and tr["ids"].tolist() == want[2][0].tolist()
    img, mask, tr_v = inf.visualize_tracks(a, b)
    assert img.shape == (128, 152, 3) and img.dtype == np.uint8 and mask.shape == (128, 152)
    assert set(np.unique(mask).tolist()) <= {0, 128, 255} and tr_v["status"].tolist() == tr["status"].tolist()


# ---------------------------------------------------------------------------- ROS node
class TrackRecorder:
    def __init__(self):
        self.calls = []

    def visualize(self, prev, curr, prev_stamp=None, curr_stamp=None):
        self.calls.append(("visualize", prev_stamp, curr_stamp))
        return np.zeros(prev.shape, np.uint8)

    def visualize_tracks(self, prev, curr, prev_stamp=None, curr_stamp=None):
        self.calls.append(("visualize_tracks", prev_stamp, curr_stamp))
        tracks = dict(points=np.array([[1.5, 2.0], [3.0, 4.0], [5.25, 6.0], [7.0, 8.0]], np.float32),
                      prev=np.array([[1.0, 2.5], [np.nan, np.nan], [5.0, 6.5], [np.nan, np.nan]], np.float32),
                      ids=np.array([7, 8, (1 << 24) + 5, 10], np.int64), age=np.array([3, 0, 12, 0], np.int32),
                      status=np.array([0, 2, 0, 3], np.uint8))
        return np.zeros(prev.shape, np.uint8), np.zeros(prev.shape[:2], np.uint8), tracks


class Cloud(types.SimpleNamespace):
    def __init__(self):
        super().__init__(header=None, points=[], channels=[])


def Point32(x=0.0, y=0.0, z=0.0):
    return types.SimpleNamespace(x=x, y=y, z=z)


def Channel(name="", values=()):
    return types.SimpleNamespace(name=name, values=list(values))


BASE = {"/ROS/prev_img": "/p", "/ROS/curr_img": "/c"}
MSGS = (Cloud, Point32, Channel)


def test_node_without_the_parameter_has_no_third_publisher():
    for extra in ({}, {"/RAFT/occlusion": True}):
        rospy = FakeRospy(dict(BASE, **extra))
        node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=TrackRecorder(), track_msgs=MSGS)
        assert node.track is False and "/raft_tracks" not in [p.topic for p in rospy.pubs]
    rospy = FakeRospy(dict(BASE))
    rec = TrackRecorder()
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=rec)  # the old call still works
    img = np.zeros((16, 24, 3), np.uint8)
    node.process_pair(Msg(1.0, img), Msg(2.0, img))
    assert rec.calls == [("visualize", None, None)] and [p.topic for p in rospy.pubs] == ["/raft_result"]


@pytest.mark.parametrize("occlusion", [False, True])
def test_node_publishes_the_tracks(occlusion):
    rospy = FakeRospy(dict(BASE, **{"/RAFT/track": True, "/RAFT/track_cell": 16, "/RAFT/occlusion": occlusion}))
    rec = TrackRecorder()
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=rec, track_msgs=MSGS)
    assert node.track is True and node.track_cell == 16
    topics = [(p.topic, p.queue_size) for p in rospy.pubs]
    assert topics == [("/raft_result", 100)] + ([("/raft_occlusion", 100)] if occlusion else []) + [("/raft_tracks", 100)]
    img = np.zeros((16, 24, 3), np.uint8)
    out = node.process_pair(Msg(1.0, img), Msg(2.0, img))
    assert rec.calls == [("visualize_tracks", 1.0, 2.0)]  # the stamps decide continuity
    cloud = rospy.pubs[-1].sent
    assert len(cloud) == 1 and len(rospy.pubs[0].sent) == 1 and rospy.pubs[0].sent[0] is out
    cloud = cloud[0]
    assert cloud.header is out.header and cloud.header.frame_id == "raft_image" and cloud.header.stamp.t == 2.0
    assert [(p.x, p.y, p.z) for p in cloud.points] == [(1.5, 2.0, 0.0), (5.25, 6.0, 0.0)]  # status 0 only
    assert [c.name for c in cloud.channels] == ["id", "prev_x", "prev_y", "age"]
    assert [c.values for c in cloud.channels] == [[7.0, 5.0], [1.0, 5.0], [2.5, 6.5], [3.0, 12.0]]
    if occlusion:
        assert len(rospy.pubs[1].sent) == 1 and rospy.pubs[1].sent[0].encoding == "mono8"


def test_node_builds_inference_with_track(monkeypatch):
    import raft_ros_amd.ros.node as node_mod

    seen = {}

    def fake_inference(weight_path, small, device, **kw):
        seen.clear()
        seen.update(kw)
        return TrackRecorder()

    monkeypatch.setattr(node_mod, "FlowInference", fake_inference)
    base = dict(BASE, **{"/RAFT/weight_path": "", "/RAFT/is_small": True, "/RAFT/device": "cpu"})
    RaftRosNode(FakeRospy(dict(base)), image_msg=object, cv_bridge_cls=FakeBridge)
    assert not seen.get("track", False)
    RaftRosNode(FakeRospy(dict(base, **{"/RAFT/track": True, "/RAFT/track_cell": 24})), image_msg=object,
                cv_bridge_cls=FakeBridge, track_msgs=MSGS)
    assert seen["track"] is True and seen["track_cell"] == 24 and seen["consistency"] is False


def test_node_end_to_end_tracks():
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cpu", iters=2, track=True, track_cell=32)
    rospy = FakeRospy(dict(BASE, **{"/RAFT/track": True}))
    node = RaftRosNode(rospy, image_msg=object, cv_bridge_cls=FakeBridge, inference=inf, track_msgs=MSGS)
    rng = np.random.RandomState(1)
    a, b, c = [(rng.rand(130, 150, 3) * 255).astype(np.uint8) for _ in range(3)]
    node.process_pair(Msg(1.0, a), Msg(2.0, b))
    node.process_pair(Msg(2.0, b), Msg(3.0, c))
    first, second = rospy.pubs[1].sent
    assert rospy.pubs[1].topic == "/raft_tracks" and 0 < len(second.points) <= 5 * 5
    ages = second.channels[3].values
    assert max(ages) == 2.0 and inf._tracker.resets == 1
    for p, px, py in zip(second.points, second.channels[1].values, second.channels[2].values):
        assert 0 <= p.x <= 149 and 0 <= p.y <= 129 and p.z == 0.0 and 0 <= px <= 149 and 0 <= py <= 129


def test_config_yaml_has_the_parameters():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "ros", "config", "config.yaml")).read()
    assert "track: false" in text and "track_cell: 32" in text


# ---------------------------------------------------------------------------- demo.py
def test_demo_tracks_flag(tmp_path):
    import demo
    from raft_ros_amd.data.synthetic import demo_sequence

    frames_dir = str(tmp_path / "frames")
    os.makedirs(frames_dir)
    for k, fr in enumerate(demo_sequence(4, 128, 128)):
        Image.fromarray(fr.permute(1, 2, 0).numpy()).save(os.path.join(frames_dir, "frame_%04d.png" % k))
    common = ["--path", frames_dir, "--device", "cpu", "--small", "--iters", "2"]
    torch.manual_seed(0)
    plain = demo.main(common + ["--output", str(tmp_path / "plain")])
    assert "tracks.csv" not in os.listdir(tmp_path / "plain")
    for extra in ([], ["--occlusion"]):
        out_dir = tmp_path / ("tracks" + "".join(extra))
        torch.manual_seed(0)
        outs = demo.main(common + ["--tracks", "--track_cell", "16", "--output", str(out_dir)] + extra)
        assert [os.path.basename(f) for f in outs] == [os.path.basename(f) for f in plain]
        with open(out_dir / "tracks.csv") as f:
            rows = list(csv.reader(f))
        assert rows[0] == ["frame", "id", "x", "y", "prev_x", "prev_y", "age"] and len(rows) > 1
        per_frame = {}
        for r in rows[1:]:
            assert len(r) == 7
            frame, pid, age = int(r[0]), int(r[1]), int(r[6])
            x, y, px, py = map(float, r[2:6])
            assert 0 <= frame < 3 and 1 <= age <= frame + 1 and pid >= 0
            assert 0 <= x <= 127 and 0 <= y <= 127 and 0 <= px <= 127 and 0 <= py <= 127
            per_frame.setdefault(frame, []).append(pid)
        assert all(len(v) == len(set(v)) <= 64 for v in per_frame.values())  # unique ids, at most one per cell
