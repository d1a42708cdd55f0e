#!/usr/bin/env python3
"""RAFT demo -- same command line as the reference demo.py (:66-75).

    python demo.py --model=models/raft-things.pth --path=demo-frames

Without ``--path`` the frames are read from ``demo-frames/``; when that directory holds no
frames a synthetic sequence (textured background drift + a moving disc,
``data/synthetic.demo_sequence``) is written there first.

Runs every consecutive pair of *.png / *.jpg frames in ``--path`` (sorted) with
20 refinement iterations.  The reference shows [image; flow] in a cv2 window;
here the visualisation is shown with cv2 when it is importable and a display is
available, and is always written to ``--output`` (default ``demo-output/``) as
PNG.  With ``--occlusion`` every pair also runs backwards (one batch of two) and the
forward-backward consistency mask is written beside the flow as ``occ_%04d.png``
(0 consistent, 128 inconsistent, 255 the flow leaves the frame).  With ``--tracks`` a
grid of points (one per ``--track_cell`` cell of the image) is followed through the
flows on the device and the tracked points of every pair are written to
``tracks.csv`` (``frame,id,x,y,prev_x,prev_y,age``, image coordinates); ``--track_seeds corners``
starts every new point on the Shi-Tomasi corner of its cell and adds the column ``score``.  With ``--scale D``
(an integer in 2..8) the model runs on the frames reduced by ``D`` and its flow is brought
back to the frames' resolution and pixel units on the device (``ops/frame_scale.py``); the
picture, the mask and the tracks are those of the unpadded frame.  ``--model`` is
optional (random weights) so the pipeline can be smoke-tested without the
pretrained files.
"""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from raft_ros_amd.models import RAFT  # noqa: E402
from raft_ros_amd.ops.consistency import OCC_LEVELS, fb_consistency  # noqa: E402
from raft_ros_amd.ops.frame_io import flow_to_image, ingest_frames  # noqa: E402
from raft_ros_amd.ops.frame_scale import ingest_frames_scaled, upscale_flow  # noqa: E402
from raft_ros_amd.ops.corners import corner_seeds, slot_scores  # noqa: E402
from raft_ros_amd.ops.track import PointTracker  # noqa: E402
from raft_ros_amd.ops.warm_start import forward_splat_nearest  # noqa: E402
from raft_ros_amd.utils import checkpoint, flow_viz  # noqa: E402
from raft_ros_amd.utils.utils import InputPadder  # noqa: E402

DEVICE = "cuda" if torch.cuda.is_available() else "cpu"


def load_image(imfile, device=DEVICE, raw=False):
    """(1, 3, H, W) fp32 on ``device``; ``raw``: the (H, W, 3) uint8 frame itself, uploaded as it is."""
    img = np.array(Image.open(imfile).convert("RGB")).astype(np.uint8)
    if raw:
        return torch.from_numpy(img).to(device)
    img = torch.from_numpy(img).permute(2, 0, 1).float()
    return img[None].to(device)


def viz(img, flo, out_path=None, show=False, device_viz=False):
    if device_viz:  # colour-code where the flow lives: only the uint8 [image; flow] comes back
        img = img[0].permute(1, 2, 0).to(torch.uint8)
        img_flo = torch.cat([img, flow_to_image(flo[0])], dim=0).cpu().numpy()
    else:
        img = img[0].permute(1, 2, 0).cpu().numpy()
        flo = flo[0].permute(1, 2, 0).cpu().numpy()
        flo = flow_viz.flow_to_image(flo)
        img_flo = np.concatenate([img, flo], axis=0).astype(np.uint8)
    if out_path:
        Image.fromarray(img_flo).save(out_path)
    if show:
        try:
            import cv2

            cv2.imshow("image", img_flo[:, :, [2, 1, 0]] / 255.0)
            cv2.waitKey()
        except Exception:
            pass
    return img_flo


def write_demo_frames(path, n_frames: int = 6):
    """No frames at ``path``: write a synthetic sequence there (the reference's Sintel demo
    frames are not redistributed with this repository)."""
    from raft_ros_amd.data.synthetic import demo_sequence

    os.makedirs(path, exist_ok=True)
    out = []
    for k, fr in enumerate(demo_sequence(n_frames)):
        f = os.path.join(path, "frame_%04d.png" % (16 + k))
        Image.fromarray(fr.permute(1, 2, 0).numpy()).save(f)
        out.append(f)
    print(f"demo: no frames in {path}; wrote {len(out)} synthetic frames there")
    return out


def demo(args):
    rank = 0
    if getattr(args, "query_shard", False):
        # torchrun --nproc-per-node N demo.py --query_shard: every rank runs the same frames,
        # each holding the correlation-volume rows of 1/N of the query pixels; rank 0 writes
        from raft_ros_amd.parallel import ddp

        info = ddp.init_distributed()
        rank = info.rank
        if info.device.type == "cuda":
            args.device = str(info.device)
    model = RAFT(args)
    if args.model:
        checkpoint.load_weights(model, args.model)
    model.to(args.device).eval()
    os.makedirs(args.output, exist_ok=True)
    images = sorted(glob.glob(os.path.join(args.path, "*.png")) + glob.glob(os.path.join(args.path, "*.jpg")))
    if not images:
        images = write_demo_frames(args.path)
    outs = []
    warm = getattr(args, "warm_start", False)
    flow_prev = None  # --warm_start: the last pair's low-resolution flow, projected onto its second frame
    device_viz = getattr(args, "device_viz", False)
    occlusion = getattr(args, "occlusion", False)
    scale = getattr(args, "scale", 1)
    # --tracks: consecutive pairs of the sorted directory are continuous; the tracker itself
    # starts over when the frame size changes
    tracker = PointTracker(S=getattr(args, "track_cell", 32)) if getattr(args, "tracks", False) else None
    # --track_seeds corners: a new point starts on the Shi-Tomasi corner of its cell, found in the
    # uint8 frames (ops/corners.py); tracks.csv gains the score each point was born with
    corners = tracker is not None and getattr(args, "track_seeds", "grid") == "corners"
    min_score = getattr(args, "track_min_score", 0)
    born = None
    rows = ["frame,id,x,y,prev_x,prev_y,age" + (",score" if corners else "")]
    with torch.inference_mode():
        for k, (imfile1, imfile2) in enumerate(zip(images[:-1], images[1:])):
            raw1 = None
            if scale > 1:
                # working resolution: the uint8 frames are reduced and padded by one launch; the
                # model sees the low-resolution pair, everything after it the upscaled flow
                raw1 = load_image(imfile1, args.device, raw=True)
                pair, padder = ingest_frames_scaled([raw1, load_image(imfile2, args.device, raw=True)], scale)
                image1, image2 = pair[0:1], pair[1:2]
            elif device_viz:
                pair, padder = ingest_frames([load_image(imfile1, args.device, raw=True),
                                              load_image(imfile2, args.device, raw=True)])
                image1, image2 = pair[0:1], pair[1:2]
            else:
                image1 = load_image(imfile1, args.device)
                image2 = load_image(imfile2, args.device)
                padder = InputPadder(image1.shape)
                image1, image2 = padder.pad(image1, image2)
            if flow_prev is not None and flow_prev.shape[-2:] != (image1.shape[-2] // 8, image1.shape[-1] // 8):
                flow_prev = None  # the frame size changed: cold start
            flow_bw = None
            if occlusion:
                # both directions as one batch of the pair and the swapped pair; the backward
                # direction has no previous flow and always starts cold
                init = None if flow_prev is None else torch.cat([flow_prev, torch.zeros_like(flow_prev)])
                flow_low, flow_up = model(torch.cat([image1, image2]), torch.cat([image2, image1]), iters=args.iters,
                                          flow_init=init, test_mode=True)
                if scale > 1:  # both directions in one call, onto the unpadded frame
                    flow_up = upscale_flow(flow_up, padder, scale, raw1.shape[:2])
                occ = fb_consistency(flow_up[0:1], flow_up[1:2])[0]
                flow_bw = flow_up[1:2].float().contiguous()
                flow_low, flow_up = flow_low[0:1], flow_up[0:1]
                if rank == 0:  # mono mask: 0 consistent, 128 inconsistent, 255 the flow leaves the frame
                    mask = OCC_LEVELS[occ[0].cpu().numpy()]
                    Image.fromarray(mask, mode="L").save(os.path.join(args.output, "occ_%04d.png" % k))
            else:
                flow_low, flow_up = model(image1, image2, iters=args.iters, flow_init=flow_prev, test_mode=True)
                if scale > 1:
                    flow_up = upscale_flow(flow_up, padder, scale, raw1.shape[:2])
            if warm:
                flow_prev = forward_splat_nearest(flow_low)
            if tracker is not None:
                # the points live in the unpadded image inside the padded frame; with --occlusion
                # the forward-backward check drops inconsistent points
                if scale > 1:  # the upscaled flow is the unpadded frame's: no pad shift
                    left, top = 0, 0
                    roi = (0, 0, raw1.shape[1], raw1.shape[0])
                else:
                    left, top = padder._pad[0], padder._pad[2]
                    roi = (left, top, padder.wd, padder.ht)
                seeds = {}
                if corners:
                    # the first frame's corners serve a fresh grid, the second frame's the points born
                    # in this step
                    pair8 = torch.stack([load_image(imfile1, args.device, raw=True),
                                         load_image(imfile2, args.device, raw=True)])
                    found, cell_score = corner_seeds(pair8, tracker.S, roi[2:], (left, top), min_score=min_score)
                    seeds = dict(first_seeds=found[0:1], seeds=found[1:2])
                    resets = tracker.resets
                pos, prv, ids, age, _, status, _, _ = tracker.update(flow_up.float().contiguous(), flow_bw, roi=roi,
                                                                    **seeds)
                if corners:
                    born = slot_scores(pos, age, born if tracker.resets == resets else cell_score[0:1],
                                       cell_score[1:2], roi, tracker.S)
                    score = born[0].cpu().numpy()
                pos, prv, ids, age, status = [t[0].cpu().numpy() for t in (pos, prv, ids, age, status)]
                for j in np.flatnonzero(status == 0):
                    rows.append("%d,%d,%.3f,%.3f,%.3f,%.3f,%d" % (k, ids[j], pos[j, 0] - left, pos[j, 1] - top,
                                                                 prv[j, 0] - left, prv[j, 1] - top, age[j])
                                + (",%d" % score[j] if corners else ""))
            out = os.path.join(args.output, "flow_%04d.png" % k)
            if rank == 0:
                # --scale: the picture shows the raw frame above the upscaled flow
                shown = image1 if raw1 is None else raw1.permute(2, 0, 1)[None].float()
                viz(shown, flow_up, out, show=args.show, device_viz=device_viz)
            outs.append(out)
    if tracker is not None and rank == 0:
        with open(os.path.join(args.output, "tracks.csv"), "w") as f:
            f.write("\n".join(rows) + "\n")
    return outs


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model", help="restore checkpoint")
    p.add_argument("--path", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "demo-frames"),
                   help="directory of frames (default: demo-frames/, synthesised on first use)")
    p.add_argument("--small", action="store_true", help="use small model")
    p.add_argument("--mixed_precision", action="store_true", help="use mixed precision")
    p.add_argument("--alternate_corr", action="store_true", help="use efficent correlation implementation")
    p.add_argument("--amp_dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--corr_fp32", action="store_true",
                   help="with --mixed_precision bf16: fp32-faithful correlation volume (the reference's precision)")
    p.add_argument("--device", default=DEVICE)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--output", default="demo-output")
    p.add_argument("--show", action="store_true", help="also display with cv2 (if available)")
    p.add_argument("--warm_start", action="store_true",
                   help="start every pair from the previous pair's flow, forward-projected on the device "
                        "(consecutive pairs of the sorted directory are continuous)")
    p.add_argument("--device_viz", action="store_true",
                   help="frames are uploaded as uint8 and converted and padded on the device, the flow is "
                        "colour-coded on the device: only the uint8 image comes back (ops/frame_io.py)")
    p.add_argument("--occlusion", action="store_true",
                   help="run every pair in both directions (one batch of two) and write the forward-backward "
                        "consistency mask as occ_%%04d.png beside the flow: 0 consistent, 128 inconsistent, "
                        "255 the flow leaves the frame (ops/consistency.py)")
    p.add_argument("--tracks", action="store_true",
                   help="follow a grid of points through the flows on the device and write the tracked points of "
                        "every pair to tracks.csv (frame,id,x,y,prev_x,prev_y,age; ops/track.py)")
    p.add_argument("--track_cell", type=int, default=32, help="with --tracks: the cell size, one point per cell")
    p.add_argument("--track_seeds", default="grid", choices=["grid", "corners"],
                   help="with --tracks: where a new point starts: the centre of its cell (grid) or the cell's "
                        "Shi-Tomasi corner, found on the device (ops/corners.py); with corners tracks.csv gains "
                        "the column score, the corner score the point was born with")
    p.add_argument("--track_min_score", type=int, default=0,
                   help="with --track_seeds corners: a cell whose best score is not above this keeps its centre")
    p.add_argument("--scale", type=int, default=1, choices=range(1, 9), metavar="D",
                   help="working resolution: run the model on the frames reduced by the integer factor D (1..8) and "
                        "bring the flow back to the frames' resolution and pixel units (ops/frame_scale.py)")
    p.add_argument("--query_shard", action="store_true",
                   help="under torchrun: shard the correlation volume over the ranks' query pixels "
                        "(high-resolution inference; raft_ros_amd/parallel/query_shard.py)")
    args = p.parse_args(argv)
    return demo(args)


if __name__ == "__main__":
    main()
