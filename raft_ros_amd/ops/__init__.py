"""Native (HIP/CDNA4) ops of raft_ros_amd with their autograd wiring.

``torch.ops.raft_amd.*`` are registered by the in-tree extension
``raft_ros_amd/_C.so`` (built from ``raft_ros_amd/csrc``); the
``reference`` module holds the pure-PyTorch equivalents used on CPU and as the
numerical oracle in tests.
"""
from ._ext import is_loaded, library_path, load_error, use_native  # noqa: F401
from .consistency import fb_consistency, fb_consistency_ref  # noqa: F401
from .corners import corner_seeds, corner_seeds_ref  # noqa: F401
from .corr import CorrPyramid, LocalCorrPyramid  # noqa: F401
from .frame_io import flow_to_image, ingest_frames  # noqa: F401
from .frame_scale import ingest_frames_scaled, ingest_frames_scaled_ref, scaled_shape, upscale_flow, upscale_flow_ref  # noqa: F401
from .metrics import flow_metrics, flow_metrics_ref  # noqa: F401
from .track import PointTracker, seed_points, track_points, track_points_ref  # noqa: F401
from .upsample import convex_upsample, upflow8  # noqa: F401
from .warm_start import forward_splat_nearest  # noqa: F401
from . import reference  # noqa: F401
