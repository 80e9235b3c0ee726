"""Visual localization on the engine: mirrors of the reference's `dust3r_visloc.localization` (run_pnp) and
`dust3r_visloc.evaluation`, plus `localize`, the batched form of visloc.py's per-query loop."""
from .evaluation import aggregate_stats, export_results, get_pose_error  # noqa: F401
from .localization import localize, match_pairs, run_pnp, run_pnp_batch, subsample_indices, undistort_points  # noqa: F401
