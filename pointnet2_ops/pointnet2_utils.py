"""`from pointnet2_ops.pointnet2_utils import ball_query, furthest_point_sample` resolves to the MI355X implementation
(materialrefgs_amd.ballquery -> libmrgs.so).

The reference imports the two at the top of utils/ref_score_utils.py:1 and calls them in ref_scores_max_pooling (:50, :58); with this
repository's root on the path instead of the CUDA extension those imports bind the HIP implementation unchanged: the same positional
arguments, int32 results, no graph.  Only these two names of pointnet2_utils are served.  See INTEGRATION.md.
"""
from materialrefgs_amd.ballquery import ball_query, furthest_point_sample  # noqa: F401

__all__ = ["ball_query", "furthest_point_sample"]
