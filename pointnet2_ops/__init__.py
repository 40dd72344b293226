"""`import pointnet2_ops` resolves to the MI355X implementation (materialrefgs_amd.ballquery -> libmrgs.so).

The reference's utils/ref_score_utils.py:1 imports `ball_query` and `furthest_point_sample` from `pointnet2_ops.pointnet2_utils`, a
CUDA-only extension that its tree does not carry; with this repository's root on the path, `pointnet2_ops/pointnet2_utils.py` takes that
module's place.  See INTEGRATION.md.
"""
