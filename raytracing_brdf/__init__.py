"""`import raytracing_brdf` resolves to the MI355X mesh tracer (materialrefgs_amd.raytracing -> libmrgs.so).

The reference does `from raytracing_brdf import RayTracer` (scene/gaussian_model.py); its native backend `_raytracing_brdf` is not part
of the reference tree.  With this directory on the path the import binds the HIP implementation: `trace`, `shade`,
`secondary_indirect_color` and the material-mesh constructor (`ply_path=...`).  INTEGRATION.md lists the three places where `shade`
differs from the reference's text on purpose.
"""
from materialrefgs_amd.raytracing import RayTracer  # noqa: F401
from materialrefgs_amd.shading import raytraced_indirect_light  # noqa: F401

__all__ = ["RayTracer", "raytraced_indirect_light"]
