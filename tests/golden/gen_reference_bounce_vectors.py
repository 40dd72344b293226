"""Generates tests/golden/reference_bounce.npz by running the REFERENCE'S OWN raytracing_brdf/raytracer.py on the CPU in float32:
`RayTracer.secondary_indirect_color` (:218-271) and `RayTracer.shade` (:274-297) with scene/light.py's EnvLight (`__call__`, `get_mip`).

Stand-ins, the ones tests/golden/gen_reference_render_vectors.py uses, for the leaves that are not vendored:
    nvdiffrast.torch.texture -> oracle/shading_oracle.py (lut_fetch, cube_fetch + trilinear)
    _raytracing_brdf         -> oracle/trace_oracle.py brute force
    plyfile, ipdb, imageio, simple_knn, cubemapencoder, diff_surfel_tracing, the rasterizer's _C, ...
                             -> empty placeholders (importing scene.light imports the whole model; none is called on this path)
`.cuda()` / device="cuda" map to the CPU.  The FG table is this repository's (the reference's asset is not redistributed); the working
directory is the reference while it is imported, because raytracer.py opens ./assets/bsdf_256_256.bin at import.  The environment's
prefiltered chain is set to seeded tensors (EnvLight.build_mips needs the un-vendored renderutils plugin and is pinned elsewhere); the
mesh, its `vertex_attrs` (normals ENCODED, so that the reader's `* 2 - 1` at :245 yields the table the statement takes) and the rays
come from tests/bounce_statement.py.

Only inputs and outputs are stored; the reference source never travels.

    python tests/golden/gen_reference_bounce_vectors.py        # needs the reference checkout at /root/reference; a few seconds
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)                            # the reference's raytracing_brdf must win over the shim package at the repository root
sys.path.insert(0, os.path.join(REF, "submodules", "diff-surfel-rasterization"))

from oracle import shading_oracle as so        # noqa: E402
from oracle import trace_oracle as to          # noqa: E402
import bounce_statement as bs                  # noqa: E402

N_RAYS = 1031


def _cpu(v):
    if isinstance(v, str) and v.startswith("cuda"):
        return "cpu"
    if isinstance(v, torch.device) and v.type == "cuda":
        return torch.device("cpu")
    return v


class _CudaIsCpu(torch.overrides.TorchFunctionMode):
    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = kwargs or {}
        if getattr(func, "__name__", "") == "cuda" and args and isinstance(args[0], torch.Tensor):
            return args[0]
        return func(*[_cpu(a) for a in args], **{k: _cpu(v) for k, v in kwargs.items()})


_CudaIsCpu().__enter__()


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _never(*a, **k):
    raise RuntimeError("a placeholder module was called: this path is not supposed to reach it")


def _dr_texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None):
    """The call shapes of this path: FG table (linear, clamp; raytracer.py:259), one cubemap level (linear, cube; light.py:114) and the
    chain with an explicit level (linear-mipmap-linear, cube; light.py:118-125)."""
    assert uv_da is None and max_mip_level is None
    if boundary_mode == "clamp":
        assert filter_mode == "linear" and tex.dim() == 4 and tex.shape[0] == 1 and mip is None
        return so.lut_fetch(tex[0], uv.reshape(-1, 2)).reshape(*uv.shape[:-1], tex.shape[-1])
    assert boundary_mode == "cube" and tex.dim() == 5 and tex.shape[0] == 1
    dirs = uv.reshape(-1, 3)
    if mip is None:
        assert filter_mode == "linear"
        out = so.cube_fetch(tex[0], dirs)
    else:
        assert filter_mode == "linear-mipmap-linear"
        levels = [tex[0]] + [m[0] for m in mip]
        n = len(levels)
        lc = torch.clamp(mip_level_bias.reshape(-1), 0, n - 1)
        l0 = torch.clamp(torch.floor(lc).detach().long(), max=n - 1)
        l1 = torch.clamp(l0 + 1, max=n - 1)
        f = lc - l0.to(lc.dtype)
        samples = torch.stack([so.cube_fetch(m, dirs) for m in levels], 0)
        ar = torch.arange(dirs.shape[0])
        out = (1 - f).unsqueeze(-1) * samples[l0, ar] + f.unsqueeze(-1) * samples[l1, ar]
    return out.reshape(*uv.shape[:-1], tex.shape[-1])


class _BruteForceTracer:
    """`_backend.create_raytracer(vertices, triangles)`; `.trace(...)` fills its four outputs in place (raytracer.py:112)."""

    def __init__(self, vertices, triangles):
        self.v, self.t = np.asarray(vertices, dtype=np.float32), np.asarray(triangles, dtype=np.int64)

    def trace(self, rays_o, rays_d, positions, face_normals, depth, triangle_indices):
        pos, nrm, dpt, ids = to.trace(self.v, self.t, rays_o.detach().numpy(), rays_d.detach().numpy())
        positions.copy_(torch.from_numpy(pos))
        face_normals.copy_(torch.from_numpy(nrm))
        depth.copy_(torch.from_numpy(dpt))
        triangle_indices.copy_(torch.from_numpy(ids.astype(np.int32)))

    def get_triangels_ids_mapping(self):
        return torch.arange(self.t.shape[0], dtype=torch.int32)          # the brute force reports ids in the caller's order


for _n in ("cv2", "imageio", "kornia", "kornia.filters", "lpips", "open3d", "mediapy", "torchvision", "simple_knn"):
    _placeholder(_n)
_placeholder("ipdb", set_trace=_never)
# (importing scene.light runs scene/__init__.py, which imports the whole model: its native leaves are never called here)
_placeholder("simple_knn._C", distCUDA2=_never)
_placeholder("cubemapencoder", CubemapEncoder=type("CubemapEncoder", (), {}))
_placeholder("diff_surfel_tracing", SurfelTracer=_never, SurfelTracingSettings=_never)
_placeholder("diff_surfel_rasterization._C", rasterize_gaussians=_never, rasterize_gaussians_backward=_never, mark_visible=_never)
_placeholder("plyfile", PlyData=type("PlyData", (), {}), PlyElement=type("PlyElement", (), {}))
_placeholder("nvdiffrast")
sys.modules["nvdiffrast"].torch = _placeholder("nvdiffrast.torch", texture=_dr_texture)
_placeholder("_raytracing_brdf", create_raytracer=_BruteForceTracer)

os.chdir(REF)
from raytracing_brdf import raytracer as ref_rt            # noqa: E402
from scene.light import EnvLight as RefEnvLight            # noqa: E402
assert ref_rt.__file__.startswith(REF), ref_rt.__file__
os.chdir(ROOT)

OUR_LUT = torch.from_numpy(np.load(os.path.join(ROOT, "materialrefgs_amd", "assets", "fg_lut_256.npy")).astype(np.float32))
ref_rt.FG_LUT = OUR_LUT.reshape(1, 256, 256, 2)


def make_env(base, spec):
    """A reference EnvLight around the given tensors, without build_mips (see the module docstring)."""
    env = RefEnvLight.__new__(RefEnvLight)
    torch.nn.Module.__init__(env)
    env.min_roughness, env.max_roughness = 0.08, 0.5
    env.base = torch.nn.Parameter(base.clone(), requires_grad=True)
    env.specular = [m.clone().requires_grad_(True) for m in spec]
    return env


def main():
    sc = bs.scene(seed=0, n_rays=N_RAYS)
    # Ray 0 becomes the hit ray that meets its surface at the most grazing angle: raytracer.py:263 weights EVERY hit ray with the FG pair of
    # the first one, and the grazing pair is the one furthest from the others' own -- the quirk at its plainest.
    inc0 = bs.incident(sc["rays_n"], sc["rays_v"])
    p0, _, d0, i0 = bs.trace_cpu(sc, sc["surface_pos"], inc0)
    hits = torch.nonzero(d0 < 10)[:, 0]
    nrm0 = bs.gather(p0[hits], i0[hits], sc["vertices"], sc["triangles"], {"normal": sc["tables"]["normal"]})[0]["normal"]
    grazing = int(hits[torch.argmin(torch.sum(nrm0 * -inc0[hits], dim=-1))])
    for k in ("surface_pos", "rays_n", "rays_v"):
        sc[k][[0, grazing]] = sc[k][[grazing, 0]]
    base, spec = bs.environment(seed=0)
    tracer = ref_rt.RayTracer.__new__(ref_rt.RayTracer)
    tracer.impl = _BruteForceTracer(sc["vertices"].numpy(), sc["triangles"].numpy())
    tracer.mappings = tracer.impl.get_triangels_ids_mapping()
    tracer.vertices, tracer.triangles = sc["vertices"], sc["triangles"].long()
    tab = sc["tables"]
    tracer.vertex_attrs = {k: tab[k].clone() for k in ("diffuse", "albedo", "metallic", "roughness")}
    tracer.vertex_attrs["normal"] = (tab["normal"] + 1.0) * 0.5            # the reader decodes with * 2 - 1
    store = {"vertices": sc["vertices"].numpy(), "triangles": sc["triangles"].numpy(), "surface_pos": sc["surface_pos"].numpy(),
             "rays_n": sc["rays_n"].numpy(), "rays_v": sc["rays_v"].numpy(), "env_base": base.numpy(),
             "normal_encoded": tracer.vertex_attrs["normal"].numpy()}
    for k, v in tab.items():
        store[f"table_{k}"] = v.numpy()
    for i, m in enumerate(spec):
        store[f"env_spec_{i}"] = m.numpy()

    inc = bs.incident(sc["rays_n"], sc["rays_v"])
    hit_pos, hit_nrm, depth, ids = tracer.trace(sc["surface_pos"], inc, return_faceids=True)
    store.update(hit_pos=hit_pos.numpy(), hit_depth=depth.numpy(), hit_ids=ids.numpy().astype(np.int32), incident=inc.numpy())
    g = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(5))
    store["upstream"] = g.numpy()
    for name, fn in (("sic", lambda env: tracer.secondary_indirect_color(hit_pos, -inc, hit_nrm, ids.long(), depth, env)),
                     ("shade", lambda env: tracer.shade(sc["surface_pos"], sc["rays_n"], sc["rays_v"], None, None, None, 32, env))):
        env = make_env(base, spec)
        out = fn(env)
        (out * g).sum().backward()
        store[f"{name}_out"] = out.detach().numpy()
        store[f"{name}_grad_base"] = env.base.grad.numpy()
        for i, m in enumerate(env.specular):
            store[f"{name}_grad_spec_{i}"] = m.grad.numpy()
    print("hit share", float((depth < 10).float().mean()), "largest output", float(np.abs(store["sic_out"]).max()))
    dst = os.path.join(HERE, "reference_bounce.npz")
    np.savez_compressed(dst, **store)
    print("wrote", dst, len(store), "arrays", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
