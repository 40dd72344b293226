"""Mesh ray queries behind the reference's `RayTracer` (submodules/raytracing/raytracing/raytracer.py:8-56 and the variant the
training code constructs, raytracing_brdf/raytracer.py:18-297: `RayTracer(vertices, triangles, ply_path=None)`, `.trace(rays_o, rays_d,
inplace=False[, return_faceids=False]) -> positions, face_normals, depth[, triangle ids]`, `.shade(...)`,
`.secondary_indirect_color(...)`).  The hierarchy is built on the host by libmrgs.so (`mrgs_bvh_build`, csrc/mrgs_bvh.hip) and traversed
on the GPU (`mrgs_bvh_trace`); depth = 10 marks a miss (utils/refl_utils.py:390-391 tests `depth >= 10`).  Face ids index the
`triangles` array that was passed in (the reference returns build-order ids and maps them back with `trans_ids`; here the mapping
happens inside the kernel).

A tracer built from a material mesh (`ply_path=...`, a file of io.save_material_ply, or `RayTracer.from_mesh`) also carries the
per-vertex material `vertex_attrs` and shades one mirror bounce with it: `mrgs_bounce_shade_forward / _backward` (csrc/mrgs_bounce.hip;
the contract and the three places where this differs from the reference's text on purpose are in include/mrgs.h and INTEGRATION.md)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._camconst import kinv

ATTRIBUTE_NAMES = ("diffuse", "albedo", "normal", "metallic", "roughness")     # the `prefix_*` groups of the reference's reader (:59-75)
_WIDTHS = {"diffuse": 3, "albedo": 3, "normal": 3, "metallic": 1, "roughness": 1}
_MESH_GROUPS = {"diffuse": "diffuse", "albedo": "base_color", "normal": "normal", "metallic": "metallic", "roughness": "roughness"}


class _BounceShade(torch.autograd.Function):
    """out[N,3] of mrgs_bounce_shade_forward; gradients to the base level, to every level of the prefiltered chain and to the diffuse,
    albedo, metallic and roughness tables.  The rays, the mesh and the normal table are constants."""

    @staticmethod
    def forward(ctx, consts, base, n_spec, *rest):
        from . import shading
        spec, (diffuse, albedo, metallic, roughness) = [m.contiguous() for m in rest[:n_spec]], rest[n_spec:]
        pos, view, ids, depth, active, vertices, triangles, normal, lut, rough_range = consts
        base = base.contiguous()
        table = torch.cat([diffuse, albedo, metallic, roughness, normal, normal.new_zeros((normal.shape[0], 1))], dim=1).contiguous()
        N = pos.shape[0]
        out = torch.empty((N, 3), dtype=torch.float32, device=pos.device)
        cfg = _lib.MrgsBounceConfig(0, N, vertices.shape[0], triangles.shape[0], base.shape[1], lut.shape[0])
        ms = shading._mips_struct(spec, None, *rough_range)
        p = _lib.ptr
        with _lib.guard(pos.device):
            _lib.check(_lib.lib().mrgs_bounce_shade_forward(ctypes.byref(cfg), ctypes.byref(ms), p(base), p(pos), p(view), p(ids), p(depth),
                                                            p(active), p(vertices), p(triangles), p(table), p(lut), p(out),
                                                            _lib.stream_ptr(pos.device)))
        ctx.consts, ctx.n_spec, ctx.cfg = consts, n_spec, cfg
        ctx.save_for_backward(base, table, *spec)
        return out

    @staticmethod
    def backward(ctx, g_out):
        from . import shading
        base, table, *spec = ctx.saved_tensors
        pos, view, ids, depth, active, vertices, triangles, _normal, lut, rough_range = ctx.consts
        n = ctx.n_spec
        need = ctx.needs_input_grad
        g_out = g_out.contiguous().float()
        grads = shading._grad_buffers([base] + spec, [need[1]] + [need[3 + i] for i in range(n)])
        want_table = any(need[3 + n:3 + n + 4])
        g_table = torch.zeros((vertices.shape[0], 8), dtype=torch.float32, device=pos.device) if want_table else None
        ms = shading._mips_struct(spec, grads[1:], *rough_range)
        p = _lib.ptr
        with _lib.guard(pos.device):
            _lib.check(_lib.lib().mrgs_bounce_shade_backward(ctypes.byref(ctx.cfg), ctypes.byref(ms), p(base), p(grads[0]), p(pos), p(view),
                                                             p(ids), p(depth), p(active), p(vertices), p(triangles), p(table), p(lut),
                                                             p(g_out), p(g_table), _lib.stream_ptr(pos.device)))
        g_env = shading._sum_copies(grads)
        g_tabs = [None] * 4
        if want_table:
            g_tabs = [g_table[:, 0:3], g_table[:, 3:6], g_table[:, 6:7], g_table[:, 7:8]]
            g_tabs = [g if need[3 + n + k] else None for k, g in enumerate(g_tabs)]
        return (None, g_env[0], None, *g_env[1:], *g_tabs)


class RayTracer:
    def __init__(self, vertices, triangles, ply_path=None, device=None, normal_encoding="reference"):
        if normal_encoding not in ("reference", "signed"):
            raise ValueError(f"normal_encoding is 'reference' (the file's normal columns go through * 2 - 1, raytracer.py:245) or 'signed' "
                             f"(taken as stored), not {normal_encoding!r}")
        attrs = None
        if ply_path is not None:
            from . import io
            d = io.load_material_ply(ply_path)
            vertices, triangles = d["vertices"].astype(np.float32), d["triangles"]       # positions narrowed as raytracer.py:34 does
            attrs = {name: d[_MESH_GROUPS[name]] for name in ATTRIBUTE_NAMES}
        if torch.is_tensor(vertices):
            vertices = vertices.detach().cpu().numpy()
        if torch.is_tensor(triangles):
            triangles = triangles.detach().cpu().numpy()
        vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        triangles = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        if not triangles.shape[0] > 8:                                            # raytracer.py:15
            raise AssertionError(f"RayTracer needs more than 8 triangles for its BVH, got {triangles.shape[0]}: post_process_mesh removes every "
                                 "cluster of fewer than 50 triangles, so an extraction whose largest cluster is smaller leaves an empty mesh")
        self.n_triangles = int(triangles.shape[0])
        lib = _lib.lib()
        nbytes = lib.mrgs_bvh_bytes(self.n_triangles)
        blob = torch.empty(nbytes, dtype=torch.uint8)
        _lib.check(lib.mrgs_bvh_build(ctypes.c_void_p(vertices.ctypes.data), vertices.shape[0], ctypes.c_void_p(triangles.ctypes.data),
                                      self.n_triangles, ctypes.c_void_p(blob.data_ptr()), nbytes))
        self.blob_host = blob
        self.device = torch.device(device) if device is not None else (torch.device("cuda") if torch.cuda.is_available() else None)
        self.blob = blob.to(self.device) if self.device is not None else None
        self.normal_encoding = normal_encoding
        self.vertex_attrs = self.vertices = self.triangles = None
        if attrs is not None:
            self._set_attributes(attrs, vertices, triangles)

    @classmethod
    def from_mesh(cls, mesh, device=None, normal_encoding="reference"):
        """The tracer of a mesh.TriangleMesh that carries the groups diffuse, base_color, normal, metallic and roughness (what
        GaussianExtractor.extract_mesh_bouned_with_material returns), without the file in between."""
        missing = [g for g in _MESH_GROUPS.values() if mesh.layout is None or g not in mesh.layout]
        if missing:
            raise ValueError(f"RayTracer.from_mesh: the mesh carries no vertex attribute group {missing}")
        self = cls(mesh.vertices, mesh.triangles, device=device, normal_encoding=normal_encoding)
        self._set_attributes({name: mesh.attribute(_MESH_GROUPS[name])[:, :_WIDTHS[name]] for name in ATTRIBUTE_NAMES},
                             np.ascontiguousarray(mesh.vertices, dtype=np.float32).reshape(-1, 3),
                             np.ascontiguousarray(mesh.triangles, dtype=np.int32).reshape(-1, 3))
        return self

    def _set_attributes(self, attrs, v, t):
        """vertices / triangles as device tensors and `vertex_attrs` {diffuse, albedo, normal [V,3], metallic, roughness [V,1]} fp32,
        the values as the file holds them (raytracer.py:34-37)."""
        dev = self.device if self.device is not None else torch.device("cpu")
        self.vertices = torch.from_numpy(v).to(dev).contiguous()
        self.triangles = torch.from_numpy(t).to(dev).contiguous()
        out = {}
        for name in ATTRIBUTE_NAMES:
            a = attrs[name]
            a = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
            a = a.to(device=dev, dtype=torch.float32).reshape(v.shape[0], -1).contiguous()
            if a.shape[1] != _WIDTHS[name]:
                raise ValueError(f"vertex attribute {name!r} must be [V,{_WIDTHS[name]}], got {tuple(a.shape)}")
            out[name] = a
        self.vertex_attrs = out

    def _need_attributes(self, what):
        missing = list(ATTRIBUTE_NAMES) if self.vertex_attrs is None else [n for n in ATTRIBUTE_NAMES if n not in self.vertex_attrs]
        if missing:
            raise ValueError(f"RayTracer.{what} needs the vertex attributes {missing}: build the tracer from a material mesh "
                             "(ply_path=... or RayTracer.from_mesh)")

    def decoded_normals(self):
        """The normal table the shading reads: `vertex_attrs["normal"]` through * 2 - 1 with normal_encoding="reference", as stored with
        "signed"."""
        n = self.vertex_attrs["normal"].detach()
        return n * 2.0 - 1.0 if self.normal_encoding == "reference" else n

    def trace(self, rays_o, rays_d, inplace=False, return_faceids=False):
        if self.blob is None:
            raise RuntimeError("materialrefgs_amd.raytracing needs a GPU (libmrgs.so has no CPU traversal)")
        rays_o = rays_o.float().contiguous()
        rays_d = rays_d.float().contiguous()
        if not rays_o.is_cuda:
            rays_o = rays_o.to(self.device)
        if not rays_d.is_cuda:
            rays_d = rays_d.to(self.device)
        prefix = rays_o.shape[:-1]
        rays_o, rays_d = rays_o.view(-1, 3), rays_d.view(-1, 3)
        N = rays_o.shape[0]
        positions = rays_o if inplace else torch.empty_like(rays_o)
        face_normals = rays_d if inplace else torch.empty_like(rays_d)
        depth = torch.empty(N, dtype=torch.float32, device=rays_o.device)
        ids = torch.empty(N, dtype=torch.int32, device=rays_o.device) if return_faceids else None
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        with _lib.guard(rays_o.device):
            st = _lib.stream_ptr(rays_o.device)
            _lib.check(_lib.lib().mrgs_bvh_trace(p(self.blob), self.n_triangles, N, p(rays_o), p(rays_d), p(positions), p(face_normals),
                                                 p(depth), p(ids), st))
        positions, face_normals, depth = positions.view(*prefix, 3), face_normals.view(*prefix, 3), depth.view(*prefix)
        if not return_faceids:
            return positions, face_normals, depth
        return positions, face_normals, depth, ids.view(*prefix)

    def secondary_indirect_color(self, surface_pos, rays_v, face_normals, triangle_indices, hit_depth, env_map, active=None):
        """raytracer.py:218-271 in one launch: [N,3], per ray the environment along -rays_v where the ray left the scene (hit_depth >= 10),
        otherwise the hit point's own material -- interpolated from the three vertices of triangle `triangle_indices` -- shaded with the
        split-sum terms against `env_map`'s prefiltered chain.  Every ray uses its own FG pair (the reference's text takes the first hit
        ray's for all).  `face_normals` is accepted and unused, as in the reference.  `active` [N] bool / uint8: rays with 0
        write zeros and receive no gradient.  Differentiable to env_map.base (through build_mips), env_map.specular and the diffuse,
        albedo, metallic and roughness entries of `vertex_attrs`."""
        from . import shading
        self._need_attributes("secondary_indirect_color")
        if self.blob is None:
            raise RuntimeError("materialrefgs_amd.raytracing needs a GPU (libmrgs.so has no CPU fallback)")
        dev = self.vertices.device
        pos = _lib.f32c(surface_pos).reshape(-1, 3)
        view = _lib.f32c(rays_v).reshape(-1, 3)
        depth = _lib.f32c(hit_depth).reshape(-1)
        ids = triangle_indices.detach().reshape(-1)
        ids = ids if ids.dtype == torch.int32 else ids.to(torch.int32)
        ids = ids.contiguous()
        N = pos.shape[0]
        if not (view.shape[0] == depth.shape[0] == ids.shape[0] == N):
            raise ValueError("secondary_indirect_color: surface_pos, rays_v, triangle_indices and hit_depth must describe the same N rays")
        if active is not None:
            active = active.detach().reshape(-1)
            active = (active.view(torch.uint8) if active.dtype == torch.bool else active.to(torch.uint8)).contiguous()
            if active.shape[0] != N:
                raise ValueError("secondary_indirect_color: `active` must be [N]")
        a = self.vertex_attrs
        consts = (pos, view, ids, depth, active, self.vertices, self.triangles, self.decoded_normals(), shading.load_fg_lut(dev),
                  (env_map.min_roughness, env_map.max_roughness))
        spec = list(env_map.specular)
        return _BounceShade.apply(consts, env_map.base, len(spec), *spec, a["diffuse"], a["albedo"], a["metallic"], a["roughness"])

    def shade(self, surface_pos, rays_n, rays_v, roughness, metallic, albedo, num_samples, envmap, active=None):
        """raytracer.py:274-297: the mirror ray of every surface point (normal rays_n, view direction rays_v off the surface, both
        expected at UNIT length: like the reference, the mirror direction 2 n (n . v) - v is not normalised before the trace) against the
        mesh, then secondary_indirect_color on what the trace reports.  roughness, metallic, albedo and num_samples are accepted and
        unused, as in the reference.  No host read."""
        self._need_attributes("shade")
        rays_n, rays_v = rays_n.detach().float().reshape(-1, 3), rays_v.detach().float().reshape(-1, 3)
        incident = 2.0 * rays_n * torch.sum(rays_v * rays_n, dim=-1, keepdim=True) - rays_v          # reflection(rays_v, rays_n)
        hit_pos, hit_normal, hit_depth, ids = self.trace(surface_pos.detach().reshape(-1, 3), incident, return_faceids=True)
        return self.secondary_indirect_color(hit_pos, -incident, hit_normal, ids, hit_depth, envmap, active=active)

    def get_materials_by_faceids(self, surf_points, face_ids):
        """(diffuse [N,3], refl_strength [N,1], roughness [N,1], albedo [N,3], normal_map [N,3]) at `surf_points` on the triangles
        `face_ids`: the gather and interpolation of secondary_indirect_color alone, under the name and in the order of
        raytracer_optimizable.py:281-298 but without that variant's clamps and sigmoid (this follows raytracer.py).  Element-wise torch
        on the caller's device; every id must name a triangle."""
        self._need_attributes("get_materials_by_faceids")
        vid = self.triangles[face_ids.reshape(-1).long()].long()                              # [N,3]
        vp = self.vertices[vid]                                                               # [N,3,3]
        p = surf_points.reshape(-1, 3).float()

        def area(v1, v2, v3):                                                                 # barycentric_interpolation, :209-216
            return 0.5 * torch.abs(v1[..., 0] * (v2[..., 1] - v3[..., 1]) + v2[..., 0] * (v3[..., 1] - v1[..., 1]) +
                                   v3[..., 0] * (v1[..., 1] - v2[..., 1]))
        a, b, c = vp[:, 0], vp[:, 1], vp[:, 2]
        w = torch.stack([area(p, b, c), area(p, c, a), area(p, a, b)], dim=-1)                # [N,3]
        den = area(a, b, c).unsqueeze(-1)

        def interp(table):
            return (w.unsqueeze(-1) * table[vid]).sum(dim=1) / den
        at = self.vertex_attrs
        return (interp(at["diffuse"]), interp(at["metallic"]), interp(at["roughness"]), interp(at["albedo"]), interp(self.decoded_normals()))

    def visibility(self, HWK, R, T, normal_map, render_alpha, surf_depth):
        """The visibility block of get_specular_color_surfel (utils/refl_utils.py:379-391) as one launch: normal_map [H,W,3],
        render_alpha [H,W,1], surf_depth [1,H,W] -> visibility [H,W,1] (1 = the mirror ray is free for 10 units or alpha <= 0).
        Not differentiable (the reference's is a comparison)."""
        if self.blob is None:
            raise RuntimeError("materialrefgs_amd.raytracing needs a GPU (libmrgs.so has no CPU traversal)")
        H, W, K = HWK
        kin = (ctypes.c_float * 9)(*kinv(K))
        nm, al = normal_map.detach().float(), render_alpha.detach().float()
        sd = surf_depth.detach().float().contiguous()
        Rc, Tc = R.detach().float().contiguous(), T.detach().float().contiguous()
        vis = torch.empty((H, W, 1), dtype=torch.float32, device=nm.device)
        m_n = _lib.MrgsStridedMap(nm.data_ptr(), nm.stride(0), nm.stride(1), nm.stride(2))
        m_a = _lib.MrgsStridedMap(al.data_ptr(), al.stride(0), al.stride(1), al.stride(2) if al.dim() > 2 else 0)
        with _lib.guard(nm.device):
            st = _lib.stream_ptr(nm.device)
            _lib.check(_lib.lib().mrgs_bvh_visibility(ctypes.c_void_p(self.blob.data_ptr()), self.n_triangles, H, W, kin,
                                                      ctypes.c_void_p(Rc.data_ptr()), ctypes.c_void_p(Tc.data_ptr()), ctypes.byref(m_n),
                                                      ctypes.byref(m_a), ctypes.c_void_p(sd.data_ptr()), ctypes.c_void_p(vis.data_ptr()), st))
        return vis
