"""Times the one-bounce light from the material mesh (libmrgs.so: bounce_shade_fwd / _bwd behind RayTracer.shade and
shading.raytraced_indirect_light) at 800^2 and 1600^2 rays against make_occluder_mesh(1_000_000) with random vertex attributes, forward
and forward+backward (gradients to the environment's base level, every prefiltered level and the four material tables), each alternating
in one process with the fp32 torch form of the same statements on the device: the existing trace, EnvLight calls and boolean indexing,
which is what the reference writes (raytracing_brdf/raytracer.py:218-297, utils/refl_utils.py:118-147; every ray with its own FG pair).
Rays: the bench scene's shaded pixels -- every pixel of an orbit camera whose ray meets the unit sphere the shell scene lives on, with the
sphere's normal there; the other pixels are inactive.  Device events after warm-up over 3 batches of 20 native and 5 torch calls, the
minimum and all batches printed; also the trace alone (the launch `shade` starts with), the host time of one native call (wall clock, the
queue drained once at the end) and the algorithmic bytes of the shade kernel.  Per-kernel times, in a run of its own (--profile: one
short batch of each, so that the trace stays small):
    rocprofv3 --kernel-trace --stats -d OUT -o b -- python tools/bounce_time.py --profile
Developer tool; prints three lines per size."""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from materialrefgs_amd import shading  # noqa: E402
from materialrefgs_amd.gs_utils import safe_normalize  # noqa: E402
from materialrefgs_amd.mesh import TriangleMesh  # noqa: E402
from materialrefgs_amd.raytracing import RayTracer  # noqa: E402
from materialrefgs_amd.synthetic import make_occluder_mesh, orbit_camera  # noqa: E402

TABLES = ("diffuse", "albedo", "metallic", "roughness")


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def material_tracer(dev, n_triangles):
    v, t = make_occluder_mesh(n_triangles)
    g = torch.Generator().manual_seed(0)
    V = v.shape[0]
    vt = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    normal = torch.nn.functional.normalize(vt + 0.2 * torch.randn(V, 3, generator=g), dim=-1)        # about the spheres' own normals
    cols = [("rgb", torch.rand(V, 3, generator=g)), ("normal", normal), ("diffuse", torch.rand(V, 3, generator=g)),
            ("base_color", torch.rand(V, 3, generator=g)), ("metallic", torch.rand(V, 1, generator=g)), ("roughness", torch.rand(V, 1, generator=g))]
    layout, at = {}, 0
    for name, c in cols:
        layout[name] = slice(at, at + c.shape[1])
        at += c.shape[1]
    mesh = TriangleMesh(vt.to(dev), torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(dev),
                        attributes=torch.cat([c for _, c in cols], dim=1).contiguous().to(dev), layout=layout)
    return RayTracer.from_mesh(mesh, device=dev, normal_encoding="signed")


def shaded_pixels(cam, H, dev):
    """(surface points on the unit sphere, unit normals, unit view directions off the surface, mask of the pixels that meet it), [H H,*]."""
    K = torch.as_tensor(cam.HWK[2], dtype=torch.float32, device=dev)
    c2w = cam.world_view_transform.to(dev).T.inverse()
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32), indexing="ij")
    d = safe_normalize((torch.stack([xs, ys, torch.ones_like(xs)], dim=-1) @ torch.linalg.inv(K).T) @ c2w[:3, :3].T).reshape(-1, 3)
    o = c2w[:3, 3].expand_as(d)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - 1.0)
    x = o + (-b - torch.sqrt(disc.clamp_min(0)))[:, None] * d
    return x.contiguous(), safe_normalize(x), (-d).contiguous(), disc > 0


def torch_bounce(rt, env, hit_pos, view, ids, depth):
    """secondary_indirect_color as the reference writes it, fp32 torch ops and EnvLight calls, every ray with its own FG pair."""
    out = torch.zeros_like(hit_pos)
    hit = depth < 10.0
    if (~hit).sum() > 0:                                              # raytracer.py:230 (a host read; EnvLight refuses an empty batch)
        out[~hit] = env(-view[~hit], mode="pure_env")
    p, v = hit_pos[hit], view[hit]
    vid = rt.triangles[ids[hit].long()].long()
    vp = rt.vertices[vid]

    def area(v1, v2, v3):
        return 0.5 * torch.abs(v1[..., 0] * (v2[..., 1] - v3[..., 1]) + v2[..., 0] * (v3[..., 1] - v1[..., 1]) + v3[..., 0] * (v1[..., 1] - v2[..., 1]))
    a, b, c = vp[:, 0], vp[:, 1], vp[:, 2]
    w = torch.stack([area(p, b, c), area(p, c, a), area(p, a, b)], dim=-1).unsqueeze(-1)
    den = area(a, b, c).unsqueeze(-1)
    at = rt.vertex_attrs
    interp = lambda tab: (w * tab[vid]).sum(dim=1) / den   # noqa: E731
    diffuse, m, r, albedo, n = interp(at["diffuse"]), interp(at["metallic"]), interp(at["roughness"]), interp(at["albedo"]), interp(rt.decoded_normals())
    ndv = torch.sum(v * n, dim=-1, keepdim=True)
    l = safe_normalize(2 * n * ndv - v)
    fg = shading._lut_fetch(shading.load_fg_lut(p.device), torch.cat([ndv, r], -1).clamp(0, 1))
    light = env(l, roughness=r)
    out[hit] = torch.nan_to_num((1 - m) * diffuse + ((0.04 * (1 - m) + albedo * m) * fg[..., 0:1] + fg[..., 1:2]) * light, nan=0.0, posinf=0.0, neginf=0.0)
    return out


def torch_shade(rt, env, pos, n, v, mask):
    """shade on the masked pixels, compacted, as utils/refl_utils.py:143-146 calls it."""
    pos, n, v = pos[mask], n[mask], v[mask]
    inc = 2.0 * n * torch.sum(v * n, dim=-1, keepdim=True) - v
    hit_pos, _, depth, ids = rt.trace(pos, inc, return_faceids=True)
    return torch_bounce(rt, env, hit_pos, -inc, ids, depth)


def torch_indirect(rt, env, HWK, R, T, normal_map, prior, alpha):
    """utils/refl_utils.py:118-147 (rend_surf_points = True)."""
    H, W, _ = HWK
    Rw = R.T
    rays_o = (-Rw.T @ T.unsqueeze(-1)).flatten()
    rays_cam = ((shading._pixel_camera(HWK, normal_map.device) - T[None, None]).reshape(-1, 3) @ Rw - rays_o[None]).reshape(H, W, 3)
    mask = (alpha > 0)[..., 0]
    w_o = safe_normalize(-rays_cam)
    rays_refl = safe_normalize(2 * normal_map * torch.sum(w_o * normal_map, dim=-1, keepdim=True) - w_o)
    surf, _, _ = rt.trace(rays_o[None, None].expand_as(rays_cam).reshape(-1, 3), safe_normalize(rays_cam).reshape(-1, 3))
    surf = surf.reshape(H, W, 3)
    _, _, depth = rt.trace(surf[mask], rays_refl[mask])
    visibility = torch.ones_like(alpha)
    visibility[mask] = (depth >= 10.0).float().unsqueeze(-1)
    mc = mask.clone()
    mc[mask] = depth < 10.0
    light = torch.zeros(H, W, 3, device=alpha.device)
    light[mc] = torch_shade(rt, env, surf.reshape(-1, 3), prior.reshape(-1, 3), w_o.reshape(-1, 3), mc.reshape(-1))
    return visibility, light


def main():
    dev = torch.device("cuda:0")
    profile = "--profile" in sys.argv[1:]
    sizes = [int(a) for a in sys.argv[1:] if a != "--profile"] or [800, 1600]
    batches, n_native, n_torch = (1, 5, 2) if profile else (3, 20, 5)
    rt = material_tracer(dev, 1_000_000)
    env = shading.EnvLight(device=dev, trainable=True)
    with torch.no_grad():
        env.base.copy_(torch.randn(env.base.shape, generator=torch.Generator().manual_seed(1)).to(dev))
    env.build_mips()
    env.specular = [m.detach().clone().requires_grad_(True) for m in env.specular]       # leaves: the backward timed is the bounce's own
    for k in TABLES:
        rt.vertex_attrs[k].requires_grad_(True)
    leaves = [env.base] + list(env.specular) + [rt.vertex_attrs[k] for k in TABLES]
    pc = SimpleNamespace(ray_tracer=rt)
    for H in sizes:
        cam = orbit_camera(0, H, H).to(dev)
        pos, n, v, mask = shaded_pixels(cam, H, dev)
        HWK = (H, H, np.asarray(cam.HWK[2], dtype=np.float32))
        R, T = torch.as_tensor(cam.R, dtype=torch.float32, device=dev), torch.as_tensor(cam.T, dtype=torch.float32, device=dev)
        normal_map, alpha = n.reshape(H, H, 3), mask.float().reshape(H, H, 1)
        inc = 2.0 * n * torch.sum(v * n, dim=-1, keepdim=True) - v
        depth = rt.trace(pos, inc)[2]
        n_hit = int(((depth < 10) & mask).sum())
        forms = {
            "shade": (lambda: rt.shade(pos, n, v, None, None, None, 32, env, active=mask), lambda: torch_shade(rt, env, pos, n, v, mask)),
            "raytraced_indirect_light": (lambda: shading.raytraced_indirect_light(env, HWK, R, T, normal_map, normal_map, alpha, pc)["indirect_light_raytracing"],
                                         lambda: torch_indirect(rt, env, HWK, R, T, normal_map, normal_map, alpha)[1]),
        }
        t_trace = min(timed(lambda: rt.trace(pos, inc, return_faceids=True), n_native) for _ in range(batches + 1))
        print(f"{H}x{H}: {int(mask.sum())} shaded pixels of {H * H}, {n_hit} mirror rays meet the mesh; the trace alone {t_trace:.3f} ms; the shade kernel "
              f"reads 33 B and writes 12 B per ray, gathers 3 x (8 + 48) B per hit ray and fetches 8 texels (96 B) of the environment and 4 x 8 B of the "
              f"FG table", flush=True)
        for what, (native, torch_form) in forms.items():
            fb = lambda f: (lambda: torch.autograd.grad(f().sum(), leaves, allow_unused=True))   # noqa: E731
            runs = {}
            for label, f, reps in (("native fwd", native, n_native), ("torch fwd", torch_form, n_torch), ("native fwd+bwd", fb(native), n_native),
                                   ("torch fwd+bwd", fb(torch_form), n_torch)):
                for _ in range(2):
                    f()
                torch.cuda.synchronize()
                runs[label] = [timed(f, reps) for _ in range(batches)]
            t0 = time.perf_counter()
            for _ in range(n_native):
                native()
            host = (time.perf_counter() - t0) / n_native * 1e3
            torch.cuda.synchronize()
            fmt = lambda xs: ", ".join(f"{x:.3f}" for x in xs)   # noqa: E731
            m = {k: min(x) for k, x in runs.items()}
            print(f"{H}x{H} {what}: native fwd {m['native fwd']:.3f} ms, fwd+bwd {m['native fwd+bwd']:.3f} ms (host {host:.3f} ms per forward call); "
                  f"fp32 torch form fwd {m['torch fwd']:.3f} ms, fwd+bwd {m['torch fwd+bwd']:.3f} ms; ratio {m['torch fwd'] / m['native fwd']:.1f}x / "
                  f"{m['torch fwd+bwd'] / m['native fwd+bwd']:.1f}x (batches {' / '.join(fmt(runs[k]) for k in runs)})", flush=True)


if __name__ == "__main__":
    main()
