"""RayTracer.shade / secondary_indirect_color (mrgs_bounce_shade_forward / _backward, csrc/mrgs_bounce.hip) against the float64 statement
of tests/bounce_statement.py, and that statement against the reference's own recorded output (tests/golden/reference_bounce.npz,
written by tests/golden/gen_reference_bounce_vectors.py).

Bars: forward 1e-5 of the output's largest element, gradients 1e-4 of each gradient tensor's largest element (the project's bars for
forward terms and gradients); the CPU test `test_gpu_inputs_are_well_conditioned` holds the literal float32 reading of the statement and
its float32 autograd to half of them on the same inputs."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import bounce_statement as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_bounce.npz")
FWD_BAR, GRAD_BAR = 1e-5, 1e-4
TABLE_KEYS = ("diffuse", "albedo", "metallic", "roughness")


def _lut():
    return torch.from_numpy(np.load(os.path.join(ROOT, "materialrefgs_amd", "assets", "fg_lut_256.npy")).astype(np.float32))


# ---- the statement against the reference's recorded output -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    d = np.load(GOLDEN)
    return {k: torch.from_numpy(d[k]) for k in d.files}


def _golden_statement(order=None, first_row_fg=True):
    """The float64 statement on the fixture's inputs (rays permuted by `order`): (out, grad base, [grad level])."""
    d = _golden()
    idx = torch.arange(d["hit_pos"].shape[0]) if order is None else order
    base = d["env_base"].double().requires_grad_(True)
    spec = [d[f"env_spec_{i}"].double().requires_grad_(True) for i in range(3)]
    tables = {k: d[f"table_{k}"].double() for k in TABLE_KEYS + ("normal",)}
    out = bs.secondary_indirect_color(d["hit_pos"][idx].double(), -d["incident"][idx].double(), d["hit_ids"][idx], d["hit_depth"][idx],
                                      d["vertices"].double(), d["triangles"], tables, base, spec, _lut().double(), first_row_fg=first_row_fg)
    (out * d["upstream"][idx].double()).sum().backward()
    return out.detach(), base.grad, [m.grad for m in spec]


def test_statement_with_the_first_row_fg_reproduces_the_reference():
    """The reference's float32 output and environment gradients (secondary_indirect_color and shade, which agree bit for bit) sit within
    the float32-against-float64 distance of the statement with first_row_fg=True."""
    d = _golden()
    out, g_base, g_spec = _golden_statement()
    assert torch.equal(d["shade_out"], d["sic_out"])
    assert float(d["sic_out"].abs().max()) > 0.5 and 0.2 < float((d["hit_depth"] < 10).float().mean()) < 0.6
    assert float((out - d["sic_out"]).abs().max()) <= FWD_BAR * float(out.abs().max())
    for name, g in [("base", g_base)] + [(f"spec_{i}", g) for i, g in enumerate(g_spec)]:
        for run in ("sic", "shade"):
            ref = d[f"{run}_grad_{name}"]
            assert float(ref.abs().max()) > 0
            assert float((g - ref).abs().max()) <= GRAD_BAR * float(g.abs().max()), (run, name)


def test_the_first_row_fg_depends_on_ray_order_and_the_built_form_does_not():
    """raytracer.py:259-263 weights every hit ray with the FG pair of the FIRST hit ray: with that ray moved to the end the literal
    reading changes by more than 0.1 somewhere, the per-ray reading (what is built) by nothing."""
    d = _golden()
    N = d["hit_pos"].shape[0]
    first = int(torch.nonzero(d["hit_depth"] < 10)[0])
    order = torch.cat([torch.arange(N)[torch.arange(N) != first], torch.tensor([first])])
    inv = torch.empty(N, dtype=torch.long)
    inv[order] = torch.arange(N)
    lit, lit_moved = _golden_statement()[0], _golden_statement(order)[0][inv]
    own, own_moved = _golden_statement(first_row_fg=False)[0], _golden_statement(order, first_row_fg=False)[0][inv]
    assert float((lit - lit_moved).abs().max()) > 0.1
    assert torch.equal(own, own_moved)
    assert float((own - lit).abs().max()) > 0.1


# ---- Python surface without a GPU ------------------------------------------------------------------------------------------------
def _material_mesh(sc, device="cpu", encode_normals=False):
    from materialrefgs_amd.mesh import TriangleMesh
    t = sc["tables"]
    V = sc["vertices"].shape[0]
    normal = (t["normal"] + 1.0) * 0.5 if encode_normals else t["normal"]
    cols = [("rgb", torch.zeros(V, 3)), ("normal", normal), ("diffuse", t["diffuse"]), ("base_color", t["albedo"]), ("metallic", t["metallic"]),
            ("roughness", t["roughness"])]
    layout, at = {}, 0
    for name, c in cols:
        layout[name] = slice(at, at + c.shape[1])
        at += c.shape[1]
    attrs = torch.cat([c for _, c in cols], dim=1).float().contiguous().to(device)
    return TriangleMesh(sc["vertices"].to(device), sc["triangles"].to(device), attributes=attrs, layout=layout)


def test_tracer_from_a_material_ply_and_from_a_mesh(tmp_path):
    from materialrefgs_amd import io
    from materialrefgs_amd.raytracing import RayTracer
    sc = bs.scene(seed=3, n_rays=8)
    V, T = sc["vertices"].shape[0], sc["triangles"].shape[0]
    mesh = _material_mesh(sc, encode_normals=True)
    path = str(tmp_path / "material.ply")
    io.save_material_ply(path, mesh)
    for rt in (RayTracer(None, None, ply_path=path, device="cpu"), RayTracer.from_mesh(mesh, device="cpu")):
        assert rt.n_triangles == T and rt.vertices.shape == (V, 3) and rt.vertices.dtype == torch.float32
        assert rt.triangles.shape == (T, 3) and rt.triangles.dtype == torch.int32
        assert sorted(rt.vertex_attrs) == ["albedo", "diffuse", "metallic", "normal", "roughness"]
        for k, w in (("diffuse", 3), ("albedo", 3), ("normal", 3), ("metallic", 1), ("roughness", 1)):
            assert rt.vertex_attrs[k].shape == (V, w) and rt.vertex_attrs[k].dtype == torch.float32
        assert torch.equal(rt.vertices, sc["vertices"]) and torch.equal(rt.triangles, sc["triangles"])
        assert torch.allclose(rt.vertex_attrs["albedo"], sc["tables"]["albedo"]) and torch.allclose(rt.vertex_attrs["roughness"], sc["tables"]["roughness"])
        # "reference" (the default): the file's columns go through * 2 - 1 once more, as raytracer.py:245 does
        assert torch.allclose(rt.decoded_normals(), sc["tables"]["normal"], atol=1e-6)
    signed = RayTracer(None, None, ply_path=path, device="cpu", normal_encoding="signed")
    assert torch.equal(signed.decoded_normals(), signed.vertex_attrs["normal"])
    assert torch.allclose(signed.decoded_normals(), (sc["tables"]["normal"] + 1.0) * 0.5, atol=1e-6)
    with pytest.raises(ValueError, match="normal_encoding"):
        RayTracer(None, None, ply_path=path, device="cpu", normal_encoding="unit")


def test_a_tracer_without_attributes_names_what_shade_misses():
    from materialrefgs_amd.mesh import TriangleMesh
    from materialrefgs_amd.raytracing import RayTracer
    sc = bs.scene(seed=3, n_rays=8)
    rt = RayTracer(sc["vertices"], sc["triangles"], device="cpu")
    assert rt.vertex_attrs is None
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match=r"diffuse.*albedo.*normal.*metallic.*roughness"):
        rt.shade(z, z, z, None, None, None, 32, None)
    with pytest.raises(ValueError, match="vertex attributes"):
        rt.secondary_indirect_color(z, z, z, torch.zeros(4, dtype=torch.int32), torch.zeros(4), None)
    with pytest.raises(ValueError, match="base_color"):
        RayTracer.from_mesh(TriangleMesh(sc["vertices"], sc["triangles"]), device="cpu")


def test_shim_package_resolves_to_the_hip_tracer():
    import raytracing_brdf
    from materialrefgs_amd import raytracing, shading
    assert raytracing_brdf.RayTracer is raytracing.RayTracer
    assert raytracing_brdf.raytraced_indirect_light is shading.raytraced_indirect_light


# ---- C ABI without a GPU ------------------------------------------------------------------------------------------------------------
def test_bounce_prototypes_match_the_header():
    from materialrefgs_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrgs.h")).read(), flags=re.S)
    assert _lib.lib().mrgs_abi_version() == _lib.MRGS_ABI_VERSION == 10
    for name in ("mrgs_bounce_shade_forward", "mrgs_bounce_shade_backward"):
        m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m is not None, name
        assert len(_lib.SYMBOLS[name][1]) == m.group(1).count(",") + 1
    fields = re.search(r"typedef struct MrgsBounceConfig \{(.*?)\} MrgsBounceConfig;", src, flags=re.S).group(1)
    names = [n for decl in fields.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.MrgsBounceConfig._fields_]
    assert ctypes.sizeof(_lib.MrgsBounceConfig) == 4 + 4 + 3 * 8 + 2 * 4


def test_bounce_argument_checks_without_gpu():
    from materialrefgs_amd import _lib
    from materialrefgs_amd._lib import MrgsBounceConfig, MrgsEnvMips
    L = _lib.lib()
    BAD = _lib.MRGS_E_BAD_ARG
    p = ctypes.c_void_p(0x1000)          # never dereferenced: every call below is refused, or has nothing to do, before a launch
    mips = MrgsEnvMips()
    mips.n_levels, mips.res[0], mips.tex[0], mips.min_roughness, mips.max_roughness = 1, 8, 0x1000, 0.08, 0.5

    def fwd(cfg, table=p, base=p, out=p, m=mips):
        return L.mrgs_bounce_shade_forward(ctypes.byref(cfg), ctypes.byref(m), base, p, p, p, p, None, p, p, table, p, out, None)

    def bwd(cfg, table=p, g_out=p):
        return L.mrgs_bounce_shade_backward(ctypes.byref(cfg), ctypes.byref(mips), p, None, p, p, p, p, None, p, p, table, p, g_out, None, None)
    good = lambda n=4: MrgsBounceConfig(0, n, 10, 12, 8, 256)   # noqa: E731
    for call in (fwd, bwd):
        assert call(good(), table=None) == BAD                               # null table
        assert call(good(), table=ctypes.c_void_p(0x1004)) == BAD           # rows are read as three 16-byte loads
        short = good()
        short.struct_size -= 4
        assert call(short) == BAD
        assert call(good(-1)) == BAD
        assert call(MrgsBounceConfig(1, 4, 10, 12, 8, 256)) == BAD           # flags
        assert call(MrgsBounceConfig(0, 4, 0, 12, 8, 256)) == BAD            # rays, but no vertices
        assert call(MrgsBounceConfig(0, 4, 10, 12, 0, 256)) == BAD           # base_res
        assert call(good(0)) == 0                                            # nothing to launch
        assert call(good(0), table=None) == 0
    assert fwd(good(), out=None) == BAD and fwd(good(), base=None) == BAD and bwd(good(), g_out=None) == BAD
    assert fwd(good(), m=MrgsEnvMips()) == BAD                                # a chain without levels
    assert L.mrgs_bounce_shade_forward(None, ctypes.byref(mips), p, p, p, p, p, None, p, p, p, p, p, None) == BAD


# ---- the GPU cases: inputs on the host, traced by the brute-force oracle for the CPU test and by the kernel for the GPU tests -------
def _rays(name):
    """(scene, surface_pos, rays_n, rays_v) of a case."""
    if name == "n4099":
        sc = bs.scene(seed=0, n_rays=4099)
    elif name == "n1":
        sc = bs.scene(seed=1, n_rays=1)
        sc["surface_pos"][:] = torch.tensor([0.11, -0.32, 0.0])
        sc["rays_n"][:] = sc["rays_v"][:] = torch.tensor([0.0, 0.0, 1.0])
    elif name == "all_miss":
        sc = bs.scene(seed=2, n_rays=700)
        sc["surface_pos"][:, 0] += 4.3                                         # beside the sheets, near-vertical mirrors: every ray leaves
        up = torch.tensor([0.0, 0.0, 1.0])
        sc["rays_n"] = torch.nn.functional.normalize(up + 0.2 * (sc["rays_n"] - up), dim=-1)
        sc["rays_v"] = torch.nn.functional.normalize(up + 0.2 * (sc["rays_v"] - up), dim=-1)
    elif name == "all_hit":
        sc = bs.scene(seed=4, n_rays=700)
        sc["surface_pos"][:, :2] *= 0.3
        up = torch.tensor([0.0, 0.0, 1.0])
        sc["rays_n"] = torch.nn.functional.normalize(up + 0.2 * (sc["rays_n"] - up), dim=-1)
        sc["rays_v"] = torch.nn.functional.normalize(up + 0.2 * (sc["rays_v"] - up), dim=-1)
    elif name == "one_triangle":
        sc = bs.scene(seed=5, n_rays=2048)
        g = torch.Generator().manual_seed(55)
        sc["tables"]["roughness"] = 0.12 + 0.3 * torch.rand(sc["vertices"].shape[0], 1, generator=g)    # clear of the mip map's two kinks
        sc["surface_pos"][:, 0] = 0.15 + 0.05 * torch.rand(2048, generator=g)   # under the cell [0, 0.25]^2, on the side y < x
        sc["surface_pos"][:, 1] = 0.06 + 0.03 * torch.rand(2048, generator=g)
        up = torch.tensor([0.0, 0.0, 1.0])
        sc["rays_n"] = torch.nn.functional.normalize(up + 0.005 * (sc["rays_n"] - up), dim=-1)
        sc["rays_v"] = torch.nn.functional.normalize(up + 0.01 * (sc["rays_v"] - up), dim=-1)
    else:
        raise KeyError(name)
    return sc


CASES = ("n4099", "n1", "all_miss", "all_hit", "one_triangle")
BACKWARD_CASES = ("n4099", "one_triangle")          # the cases whose gradients the GPU tests compare


def _statement(sc, traced, base, spec, dtype, upstream=None, active=None, rough_range=(0.08, 0.5)):
    """Forward (and, with `upstream`, the gradients to base, every level and the four tables) of the statement in `dtype`."""
    c = lambda x: x.detach().cpu().to(dtype)   # noqa: E731
    hit_pos, view, depth, ids = traced
    base_ = c(base).requires_grad_(True)
    spec_ = [c(m).requires_grad_(True) for m in spec]
    tables = {k: c(v).requires_grad_(k != "normal") for k, v in sc["tables"].items()}
    out = bs.secondary_indirect_color(c(hit_pos), c(view), ids.cpu(), depth.cpu(), c(sc["vertices"]), sc["triangles"], tables, base_, spec_,
                                      c(_lut()), rough_range[0], rough_range[1], active=None if active is None else active.cpu())
    if upstream is None:
        return out.detach()
    grads = torch.autograd.grad((out * c(upstream)).sum(), [base_] + spec_ + [tables[k] for k in TABLE_KEYS], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, [base_] + spec_ + [tables[k] for k in TABLE_KEYS])]
    names = ["base"] + [f"spec_{i}" for i in range(len(spec_))] + list(TABLE_KEYS)
    return out.detach(), dict(zip(names, grads))


def _upstream(sc, traced, n_levels, seed=9):
    """A random upstream gradient with the rows of the ambiguous rays zeroed, and the share of those rays."""
    hit_pos, _, depth, ids = traced
    amb = bs.ambiguous(hit_pos.cpu(), ids.cpu(), depth.cpu(), sc["vertices"], sc["triangles"], sc["tables"], 256, n_levels)
    g = torch.rand(hit_pos.shape[0], 3, generator=torch.Generator().manual_seed(seed))
    g[amb] = 0.0
    return g, float(amb.float().mean())


@pytest.mark.parametrize("name", CASES)
def test_gpu_inputs_are_well_conditioned(name):
    """What the GPU tests assume of their inputs, checked where no GPU is needed: at most 1 % of a case's rays are ambiguous, both
    branches run where the case is meant to have both, and the literal float32 reading of the statement and its float32 autograd sit
    within HALF the bars of the float64 one -- so a float32 kernel has room inside them."""
    sc = _rays(name)
    inc = bs.incident(sc["rays_n"], sc["rays_v"])
    hit_pos, _, depth, ids = bs.trace_cpu(sc, sc["surface_pos"], inc)
    traced = (hit_pos, -inc, depth, ids)
    share = float((depth < 10).float().mean())
    want = {"n4099": (0.2, 0.5), "n1": (1.0, 1.0), "all_miss": (0.0, 0.0), "all_hit": (1.0, 1.0), "one_triangle": (1.0, 1.0)}[name]
    assert want[0] <= share <= want[1], share
    if name == "one_triangle":
        assert len(torch.unique(ids)) == 1
    base, spec = bs.environment(seed=0)
    up, amb_share = _upstream(sc, traced, len(spec))
    assert amb_share <= 0.01
    o64, g64 = _statement(sc, traced, base, spec, torch.float64, up)
    o32, g32 = _statement(sc, traced, base, spec, torch.float32, up)
    print(name, "forward", float((o32 - o64).abs().max()), "of", float(o64.abs().max()))
    assert float((o32 - o64).abs().max()) <= 0.5 * FWD_BAR * float(o64.abs().max())
    for k in g64:
        top = float(g64[k].abs().max())
        print(name, k, float((g32[k] - g64[k]).abs().max()), "of", top)
        if name in BACKWARD_CASES:
            assert float((g32[k] - g64[k]).abs().max()) <= 0.5 * GRAD_BAR * top, k


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
class _Env:
    """What secondary_indirect_color reads of an EnvLight, around given tensors (each a leaf, so that every level's gradient shows)."""

    def __init__(self, base, spec, device):
        self.min_roughness, self.max_roughness = 0.08, 0.5
        self.base = base.to(device).requires_grad_(True)
        self.specular = [m.to(device).requires_grad_(True) for m in spec]


def _tracer(sc, device, encoding="signed"):
    from materialrefgs_amd.raytracing import RayTracer
    return RayTracer.from_mesh(_material_mesh(sc, device, encode_normals=encoding == "reference"), device=device, normal_encoding=encoding)


def _traced(rt, sc, device):
    inc = bs.incident(sc["rays_n"].to(device), sc["rays_v"].to(device))                   # on the device, as shade evaluates it
    hit_pos, nrm, depth, ids = rt.trace(sc["surface_pos"].to(device), inc, return_faceids=True)
    return (hit_pos, -inc, depth, ids), nrm


def _close(got, want, bar):
    got, want = got.detach().cpu().double(), want.double()
    assert torch.isfinite(got).all()
    err, top = float((got - want).abs().max()), float(want.abs().max())
    assert err <= bar * top, (err, top)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n4099", "n1", "all_miss", "all_hit"])
def test_secondary_indirect_color_matches_the_statement(gpu_device, name):
    sc = _rays(name)
    rt = _tracer(sc, gpu_device)
    traced, nrm = _traced(rt, sc, gpu_device)
    depth = traced[2]
    if name == "all_miss":
        assert bool((depth >= 10).all())
    if name in ("all_hit", "n1"):
        assert bool((depth < 10).all())
    if name == "n4099":
        assert 0.2 < float((depth < 10).float().mean()) < 0.5
    base, spec = bs.environment(seed=0)
    env = _Env(base, spec, gpu_device)
    out = rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], depth, env)
    again = rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], depth, env)
    assert out.shape == (sc["surface_pos"].shape[0], 3) and torch.equal(out, again)          # the forward is deterministic
    _close(out, _statement(sc, traced, base, spec, torch.float64), FWD_BAR)


@pytest.mark.gpu
def test_inactive_rays_write_zero_and_receive_no_gradient(gpu_device):
    sc = _rays("n4099")
    rt = _tracer(sc, gpu_device)
    traced, nrm = _traced(rt, sc, gpu_device)
    base, spec = bs.environment(seed=0)
    env = _Env(base, spec, gpu_device)
    N = sc["surface_pos"].shape[0]
    active = torch.arange(N, device=gpu_device) % 2 == 0
    out = rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], traced[2], env, active=active)
    as_bytes = rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], traced[2], env, active=active.to(torch.uint8))
    assert torch.equal(out, as_bytes)
    assert float(out.detach()[~active].abs().max()) == 0.0 and float(out.detach()[active].abs().max()) > 0
    _close(out, _statement(sc, traced, base, spec, torch.float64, active=active), FWD_BAR)
    up = torch.rand(N, 3, generator=torch.Generator().manual_seed(3))
    _, want = _statement(sc, traced, base, spec, torch.float64, up * active.cpu().unsqueeze(-1))
    out.backward(up.to(gpu_device))                                                       # the inactive rows carry a gradient that must not arrive
    _close(env.base.grad, want["base"], GRAD_BAR)                                         # (texel gradients of the base fetch have no kinks)
    assert float(env.specular[0].grad.abs().max()) > 0


@pytest.mark.gpu
def test_default_four_level_environment_through_build_mips(gpu_device):
    """EnvLight as it ships (128 -> 16, four prefiltered levels): forward against the statement on the chain build_mips made, and the
    gradient reaches env.base through the prefilter's own node."""
    from materialrefgs_amd.shading import EnvLight
    sc = _rays("n4099")
    rt = _tracer(sc, gpu_device, encoding="reference")
    traced, nrm = _traced(rt, sc, gpu_device)
    env = EnvLight(device=gpu_device, trainable=True)
    with torch.no_grad():
        env.base.copy_(torch.randn(env.base.shape, generator=torch.Generator().manual_seed(8)).to(gpu_device))
    env.build_mips()
    assert [m.shape[1] for m in env.specular] == [128, 64, 32, 16]
    out = rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], traced[2], env)
    sc64 = dict(sc, tables=dict(sc["tables"], normal=rt.decoded_normals().cpu()))        # the table as decoded from its encoded columns
    _close(out, _statement(sc64, traced, env.base, env.specular, torch.float64), FWD_BAR)
    out.sum().backward()
    assert env.base.grad is not None and bool(torch.isfinite(env.base.grad).all()) and float(env.base.grad.abs().max()) > 0


@pytest.mark.gpu
def test_shade_is_the_trace_then_the_bounce_and_the_gather_matches(gpu_device):
    sc = _rays("n4099")
    rt = _tracer(sc, gpu_device)
    traced, nrm = _traced(rt, sc, gpu_device)
    base, spec = bs.environment(seed=0)
    env = _Env(base, spec, gpu_device)
    dev = lambda k: sc[k].to(gpu_device)   # noqa: E731
    shaded = rt.shade(dev("surface_pos"), dev("rays_n"), dev("rays_v"), None, None, None, 32, env)
    assert torch.equal(shaded, rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], traced[2], env))
    hit = traced[2] < 10
    got = rt.get_materials_by_faceids(traced[0][hit], traced[3][hit])
    want, _, _ = bs.gather(traced[0][hit].cpu().double(), traced[3][hit].cpu(), sc["vertices"].double(), sc["triangles"], bs.to64(sc["tables"]))
    for g, k in zip(got, ("diffuse", "metallic", "roughness", "albedo", "normal")):
        assert g.shape == want[k].shape
        _close(g, want[k], FWD_BAR)


@pytest.mark.gpu
def test_a_triangle_of_projected_area_zero_writes_zero(gpu_device):
    """One vertical wall in the mesh: a ray onto it has area(a, b, c) = 0 in the xy-projection, NaN in the reference (which its caller
    turns into 0); here the ray writes exactly 0 and gets no gradient, and nothing else turns NaN."""
    sc = bs.scene(seed=0, n_rays=300, wall=True)
    sc["surface_pos"][:40] = torch.tensor([0.0, 0.1, 0.0]) + 0.2 * (torch.rand(40, 3, generator=torch.Generator().manual_seed(2)) - 0.5)
    sc["rays_n"][:40] = sc["rays_v"][:40] = torch.tensor([1.0, 0.0, 0.0])
    rt = _tracer(sc, gpu_device)
    traced, nrm = _traced(rt, sc, gpu_device)
    wall = traced[3][:40].cpu()
    T = sc["triangles"].shape[0]
    assert bool(((wall == T - 1) | (wall == T - 2)).all())
    base, spec = bs.environment(seed=0)
    env = _Env(base, spec, gpu_device)
    for k in TABLE_KEYS:
        rt.vertex_attrs[k].requires_grad_(True)
    out = rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], traced[2], env)
    assert bool(torch.isfinite(out).all()) and float(out.detach()[:40].abs().max()) == 0.0 and float(out.detach()[40:].abs().max()) > 0
    _close(out, _statement(sc, traced, base, spec, torch.float64), FWD_BAR)
    out.sum().backward()
    for g in [env.base.grad] + [m.grad for m in env.specular] + [rt.vertex_attrs[k].grad for k in TABLE_KEYS]:
        assert bool(torch.isfinite(g).all())
    assert float(rt.vertex_attrs["diffuse"].grad[-4:].abs().max()) == 0.0                 # the wall's four vertices


@pytest.mark.gpu
@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_backward_matches_the_float64_autograd(gpu_device, name):
    """Gradients to the base level, every level of the chain and the four tables; the upstream gradient is random with the ambiguous
    rays' rows zeroed in both legs.  `one_triangle`: 2 048 rays whose 24 atomics each land on the same three table rows."""
    sc = _rays(name)
    rt = _tracer(sc, gpu_device)
    traced, nrm = _traced(rt, sc, gpu_device)
    if name == "one_triangle":
        assert len(torch.unique(traced[3])) == 1 and bool((traced[2] < 10).all())
    base, spec = bs.environment(seed=0)
    env = _Env(base, spec, gpu_device)
    for k in TABLE_KEYS:
        rt.vertex_attrs[k].requires_grad_(True)
    up, amb_share = _upstream(sc, traced, len(spec))
    assert amb_share <= 0.01
    out = rt.secondary_indirect_color(traced[0], traced[1], nrm, traced[3], traced[2], env)
    out.backward(up.to(gpu_device))
    _, want = _statement(sc, traced, base, spec, torch.float64, up)
    got = {"base": env.base.grad, **{f"spec_{i}": m.grad for i, m in enumerate(env.specular)}, **{k: rt.vertex_attrs[k].grad for k in TABLE_KEYS}}
    for k in want:
        err, top = float((got[k].cpu().double() - want[k]).abs().max()), float(want[k].abs().max())
        print(name, k, err, "of", top)
    for k in want:
        if float(want[k].abs().max()) == 0.0:                                             # (no miss ray: nothing reaches the base level)
            assert float(got[k].abs().max()) == 0.0, k
        else:
            _close(got[k], want[k], GRAD_BAR)


def _camera():
    """A camera inside the box at z = 0.6 looking down at the floor, tilted by 0.2 rad: (HWK, Camera.R, Camera.T)."""
    H, W = 40, 52
    K = np.array([[40.0, 0.0, 26.0], [0.0, 40.0, 20.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    c, s = np.cos(0.2), np.sin(0.2)
    c2w = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float32) @ np.diag([1.0, -1.0, -1.0]).astype(np.float32)
    T = -c2w.T @ np.array([0.05, -0.1, 0.6], dtype=np.float32)
    return (H, W, K), torch.from_numpy(c2w), torch.from_numpy(T.astype(np.float32))


@pytest.mark.gpu
def test_raytraced_indirect_light_against_the_reference_composition(gpu_device):
    """utils/refl_utils.py:118-147 written as the reference writes it -- boolean masks, compaction, a zero-filled map -- with the
    statement in place of shade's second half, against the one-call form that hands the masks to the kernel."""
    from types import SimpleNamespace
    from materialrefgs_amd import shading
    from materialrefgs_amd.gs_utils import safe_normalize
    dev = gpu_device
    sc = bs.scene(seed=6, n_rays=8)
    rt = _tracer(sc, dev)
    HWK, R, T = _camera()
    H, W, K = HWK
    R, T = R.to(dev), T.to(dev)
    g = torch.Generator().manual_seed(12)
    up = torch.tensor([0.0, 0.0, 1.0])
    normal_map = torch.nn.functional.normalize(up + 0.3 * torch.randn(H, W, 3, generator=g), dim=-1).to(dev)
    prior = torch.nn.functional.normalize(up + 0.3 * torch.randn(H, W, 3, generator=g), dim=-1).to(dev)
    alpha = torch.rand(H, W, 1, generator=g)
    alpha[:5] = 0.0
    alpha = alpha.to(dev)
    base, spec = bs.environment(seed=0)
    env = _Env(base, spec, dev)
    pc = SimpleNamespace(ray_tracer=rt)
    got = shading.raytraced_indirect_light(env, HWK, R, T, normal_map, prior, alpha, pc)
    assert got["visibility"].shape == (1, H, W) and got["indirect_light_raytracing"].shape == (3, H, W)

    # the reference's composition, on the same device so that the rays are the same bits
    Rw = R.T
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    pixel_camera = torch.tensor(np.dot(np.stack([i, j, np.ones_like(i)], axis=2), np.linalg.inv(K).T).astype(np.float32)).to(dev)
    rays_o = (-Rw.T @ T.unsqueeze(-1)).flatten()
    rays_cam = ((pixel_camera - T[None, None]).reshape(-1, 3) @ Rw - rays_o[None]).reshape(H, W, 3)
    mask = (alpha > 0)[..., 0]
    w_o = safe_normalize(-rays_cam)
    rays_refl = safe_normalize(2 * normal_map * torch.sum(w_o * normal_map, dim=-1, keepdim=True) - w_o)
    surf, _, _, _ = rt.trace(rays_o[None, None].expand_as(rays_cam).reshape(-1, 3), safe_normalize(rays_cam).reshape(-1, 3), return_faceids=True)
    _, _, depth, _ = rt.trace(surf.reshape(H, W, 3)[mask], rays_refl[mask], return_faceids=True)
    visibility = torch.ones_like(alpha)
    visibility[mask] = (depth >= 10.0).float().unsqueeze(-1)
    mc_mask = mask.clone()
    mc_mask[mask] = depth < 10.0
    assert 0.1 < float(mc_mask.float().mean()) < 0.9 and float(visibility.mean()) < 1.0
    pts, nrm, wo = surf.reshape(H, W, 3)[mc_mask], prior[mc_mask], w_o[mc_mask]
    inc = bs.incident(nrm, wo)
    hit_pos, _, hit_depth, ids = rt.trace(pts, inc, return_faceids=True)
    light = torch.zeros(H, W, 3, dtype=torch.float64)
    light[mc_mask.cpu()] = _statement(sc, (hit_pos, -inc, hit_depth, ids), base, spec, torch.float64)
    assert torch.equal(got["visibility"], visibility.permute(2, 0, 1))
    _close(got["indirect_light_raytracing"], light.permute(2, 0, 1), FWD_BAR)
    assert float(got["indirect_light_raytracing"].detach().permute(1, 2, 0)[~mc_mask].abs().max()) == 0.0


@pytest.mark.gpu
def test_no_host_read(gpu_device):
    """shade and raytraced_indirect_light make no synchronising call once the library is loaded and the per-camera constant is cached
    (the way test_ref_score.py::test_no_host_read checks)."""
    from types import SimpleNamespace
    from materialrefgs_amd import shading
    dev = gpu_device
    sc = _rays("n4099")
    rt = _tracer(sc, dev)
    base, spec = bs.environment(seed=0)
    env = _Env(base, spec, dev)
    pos, n, v = sc["surface_pos"].to(dev), sc["rays_n"].to(dev), sc["rays_v"].to(dev)
    active = torch.arange(pos.shape[0], device=dev) % 3 != 0
    HWK, R, T = _camera()
    R, T = R.to(dev), T.to(dev)
    H, W, _ = HWK
    nm = torch.nn.functional.normalize(torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1)) + torch.tensor([0.0, 0.0, 1.0]), dim=-1).to(dev)
    alpha = torch.ones(H, W, 1, device=dev)
    pc = SimpleNamespace(ray_tracer=rt)
    first = rt.shade(pos, n, v, None, None, None, 32, env, active=active)
    first_map = shading.raytraced_indirect_light(env, HWK, R, T, nm, nm, alpha, pc)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = rt.shade(pos, n, v, None, None, None, 32, env, active=active)
        again.backward(torch.ones_like(again))
        again_map = shading.raytraced_indirect_light(env, HWK, R, T, nm, nm, alpha, pc)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(first, again) and torch.equal(first_map["indirect_light_raytracing"], again_map["indirect_light_raytracing"])
    assert env.base.grad is not None
