"""The per-gaussian stage of `render_volume` (opt.indirect off) stated with float64 torch ops -- TEST INFRASTRUCTURE ONLY.

gaussian_renderer/__init__.py:559-661, utils/refl_utils.py:426-445 and scene/light.py:99-129, from the raw GaussianModel tensors to
what the rasterizer is handed:

    opacity = sigmoid, scales = exp, rotations = normalize                                  (the getters)
    n         = safe_normalize(third column of R(q) * flip), flip from the unit direction camera_center -> xyz (constant for autograd)
    w_o       = safe_normalize(rays_o - xyz)          rays_o: the origin of sample_camera_rays, the reference's other camera position
    NdotV     = w_o . n,   rays_refl = safe_normalize(2 n NdotV - w_o)
    diffuse   = sigmoid(fetch(diffuse map, n)) (1 - refl) ori_color
    direct    = sigmoid(trilinear fetch(specular chain, rays_refl, get_mip(roughness)))
    specular  = direct ((0.04 (1 - refl) + ori_color refl) fg0.x + fg0.y),  fg0 = FG LUT at (NdotV, roughness).clamp(0, 1) OF ROW 0
    colors_precomp = specular + diffuse,  features = (roughness, refl, diffuse, specular, ori_color [, |n_cam . centre_cam|])

The lookups are oracle.shading_oracle's (pinned).  `decision_margin` is the distance of every row to the nearest decision the float32
forms could take the other way.  `torch_chain` is the product's own chain of torch ops for the same stage (what render_volume runs with
renderer._NATIVE_VOLUME off), the second leg of the comparison rule.
"""
import torch

from oracle import shading_oracle as so

RAW_NAMES = ("xyz", "scaling", "rotation", "opacity", "refl_strength", "roughness", "ori_color")


def _geometry(xyz, rotation, campos, rays_o):
    q = rotation / torch.sqrt((rotation * rotation).sum(dim=1, keepdim=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    nr = torch.stack((2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)), dim=-1)
    d = xyz - campos
    v = d / d.norm(dim=1, keepdim=True)
    facing = (nr * -v).sum(dim=-1, keepdim=True)
    nf = nr * torch.where(facing >= 0, 1.0, -1.0).to(nr.dtype)
    n = nf / torch.clamp(torch.linalg.norm(nf, dim=-1, keepdim=True), min=1e-20)
    wo = rays_o - xyz
    wo = wo / torch.clamp(torch.linalg.norm(wo, dim=-1, keepdim=True), min=1e-20)
    ndotv = (wo * n).sum(dim=-1, keepdim=True)
    rr = 2 * n * ndotv - wo
    rr = rr / torch.clamp(torch.linalg.norm(rr, dim=-1, keepdim=True), min=1e-20)
    return n, ndotv, rr, facing


def volume_statement(raw, campos, rays_o, lut, specular, diffuse_tex, viewmatrix=None, min_roughness=0.08, max_roughness=0.5):
    """raw: the seven tensors in RAW_NAMES order (any float dtype, the statement runs in theirs); specular: list of [6,r,r,3] levels;
    diffuse_tex [6,r,r,3]; viewmatrix: world_view_transform as stored ("pgsr") or None.
    Returns (opacity[P,1], scales[P,2], rotations[P,4], colors_precomp[P,3], features[P,11 | 12])."""
    xyz, scaling, rotation, opacity_raw, refl_raw, rough_raw, ori_raw = raw
    opacity, scales = torch.sigmoid(opacity_raw), torch.exp(scaling)
    rotations = rotation / torch.clamp(torch.linalg.norm(rotation, dim=1, keepdim=True), min=1e-12)
    refl, rough, oc = torch.sigmoid(refl_raw), torch.sigmoid(rough_raw), torch.sigmoid(ori_raw)
    n, ndotv, rr, _ = _geometry(xyz, rotation, campos, rays_o)
    fg0 = so.lut_fetch(lut, torch.cat([ndotv, rough], -1).clamp(0, 1)[:1])[0]              # the reference's fg[0]
    diffuse = so.env_lookup([diffuse_tex], n) * (1 - refl) * oc
    direct = so.env_lookup(list(specular), rr, rough.reshape(-1), min_roughness, max_roughness)
    spec = direct * ((0.04 * (1 - refl) + oc * refl) * fg0[0:1] + fg0[1:2])
    feats = [rough, refl, diffuse, spec, oc]
    if viewmatrix is not None:
        normal_cam = n @ viewmatrix[:3, :3]
        centre_cam = xyz @ viewmatrix[:3, :3] + viewmatrix[3, :3]
        feats.append((normal_cam * centre_cam).sum(-1).abs().unsqueeze(-1))
    return opacity, scales, rotations, spec + diffuse, torch.cat(feats, dim=-1)


def _grid_distance(f):
    """distance of a continuous texel coordinate to the nearest integer: where the bilinear cell changes"""
    return (f - torch.round(f)).abs()


def decision_margin(raw, campos, rays_o, lut, specular, diffuse_tex, min_roughness=0.08, max_roughness=0.5, parts=False):
    """Per row the minimum of |n . dir|, |roughness - min_roughness|, |roughness - max_roughness|, the distance of each lookup's tap
    coordinates to a texel boundary at the levels it uses and, for row 0, of its LUT coordinates to a cell boundary.
    parts=True: the dictionary of the parts instead."""
    with torch.no_grad():
        xyz, _, rotation, _, _, rough_raw, _ = [t.detach().double() for t in raw]
        rough = torch.sigmoid(rough_raw).reshape(-1)
        n, ndotv, rr, facing = _geometry(xyz, rotation, campos.double(), rays_o.double())
        out = {"flip": facing.reshape(-1).abs(),
               "roughness": torch.minimum((rough - min_roughness).abs(), (rough - max_roughness).abs())}
        _, _, fx, fy, _ = so.bilinear_taps(diffuse_tex.shape[1], n)
        out["diffuse_taps"] = torch.minimum(_grid_distance(fx), _grid_distance(fy))
        nl = len(specular)
        lc = torch.clamp(so.get_mip(rough, nl, min_roughness, max_roughness), 0, nl - 1)
        l0 = torch.clamp(torch.floor(lc).long(), max=nl - 1)
        l1 = torch.clamp(l0 + 1, max=nl - 1)
        taps = torch.full_like(rough, float("inf"))
        for i, m in enumerate(specular):
            _, _, fx, fy, _ = so.bilinear_taps(m.shape[1], rr)
            dist = torch.minimum(_grid_distance(fx), _grid_distance(fy))
            used = (l0 == i) | (l1 == i)
            taps = torch.where(used, torch.minimum(taps, dist), taps)
        out["specular_taps"] = taps
        uv0 = torch.cat([ndotv, rough.unsqueeze(-1)], -1).clamp(0, 1)[0] * lut.shape[0] - 0.5
        row0 = torch.full_like(rough, float("inf"))
        row0[0] = _grid_distance(uv0).min()
        out["lut_row0"] = row0
        if parts:
            return out
        return torch.stack(list(out.values()), 0).min(dim=0).values


def torch_chain(pc, cam, flag="2dgs", dead_sh=False):
    """The product's chain of torch ops for the stage: the lines of renderer.render_volume with the native path off, without the rasterizer.
    dead_sh: with the SH evaluation along the mirror direction whose result that branch does not use (what a timing of the chain has to
    include; it changes no value).  Device tensors; fp32."""
    from materialrefgs_amd.gs_utils import eval_sh
    from materialrefgs_amd.renderer import get_distance
    from materialrefgs_amd.shading import get_full_color_volume
    means3D, opacity = pc.get_xyz, pc.get_opacity
    refl, ori_color, roughness = pc.get_refl, pc.get_ori_color, pc.get_rough
    scales, rotations = pc.get_scaling, pc.get_rotation
    dir_pp = means3D - cam.camera_center
    dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
    normals = pc.get_normal(1.0, dir_pp_normalized)
    if dead_sh:
        w_o = -dir_pp_normalized
        reflection = 2 * torch.sum(normals * w_o, dim=1, keepdim=True) * normals - w_o
        shs_indirect = pc.get_indirect.transpose(1, 2).reshape(-1, 3, (pc.max_sh_degree + 1) ** 2)
        torch.clamp_min(eval_sh(3, shs_indirect, reflection), 0.0)
    diffuse, specular = get_full_color_volume(pc.get_envmap_2, means3D, ori_color, cam.HWK, cam.R, cam.T, normals.contiguous(), opacity,
                                              refl_strength=refl, roughness=roughness)
    features = torch.cat((roughness, refl, diffuse, specular, ori_color), dim=-1)
    colors_precomp = specular + diffuse
    if flag != "2dgs":
        features = torch.cat((features, get_distance(1.0, means3D, cam, pc)), dim=-1)
    return opacity, scales, rotations, colors_precomp, features
