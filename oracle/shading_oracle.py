"""Plain-PyTorch fp32 CPU restatement of the shading half of the hot path -- TEST INFRASTRUCTURE ONLY.

Restates, with torch.autograd supplying the reference gradients:
  * EnvLight.get_mip / EnvLight.__call__            (scene/light.py:88-129)
  * sample_camera_rays, reflection, get_specular_color_surfel without visibility tracing
                                                     (utils/refl_utils.py:54-73,95-98,364-419)
The texture lookups: the reference performs them with nvdiffrast's `dr.texture`, which is not vendored
(requirements.txt:57 pins a local path) and cannot be imported here, and the reference has no test for this path.  The
sampling rules are therefore restated from nvdiffrast's documented behaviour (texel centres at (i+0.5)/res, bilinear,
`clamp` boundary for the 2D LUT, seamless cube edges, trilinear between integer mip levels at LOD = mip_level_bias); the
cube face/orientation convention is pinned in-tree by cube_to_dir (scene/light_utils.py:24-31).  tests/test_envmap_seams.py holds this
restatement to the geometry of a cube, in float64 and with no second restatement in between.  PINNED BY GEOMETRY: the face
orientation (texel centres on all six faces), all 12 seams and all 8 vertices (continuity), the weight sums, the level shares, the
tangency of the direction gradient and that it is the slope of the forward inside a cell.  STILL A RESTATEMENT of nvdiffrast: the
drop-and-renormalise rule of a vertex cell and its gradient, which holds the renormalisation constant.  The kernels' statement of the
same rules is csrc/mrgs_envmap.h, which the lookups and the shading (mrgs_shade.hip) and the one-bounce light (mrgs_bounce.hip) share;
csrc/mrgs_volume.hip restates the taps once more for fp64 coordinates.
Everything else (ray set-up, mirror direction, Fresnel-style weight, compositing) is elementwise arithmetic restated literally.
"""
import numpy as np
import torch

EPS_EDGE = 1.0 / 4096.0


def cube_to_dir(s, x, y):
    """scene/light_utils.py:24-31."""
    one = torch.ones_like(x)
    if s == 0: return torch.stack((one, -y, -x), -1)
    if s == 1: return torch.stack((-one, -y, x), -1)
    if s == 2: return torch.stack((x, one, y), -1)
    if s == 3: return torch.stack((x, -one, -y), -1)
    if s == 4: return torch.stack((x, -y, one), -1)
    return torch.stack((-x, -y, -one), -1)


def dir_to_face_uv(d):
    """Inverse of cube_to_dir: direction [N,3] -> face [N] (long), u, v in [-1,1] (differentiable w.r.t. d)."""
    ax, ay, az = d[:, 0].abs(), d[:, 1].abs(), d[:, 2].abs()
    is_x = (ax >= ay) & (ax >= az)
    is_y = (~is_x) & (ay >= az)
    is_z = ~(is_x | is_y)
    pos = torch.where(is_x, d[:, 0] >= 0, torch.where(is_y, d[:, 1] >= 0, d[:, 2] >= 0))
    face = torch.where(is_x, 0, torch.where(is_y, 2, 4)) + (~pos).long()
    ma = torch.where(is_x, ax, torch.where(is_y, ay, az))
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    sgn = torch.where(pos, 1.0, -1.0)
    u = torch.where(is_x, -sgn * z, torch.where(is_y, x, sgn * x)) / ma
    v = torch.where(is_x, -y, torch.where(is_y, sgn * z, -y)) / ma
    return face, u, v


def _wrap(face, x, y, res):
    """Integer tap (face, x, y) possibly off the face -> linear texel index on the face across the edge."""
    inb = (x >= 0) & (x < res) & (y >= 0) & (y < res)
    u = (x.float() + 0.5) / res * 2 - 1
    v = (y.float() + 0.5) / res * 2 - 1
    u = torch.where(x < 0, torch.full_like(u, -1 - EPS_EDGE), torch.where(x >= res, torch.full_like(u, 1 + EPS_EDGE), u))
    v = torch.where(y < 0, torch.full_like(v, -1 - EPS_EDGE), torch.where(y >= res, torch.full_like(v, 1 + EPS_EDGE), v))
    d = torch.zeros(u.shape[0], 3, device=u.device)
    for s in range(6):
        m = face == s
        if m.any():
            d[m] = cube_to_dir(s, u[m], v[m])
    f2, u2, v2 = dir_to_face_uv(d)
    xi = torch.clamp(torch.floor((u2 * 0.5 + 0.5) * res).long(), 0, res - 1)
    yi = torch.clamp(torch.floor((v2 * 0.5 + 0.5) * res).long(), 0, res - 1)
    wrapped = (f2 * res + yi) * res + xi
    direct = (face * res + y.clamp(0, res - 1)) * res + x.clamp(0, res - 1)
    return torch.where(inb, direct, wrapped)


def bilinear_taps(res, dirs):
    """The four taps of a seamless bilinear fetch of a res^2 cubemap at directions [N,3]: (idx, w, fx, fy, face) with idx / w lists of
    four [N] tensors (linear texel index (face res + y) res + x across the edge where a tap leaves the face; weights with the cube corner's
    tap dropped and the rest renormalised), fx / fy the continuous texel coordinates on the face the direction selects."""
    face, u, v = dir_to_face_uv(dirs)
    fx = (u * 0.5 + 0.5) * res - 0.5
    fy = (v * 0.5 + 0.5) * res - 0.5
    x0f, y0f = torch.floor(fx).detach(), torch.floor(fy).detach()
    wx, wy = fx - x0f, fy - y0f
    x0, y0 = x0f.long(), y0f.long()
    w = [(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy]
    offs = [(0, 0), (1, 0), (0, 1), (1, 1)]
    ox = [x0 < 0, x0 + 1 >= res, x0 < 0, x0 + 1 >= res]
    oy = [y0 < 0, y0 < 0, y0 + 1 >= res, y0 + 1 >= res]
    corner = [ox[k] & oy[k] for k in range(4)]
    w = [torch.where(corner[k], torch.zeros_like(w[k]), w[k]) for k in range(4)]
    any_corner = corner[0] | corner[1] | corner[2] | corner[3]
    norm = torch.where(any_corner, 1.0 / (w[0] + w[1] + w[2] + w[3]).detach(), torch.ones_like(wx))   # renormalisation held constant
    idx = []
    for k in range(4):
        i = _wrap(face, x0 + offs[k][0], y0 + offs[k][1], res)
        idx.append(torch.where(corner[k], torch.zeros_like(i), i))
    return idx, [w[k] * norm for k in range(4)], fx, fy, face


def cube_fetch(tex, dirs):
    """Seamless bilinear fetch of a [6,res,res,C] cubemap at directions [N,3] -> [N,C]."""
    idx, w, _, _, _ = bilinear_taps(tex.shape[1], dirs)
    flat = tex.reshape(-1, tex.shape[-1])
    out = 0
    for k in range(4):
        out = out + w[k].unsqueeze(-1) * flat[idx[k]]
    return out


def get_mip(roughness, n_levels, min_roughness=0.08, max_roughness=0.5):
    """scene/light.py:88-96 (n_levels = len(self.specular))."""
    return torch.where(
        roughness < max_roughness,
        (torch.clamp(roughness, min_roughness, max_roughness) - min_roughness) / (max_roughness - min_roughness) * (n_levels - 2),
        (torch.clamp(roughness, max_roughness, 1.0) - max_roughness) / (1.0 - max_roughness) + n_levels - 2)


def env_lookup(mips, dirs, roughness=None, min_roughness=0.08, max_roughness=0.5):
    """EnvLight.__call__ (scene/light.py:99-129): mips = list of [6,res,res,3] (pre-sigmoid), dirs [N,3], roughness [N] or None."""
    if roughness is None:
        return torch.sigmoid(cube_fetch(mips[0], dirs))
    n = len(mips)
    level = get_mip(roughness, n, min_roughness, max_roughness)
    lc = torch.clamp(level, 0, n - 1)
    l0 = torch.clamp(torch.floor(lc).detach().long(), max=n - 1)
    l1 = torch.clamp(l0 + 1, max=n - 1)
    f = lc - l0.float()
    samples = torch.stack([cube_fetch(m, dirs) for m in mips], 0)   # [n,N,3]
    ar = torch.arange(dirs.shape[0], device=dirs.device)
    val = (1 - f).unsqueeze(-1) * samples[l0, ar] + f.unsqueeze(-1) * samples[l1, ar]
    return torch.sigmoid(val)


def lut_fetch(lut, uv):
    """dr.texture(FG_LUT, uv, filter_mode='linear', boundary_mode='clamp'): lut [R,R,2], uv [N,2] in [0,1] (u -> width)."""
    R = lut.shape[0]
    fx, fy = uv[:, 0] * R - 0.5, uv[:, 1] * R - 0.5
    x0f, y0f = torch.floor(fx).detach(), torch.floor(fy).detach()
    wx, wy = (fx - x0f).unsqueeze(-1), (fy - y0f).unsqueeze(-1)
    x0, x1 = x0f.long().clamp(0, R - 1), (x0f.long() + 1).clamp(0, R - 1)
    y0, y1 = y0f.long().clamp(0, R - 1), (y0f.long() + 1).clamp(0, R - 1)
    return (1 - wy) * ((1 - wx) * lut[y0, x0] + wx * lut[y0, x1]) + wy * ((1 - wx) * lut[y1, x0] + wx * lut[y1, x1])


def sample_camera_rays(H, W, K, R, T, dtype=torch.float32):
    """utils/refl_utils.py:54-73 (R is Camera.R, stored transposed; pixel centres at integer coordinates).  The reference sets the rays
    up in float32 whatever follows, and so does this by default.  dtype=torch.float64: the same expressions in float64 on the same
    float32 K, R, T -- for a caller that wants the float64 reading of the WHOLE chain: `pixel_world - rays_o` cancels a camera distance,
    so float32 rays sit a few ulp from the exact ones, which a fetch of a fine level magnifies by res / 2."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    R = R.T
    if dtype == torch.float64:
        R, T = R.double(), T.double()
    i, j = np.meshgrid(np.arange(W, dtype=np_dt), np.arange(H, dtype=np_dt), indexing="xy")
    xy1 = np.stack([i, j, np.ones_like(i)], axis=2)
    pixel_camera = torch.tensor(np.dot(xy1, np.linalg.inv(K.astype(np.float32).astype(np_dt)).T))
    rays_o = (-R.T @ T.unsqueeze(-1)).flatten()
    pixel_world = (pixel_camera - T[None, None]).reshape(-1, 3) @ R
    rays_d = pixel_world - rays_o[None]
    rays_d = rays_d / torch.norm(rays_d, dim=1, keepdim=True)
    return rays_d.reshape(H, W, 3), rays_o


def specular_color_surfel(mips, lut, albedo, H, W, K, R, T, normal_map, render_alpha, refl_strength, roughness,
                          min_roughness=0.08, max_roughness=0.5, rays_dtype=torch.float32):
    """get_specular_color_surfel (utils/refl_utils.py:364-419) with pc.ray_tracer = None.
    albedo/normal_map [H,W,3], render_alpha/refl_strength/roughness [H,W,1] -> specular [3,H,W], direct_light [3,H,W],
    specular_weight [H,W,3].  rays_dtype: see sample_camera_rays."""
    rays_cam, _ = sample_camera_rays(H, W, K, R.cpu(), T.cpu(), rays_dtype)
    w_o = -rays_cam.to(normal_map.device)
    NdotV = torch.sum(w_o * normal_map, dim=-1, keepdim=True)
    rays_refl = 2 * normal_map * NdotV - w_o
    rays_refl = rays_refl / torch.clamp(torch.linalg.norm(rays_refl, dim=-1, keepdim=True), min=1e-20)
    fg_uv = torch.cat([NdotV, roughness], -1).clamp(0, 1)
    fg = lut_fetch(lut, fg_uv.reshape(-1, 2)).reshape(H, W, 2)
    direct_light = env_lookup(mips, rays_refl.reshape(-1, 3), roughness.reshape(-1), min_roughness, max_roughness).reshape(H, W, 3)
    specular_weight = (0.04 * (1 - refl_strength) + albedo * refl_strength) * fg[..., 0:1] + fg[..., 1:2]
    specular = direct_light * render_alpha * specular_weight
    return specular.permute(2, 0, 1), direct_light.permute(2, 0, 1), specular_weight


def mirror_dirs(H, W, K, R, T, normal_map, rays_dtype=torch.float32):
    """The normalised mirror directions [H*W,3] and NdotV [H*W] of specular_color_surfel (same arithmetic)."""
    rays_cam, _ = sample_camera_rays(H, W, K, R.cpu(), T.cpu(), rays_dtype)
    w_o = -rays_cam.to(normal_map.device)
    NdotV = torch.sum(w_o * normal_map, dim=-1, keepdim=True)
    rays_refl = 2 * normal_map * NdotV - w_o
    rays_refl = rays_refl / torch.clamp(torch.linalg.norm(rays_refl, dim=-1, keepdim=True), min=1e-20)
    return rays_refl.reshape(-1, 3), NdotV.reshape(-1)


def shade_taps(mip_res, H, W, K, R, T, normal_map, roughness, min_roughness=0.08, max_roughness=0.5, rays_dtype=torch.float32):
    """Where every pixel of specular_color_surfel fetches (no gradients): the cubemap taps and the quantities at which its per-pixel
    gradient is discontinuous.  mip_res: resolutions of the levels, finest first.  Returns dict:
      keys [N,8] int64: level << 24 | texel of the two levels' four taps, -1 where the tap's weight (level share x bilinear) is 0 --
                        the key layout of the fused backward's hash table (csrc/mrgs_shade.hip, env_scatter_tile);
      cell_edge [N] float64: distance of the nearest fx / fy (of a level with a share) to an integer, over the level's resolution
                        (fp32 rounds a texel coordinate in proportion to its size);
      level_edge [N]:   distance of the un-clamped mip level to an integer (inf where the level is clamped);
      face_gap [N]:     (|major| - |second|) / |major| of the mirror direction (the face decision);
      ndv [N], lut_uv [N,2], level [N]."""
    with torch.no_grad():
        dirs, ndv = mirror_dirs(H, W, K, R, T, normal_map, rays_dtype)
        rough = roughness.reshape(-1)
        n = len(mip_res)
        level = get_mip(rough, n, min_roughness, max_roughness)
        lc = torch.clamp(level, 0, n - 1)
        l0 = torch.clamp(torch.floor(lc).long(), max=n - 1)
        l1 = torch.clamp(l0 + 1, max=n - 1)
        f = lc - l0.to(lc.dtype)
        dist = lambda x: (x - torch.round(x)).abs()
        inf = torch.full_like(f, float("inf"))
        unclamped = (rough > min_roughness) & (rough < 1.0)
        level_edge = torch.where(unclamped, dist(lc), inf)
        edge = inf.clone()
        keys = torch.full((dirs.shape[0], 8), -1, dtype=torch.int64, device=dirs.device)
        for li, r_ in enumerate(mip_res):
            use0, use1 = (l0 == li) & (f < 1), (l1 == li) & (f > 0) & (l1 != l0)
            use = use0 | use1
            if not bool(use.any()):
                continue
            idx, w, fx, fy, _ = bilinear_taps(r_, dirs)
            edge = torch.where(use, torch.minimum(edge, torch.minimum(dist(fx), dist(fy)) / r_), edge)
            for k in range(4):
                key = (li << 24) | idx[k]
                keys[:, k] = torch.where(use0 & (w[k] != 0), key, keys[:, k])
                keys[:, 4 + k] = torch.where(use1 & (w[k] != 0), key, keys[:, 4 + k])
        a = dirs.abs()
        top = a.topk(2, dim=1).values
        face_gap = (top[:, 0] - top[:, 1]) / top[:, 0]
        fg_uv = torch.stack([ndv, rough], -1).clamp(0, 1)
    return dict(keys=keys, cell_edge=edge, level_edge=level_edge, face_gap=face_gap, ndv=ndv, lut_uv=fg_uv, level=level)


HASH_SIZE, HASH_PROBES, TILE_W, TILE_H, CHECK_EVERY = 4096, 8, 64, 12, 4


def _hash_slot(key):
    return ((key * 2654435761) & 0xFFFFFFFF) >> 20          # (key * 2654435761u) >> (32 - 12)


def fused_bwd_schedule(keys, H, W, n_cu, hashed_levels, simulate=(0,)):
    """Host model of the tile schedule of shade_fused_bwd_kernel (csrc/mrgs_shade.hip): tiles of 64 x 12 pixels, tile t on workgroup
    t mod min(ntiles, n_cu), the hash table's fill checked after every fourth tile of a workgroup (flushed when more than half of it was
    taken since the last flush).  keys [H*W, 8] (shade_taps; -1 = no tap); only levels in `hashed_levels` go through the table (the
    others sit in the dense LDS copy).  For every workgroup the distinct hashed keys of each 4-tile window are counted (a window with
    more than 4 096 cannot fit the table: some lanes take the global fallback); for the workgroups in `simulate` the table is replayed
    key by key in pixel order (CAS insert, linear probing, 8 probes) -> inserts, fallbacks and flushes between tiles.
    Returns dict(ntiles, grid, tiles_per_wg, max_window_keys, windows_over_table, sim: {wg: dict(fallbacks, mid_flushes, inserts)})."""
    import numpy as np
    keys = keys.detach().cpu().numpy().reshape(H, W, 8)
    lev = np.where(keys >= 0, keys >> 24, -1)
    keys = np.where(np.isin(lev, list(hashed_levels)), keys, -1)
    tiles_x, tiles_y = (W + TILE_W - 1) // TILE_W, (H + TILE_H - 1) // TILE_H
    ntiles = tiles_x * tiles_y
    grid = min(ntiles, n_cu)

    def tile_keys(t):
        x, y = (t % tiles_x) * TILE_W, (t // tiles_x) * TILE_H
        k = keys[y:y + TILE_H, x:x + TILE_W].reshape(-1)
        return k[k >= 0]

    max_win, over = 0, 0
    for wg in range(grid):
        ts = list(range(wg, ntiles, grid))
        for w0 in range(0, len(ts), CHECK_EVERY):
            d = np.unique(np.concatenate([tile_keys(t) for t in ts[w0:w0 + CHECK_EVERY]])).size
            max_win = max(max_win, d)
            over += d > HASH_SIZE
    sim = {}
    for wg in simulate:
        table, taken, flushed_at, fallbacks, mid = {}, 0, 0, 0, 0
        ts = list(range(wg, ntiles, grid))
        for i, t in enumerate(ts):
            for key in tile_keys(t).tolist():
                h = _hash_slot(key)
                for _ in range(HASH_PROBES):
                    old = table.get(h)
                    if old is None:
                        table[h] = key
                        taken += 1
                        break
                    if old == key:
                        break
                    h = (h + 1) & (HASH_SIZE - 1)
                else:
                    fallbacks += 1
            if (i + 1) % CHECK_EVERY == 0 and taken - flushed_at > HASH_SIZE // 2:
                table, flushed_at = {}, taken
                mid += i + 1 < len(ts)          # tiles follow: the flushed slots are taken again in this launch
        sim[wg] = dict(fallbacks=fallbacks, mid_flushes=mid, inserts=taken)
    return dict(ntiles=ntiles, grid=grid, tiles_per_wg=(ntiles + grid - 1) // grid, max_window_keys=max_win, windows_over_table=over, sim=sim)
