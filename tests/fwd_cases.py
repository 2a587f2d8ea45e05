"""The case table of the forward march's float64 matrix (tests/test_gpu_forward_f64.py; tests/test_fwd_referee_cpu.py checks
the oracle-only conditions every case must meet). All cases: 32^2 scenes, 8 rays of the first row (they miss every cube) and
the rest through the body, explicit sorted random bins - so a referee does not depend on the kernel."""
import torch
import torch.nn.functional as F

from _helpers import Scene


def rays(S, n_body, n_miss, seed):
    """n_body ray ids through the middle rows of an S x S frame (most hit a cube) and n_miss from its first row (none do)"""
    g = torch.Generator().manual_seed(seed)
    body = S * (S // 2 - 2) + torch.randperm(4 * S, generator=g)[:n_body]
    miss = torch.arange(n_miss)
    return torch.cat([miss, body.sort().values])


_D = dict(ol="center_fixed", style_dim=20, B=1, Nc=32, Nf=33, body=40, render_scale=1.0, modes={}, planes=None, mask_scale=1.0,
          feat_scale=1.0)
OPAQUE_FEATURE_SCALE = 12.0

CASES = {
    # fine count, one sample per lane: ragged 16-sample tiles, and the minimum
    "nf2": dict(Nf=2), "nf17": dict(Nf=17), "nf33": dict(Nf=33), "nf64": dict(Nf=64),
    # two samples per lane
    "nc72_nf65": dict(Nc=72, Nf=65), "nc72_nf128": dict(Nc=72, Nf=128),
    # ragged coarse tile
    "nc33_nf17": dict(Nc=33, Nf=17),
    # parts, style, batch (a batch marches the rays that miss every cube; per-image tri-planes)
    "p24_style256": dict(ol="center+head", style_dim=256), "b2_style256": dict(style_dim=256, B=2, body=16),
    "b3_center": dict(ol="center", B=3, body=12),
    "scale0.5": dict(render_scale=0.5), "scale2": dict(render_scale=2.0),
    # density modes; clamp_mask with the part planes x 3, so that plane samples leave [-2, 5]
    "clamp_mask": dict(modes=dict(clamp_mask=True), mask_scale=3.0),
    "density_x_weight": dict(modes=dict(multiply_density_with_weight=True)),
    "no_selector": dict(modes=dict(no_selector=True, multiply_density_with_weight=True)),
    # planes resampled from the scene's: the footprint of a sample is clamped at every border
    "planes24x40": dict(planes=(24, 40)), "planes2x5": dict(planes=(2, 5)), "planes2x2": dict(planes=(2, 2)),
    # opaque rays: the first valid samples saturate, the weights after them underflow
    "opaque": dict(feat_scale=OPAQUE_FEATURE_SCALE),
}


def build(name):
    """-> dict(sc, coord (B,3,n), bins (B,n,Nf), Nc, Nf, render_scale, modes (the oracle's keywords), kflags (ops.render_fwd's))"""
    c = {**_D, **CASES[name]}
    sc = Scene(32, c["B"], c["ol"], c["style_dim"])
    tri = sc.raw["tri_plane"].clone()
    tri[:, :96] *= c["feat_scale"]
    tri[:, 96:] *= c["mask_scale"]
    if c["planes"]:
        tri = F.interpolate(tri, size=c["planes"], mode="bilinear", align_corners=False)
    sc.raw["tri_plane"] = tri.contiguous()
    seed = sorted(CASES).index(name)
    ids = rays(32, c["body"], 8, seed)
    coord = sc.raw["image_coord"].reshape(c["B"], 3, -1)[..., ids].contiguous()
    bins = torch.rand(c["B"], len(ids), c["Nf"], generator=torch.Generator().manual_seed(100 + seed)).sort(-1).values
    m = c["modes"]
    kflags = dict(multiply_density_with_weight=m.get("multiply_density_with_weight", False), clamp_mask=m.get("clamp_mask", False),
                  uniform_part_weight=m.get("no_selector", False))
    return dict(sc=sc, coord=coord, bins=bins, Nc=c["Nc"], Nf=c["Nf"], render_scale=c["render_scale"], modes=m, kflags=kflags)


# ---- points placed in canonical space, for enarf_query_fwd / enarf_query_bwd
def place(sc, b, k, canon):
    """canonical points (3, M) float64 of part k of image b -> camera points of the scaled space (3, M) float32"""
    Rc, tc = sc.cpose[k, :3, :3].double(), sc.cpose[k, :3, 3].double()
    pose = sc.pose_scaled[b, k].double()
    s = sc.scale[b, k].double()
    local = (Rc.T @ (canon - tc[:, None])) / s
    return (pose[:3, :3] @ local + pose[:3, 3:4]).float()


def query_points(sc, b, H, W):
    """(3, N) points of image b, N % 64 != 0, placed in the canonical cube of part 5 (half-size = its scale s, around its
    canonical origin tc; the points stay within s / 2 of tc so that every one is valid): runs of 16 samples along each
    plane axis inside one texel and across one texel edge, texel centres and texel edges in both plane coordinates, the
    valid region's faces, and points far from every part."""
    k = 5
    tc = sc.cpose[k, :3, 3].double()
    lim = 0.5 * float(sc.scale[b, k])
    cx = lambda i, n: (2 * i + 1) / n - 1                     # texel centre i of n
    ex = lambda i, n: (2 * i + 2) / n - 1                     # edge between texels i and i + 1
    near = lambda v, n: int(((v + 1) * n - 1) / 2)            # the texel under coordinate v
    pts = []
    for axis in range(3):
        for at in (ex, cx):                                   # 16 samples with one bilinear footprint / with two
            c = tc[:, None].repeat(1, 16)
            u, v = axis, (axis + 1) % 3
            c[u] = at(near(float(tc[u]), W), W) + torch.linspace(-0.6 / W, 0.6 / W, 16, dtype=torch.float64)
            c[v] = cx(near(float(tc[v]), H), H)
            pts.append(place(sc, b, k, c))
    g = torch.Generator().manual_seed(4)
    off = lambda n: torch.randint(-int(lim * n / 2) + 1, int(lim * n / 2) - 1, (40,), generator=g)
    for f in (cx, ex):                                        # centres and edges in every coordinate
        c = torch.stack([f(near(float(tc[d]), W if d != 1 else H) + off(W if d != 1 else H), W if d != 1 else H).double()
                         for d in range(3)])
        pts.append(place(sc, b, k, c))
    c = tc[:, None].repeat(1, 24)                             # close to the faces of the region
    c[0] += torch.tensor([0.999 * lim, -0.999 * lim, 0.5 * lim, -0.5 * lim] * 6, dtype=torch.float64)
    c[1] += torch.linspace(-0.9 * lim, 0.9 * lim, 24, dtype=torch.float64)
    pts.append(place(sc, b, k, c))
    pts.append(torch.full((3, 7), 40.0))
    out = torch.cat(pts, dim=1)
    assert out.shape[1] % 64 != 0
    return out
