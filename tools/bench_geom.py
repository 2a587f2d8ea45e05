#!/usr/bin/env python3
"""Geometry buffers and the running depth error (libenarf_geom.so), measured on the device.

  buffers   ops.geometry_buffers (one launch of geom_buffers_kernel, all five outputs, shade "lit") at (8, 128, 128) and
            (96, 512, 512) on a synthetic undulating surface with a round silhouette, against the same five outputs
            composed from torch calls in fp64 (shifted copies for the stencil, elementwise ops);
  render    render_geometry against forward on the synthetic scene of tools/bench_mesh.py at 128 x 128: what the
            geometry costs on top of the march;
  error     DepthError.update on a batch of (4, 128, 128) against the reference's path for the same batch: a .cpu() of
            both maps and, at the end of the set, one MSELoss on the host (timed per batch with the host clock, the device
            idle before and after);
each device side timed with device events over --batch back-to-back calls, the sides taking turns, the median of --runs
rounds, and the kernel launches of one call of each. Last, agreement with the mesh path at one 128 x 128 view of the
scene: the median |depth - zbuf| between the march's depth and the z-buffer of the extracted mesh (voxel 0.003) over the
pixels both cover, and the median angle between the screen-space normals and the rasteriser's. One JSON line per result,
also appended to --log. Needs a GPU: there is no CPU path."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.mesh_rendering import extract_mesh, rasterize_mesh  # noqa: E402
from enarf_gan_amd.models.narf import TriPlaneNARF  # noqa: E402

SIZE, MESH_TH = 128, 15.0


def timed(fn, batch=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name
                   and "emset" not in e.name)
    except Exception as e:      # noqa: BLE001 - the count is a side figure; the times stand without it
        print(f"kernel count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def alternate(sides, runs, batch):
    """{name: fn} -> {name: median ms per call}, the sides taking turns within each round"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            times[k].append(timed(fn, batch))
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in times.items()}


def surface(B, H, W, dev):
    """(disparity, mask (B, H, W), inv_intrinsics (3, 3)): depth 2.5 + waves inside a round silhouette, nothing outside"""
    r, c = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                          indexing="ij")
    phase = torch.arange(B, device=dev, dtype=torch.float64)[:, None, None] * 0.3
    depth = 2.5 + 0.2 * torch.sin(r / H * 9 + phase) * torch.cos(c / W * 7)
    inside = ((r - H / 2) ** 2 + (c - W / 2) ** 2) < (0.42 * min(H, W)) ** 2
    mask = inside.expand(B, -1, -1).double() * 0.9
    f = 1.2 * max(H, W)
    K_inv = torch.linalg.inv(torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=torch.float64))
    return (mask / depth).float().contiguous(), mask.float().contiguous(), K_inv.float().to(dev)


def _shift(t, dr, dc, fill=0.0):
    """t[b, r + dr, c + dc] with `fill` outside, for (B, H, W) or (B, H, W, 3)"""
    lead = (0, 0) if t.dim() == 4 else ()
    pad = lead + (max(-dc, 0), max(dc, 0), max(-dr, 0), max(dr, 0))
    p = F.pad(t, pad, value=fill)
    H, W = t.shape[1:3]
    return p[:, max(dr, 0):max(dr, 0) + H, max(dc, 0):max(dc, 0) + W]


def torch_buffers(q, m, K_inv, edge=0.05, threshold=0.5):
    """geometry_buffers(shade="lit") from torch calls, in fp64 as the kernel computes: (depth, points, normals, flags, image)"""
    B, H, W = q.shape
    valid = torch.isfinite(q) & torch.isfinite(m) & (m >= threshold) & (q > 0)
    z = torch.where(valid, m.double() / q.double(), torch.zeros((), dtype=torch.float64, device=q.device))
    x = torch.arange(W, device=q.device, dtype=torch.float64) + 0.5
    y = torch.arange(H, device=q.device, dtype=torch.float64) + 0.5
    pix = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), torch.ones(H, W, dtype=torch.float64, device=q.device)], -1)
    p = z[..., None] * (pix @ K_inv.double().T)

    def neighbour(dr, dc):
        zn = _shift(z, dr, dc)
        ok = _shift(valid.double(), dr, dc) > 0
        return ok & ((zn - z).abs() <= edge * z), _shift(p, dr, dc)

    def difference(lo, hi):
        (use_lo, p_lo), (use_hi, p_hi) = lo, hi
        return use_lo | use_hi, torch.where(use_hi[..., None], p_hi, p) - torch.where(use_lo[..., None], p_lo, p)

    has_dx, dx = difference(neighbour(0, -1), neighbour(0, 1))
    has_dy, dy = difference(neighbour(-1, 0), neighbour(1, 0))
    n = torch.linalg.cross(dy, dx)
    length = n.norm(dim=-1)
    has = valid & has_dx & has_dy & (length > 0)
    N = torch.where(has[..., None], n / length.clamp(min=1e-300)[..., None], torch.zeros_like(n))
    N = torch.where(((N * p).sum(-1) > 0)[..., None], -N, N)
    c = -(N * p).sum(-1) / p.norm(dim=-1).clamp(min=1e-6)
    spec = torch.where(c > 0, (2 * c * c - 1).clamp(min=0) ** 64, torch.zeros_like(c))
    grey = torch.where(has, 0.5 + 0.3 * c.clamp(min=0) + 0.2 * spec, torch.ones_like(c))
    image = (255 * grey.clamp(0, 1)).floor().to(torch.uint8)[..., None].expand(-1, -1, -1, 3).contiguous()
    flags = valid.to(torch.uint8) | (has.to(torch.uint8) << 1)
    return z.float(), p.float(), N.float(), flags, image


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r13_geom.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geom.py measures on the GPU; none is available (nothing was measured)")
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    emit({"device": torch.cuda.get_device_name(0), "runs": args.runs, "batch": args.batch})

    # ---- the buffers against torch
    for B, H, W in ((8, 128, 128), (96, 512, 512)):
        q, m, K_inv = surface(B, H, W, dev)
        kernel = lambda: ops.geometry_buffers(q, m, K_inv, shade="lit")
        by_torch = lambda: torch_buffers(q, m, K_inv)
        got, want = kernel(), by_torch()
        batch = args.batch if B * H * W < 2 ** 22 else max(args.batch // 10, 2)
        ms = alternate({"geometry_buffers": kernel, "torch": by_torch}, args.runs, batch)
        mb = B * H * W * (8 + 4 + 12 + 12 + 1 + 3) / 1e6
        emit({"what": "buffers", "shape": [B, H, W], "ms_per_call": ms, "batch": batch,
              "launches": {"geometry_buffers": launches(kernel), "torch": launches(by_torch)},
              "compulsory_MB": round(mb, 2), "GB_per_s": round(mb / ms["geometry_buffers"], 1),
              "flags_differ": int((got.flags != want[3]).sum()), "max_level_difference": int((got.image.int() - want[4].int()).abs().max()),
              "max_abs_depth_difference": float((got.depth - want[0]).abs().max()),
              "max_abs_normal_difference": float((got.normals - want[2]).abs().max())})
        del got, want

    # ---- render_geometry against forward, and the mesh path's agreement, on the synthetic scene
    sc = synth.make_scene(SIZE, 1, "center_fixed", 20)
    model = TriPlaneNARF(synth.nerf_config(origin_location="center_fixed"), 20, 24, parent=sc["parents"], num_bone_param=23)
    model.register_canonical_pose(sc["canonical_pose"])
    model.load_state_dict({f"mlp.{k}": v for k, v in sc["mlp"].items()}, strict=False)
    with torch.no_grad():
        model.tri_plane.copy_(sc["tri_plane"][:1])
    model = model.cuda().eval()
    pose, bl, z = sc["pose_to_camera"].cuda(), sc["bone_length"].cuda(), sc["z_rend"].cuda()
    K = sc["intrinsics"][:1].cuda()
    K_inv = torch.linalg.inv_ex(K.float()).inverse
    nc, nf = model.config.Nc, model.config.Nf
    idx = torch.arange(SIZE * SIZE, device=dev)
    pixels = torch.stack([(idx % SIZE + 0.5).float(), (torch.div(idx, SIZE, rounding_mode="floor") + 0.5).float(),
                          torch.ones(SIZE * SIZE, device=dev)])[None, None]
    with torch.no_grad():
        march = lambda: model(1, pixels, pose, K_inv, None, z, bl, Nc=nc, Nf=nf, return_disparity=True)
        geometry = lambda: model.render_geometry(pose, K_inv, None, z, bl, SIZE, Nc=nc, Nf=nf, shade="lit")
        ms = alternate({"forward": march, "render_geometry": geometry}, args.runs, args.batch)
        emit({"what": "render", "size": SIZE, "Nc": nc, "Nf": nf, "ms_per_call": ms,
              "geometry_on_top_ms": round(ms["render_geometry"] - ms["forward"], 4),
              "launches": {"forward": launches(march), "render_geometry": launches(geometry)}})

        _, buffers, _, mask = geometry()
        center, pose_parts, mi = model._mesh_inputs(pose, None, z, bl, 1)
        verts, tris = extract_mesh(model, pose_parts, center, 0.003, MESH_TH, mi)
        frag = rasterize_mesh(verts, tris, K, SIZE, SIZE)
        both = (frag.pix_to_face >= 0) & (buffers.flags[0] & 1 > 0)
        with_normal = both & (buffers.flags[0] & 2 > 0)
        mesh_n = F.normalize(frag.normals[with_normal].double(), dim=-1)
        cos = (buffers.normals[0][with_normal].double() * mesh_n).sum(-1).clamp(-1, 1)
        emit({"what": "agreement", "size": SIZE, "voxel": 0.003, "mesh_th": MESH_TH, "mesh_pixels": int((frag.pix_to_face >= 0).sum()),
              "volume_pixels": int((buffers.flags[0] & 1 > 0).sum()), "both": int(both.sum()),
              "median_abs_depth_minus_zbuf": float((buffers.depth[0][both] - frag.zbuf[both]).abs().median()),
              "median_depth": float(buffers.depth[0][both].median()),
              "median_normal_angle_deg": float(torch.rad2deg(torch.acos(cos)).median()), "with_normal": int(with_normal.sum())})

    # ---- the running error against the reference's host path
    B = 4
    gen_d = torch.rand(B, SIZE, SIZE, device=dev)
    target = torch.rand(B, SIZE, SIZE, device=dev) * (torch.rand(B, SIZE, SIZE, device=dev) < 0.4)
    mask = torch.rand(B, SIZE, SIZE, device=dev)
    err = ops.DepthError()
    update = lambda: err.update(gen_d, target, mask)
    ms = alternate({"DepthError.update": update}, args.runs, args.batch)
    host = []
    for _ in range(args.runs * 4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = gen_d.cpu(), target.cpu()
        host.append((time.perf_counter() - t0) * 1e3)
    kept_gen, kept_gt = [a] * 64, [b] * 64
    t0 = time.perf_counter()
    value = torch.nn.MSELoss()(torch.cat(kept_gen), torch.cat(kept_gt)).item()
    final_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    result = err.result()
    read_ms = (time.perf_counter() - t0) * 1e3
    emit({"what": "error", "shape": [B, SIZE, SIZE], "ms_per_batch": {**ms, "reference_cpu_copies": round(sorted(host)[len(host) // 2], 4)},
          "launches": {"DepthError.update": launches(update)}, "result_host_read_ms": round(read_ms, 4),
          "reference_final_mse_of_64_batches_ms": round(final_ms, 3), "reference_value": value,
          "updates": result["updates"], "inv_depth_mse": result["inv_depth_mse"], "isnan": math.isnan(result["inv_depth_mse"])})
    log.close()


if __name__ == "__main__":
    main()
