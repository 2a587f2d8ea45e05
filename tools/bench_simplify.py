#!/usr/bin/env python3
"""Mesh simplification (libenarf_simp.so) on the synthetic scene of tools/bench_mesh.py: the extract_mesh mesh at voxel 0.02
(242 712 triangles) and the mesh of the reference's 667^3 lattice (voxel 0.003), each at cells of 2, 4 and 8 voxels.

Per mesh and cell:
  stages    the three kernels each on its own (simp_key_kernel, simp_corner_kernel, simp_place_kernel<quadric>) and the torch
            calls between them (the stable sort and unique_consecutive of the keys, the sort of the incidence slots, the
            compaction of the triples), device events over --batch back-to-back calls, median of --runs with the spread
            (min, max); the kernel launches of each; the compulsory traffic of each kernel and the rate it reached;
  whole     ops.simplify_mesh against the same result composed from torch calls (index_add_ sums in fp64, a batched
            linalg.solve, unique(dim=0)), the sides taking turns; whether the triangles are equal and how far the vertices
            are apart; extract_mesh itself beside them. A row says so when the torch composition is the faster one.
Quality, on the voxel 0.02 mesh: simplify(fine, cell) against marching cubes at the voxel that gives the nearest triangle
count - the volume of each over the fine mesh's, and the mean distance of its vertices to the fine mesh's surface (the
exact point-triangle distance to the 16 fine triangles whose centroids are nearest). Last, bake_texture at 1024 of the
voxel 0.02 mesh simplified to the atlas's capacity, beside the refusal of the fine mesh. One JSON line per result, also
appended to --log. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from enarf_gan_amd import _simp_lib as S  # noqa: E402
from enarf_gan_amd import ops, synth  # noqa: E402
from enarf_gan_amd.libraries.NARF.mesh_rendering import bake_texture, extract_mesh, simplify_steps  # noqa: E402
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
    """{name: fn} -> {name: [median, min, max] ms per call}, the sides taking turns within each round"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            times[k].append(timed(fn, batch))
    return {k: [round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)] for k, v in times.items()}


def torch_simplify(verts, tris, h, reg=1e-3):
    """ops.simplify_mesh(placement="quadric") from torch calls: fp64, index_add_ sums (atomics: the last bits vary from run
    to run), one batched solve, unique(dim=0)"""
    dev, V = verts.device, verts.shape[0]
    v = verts.double()
    o = verts.amin(0).double()
    h = float(torch.tensor(h, dtype=torch.float32))
    # a tensor divisor: torch divides by a Python scalar by multiplying with its reciprocal, which moves a vertex on a cell
    # face into the neighbouring cell (one vertex of 8.4 M at voxel 0.003)
    c = torch.floor((v - o) / torch.tensor(h, dtype=torch.float64, device=dev)).long()
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    keys, cluster, counts = torch.unique(key, return_inverse=True, return_counts=True)
    C = keys.shape[0]
    lo = o + torch.stack([keys >> 42, (keys >> 21) & 0x1FFFFF, keys & 0x1FFFFF], -1).double() * h
    mean = torch.zeros(C, 3, dtype=torch.float64, device=dev).index_add_(0, cluster, v - lo[cluster]) / counts[:, None]
    ok = ((tris >= 0) & (tris < V)).all(1)
    t = tris[ok]
    tc = cluster[t]
    A = torch.zeros(C, 9, dtype=torch.float64, device=dev)
    b = torch.zeros(C, 3, dtype=torch.float64, device=dev)
    for k in range(3):
        first = torch.ones(t.shape[0], dtype=torch.bool, device=dev)
        for j in range(k):
            first &= tc[:, j] != tc[:, k]
        ids = tc[first, k]
        p = v[t[first]] - lo[ids][:, None, :]
        n = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        d = (n * p[:, 0]).sum(-1)
        A.index_add_(0, ids, (n[:, :, None] * n[:, None, :]).reshape(-1, 9))
        b.index_add_(0, ids, n * d[:, None])
    A = A.reshape(C, 3, 3)
    trace = A.diagonal(dim1=1, dim2=2).sum(-1)
    lam = reg * trace
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    solve = trace > 0
    M = torch.where(solve[:, None, None], A + lam[:, None, None] * eye, eye)
    x = torch.linalg.solve(M, torch.where(solve[:, None], b + lam[:, None] * mean, mean))
    out = (x.clamp(0.0, h) + lo).float()
    keep = (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2])
    tc = tc[keep]
    r = tc.argmin(1)
    rows = torch.arange(tc.shape[0], device=dev)
    tc = torch.stack([tc[rows, (r + k) % 3] for k in range(3)], -1)
    return out, torch.unique(tc, dim=0)


def volume(verts, tris):
    p = verts.double()[tris]
    return float((p[:, 0] * torch.linalg.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def point_triangle_distance(q, a, b, c):
    """distance of points q (N, 3) to triangles (a, b, c) (N, 3) each, fp64: the closest point by regions (Ericson, Real-Time
    Collision Detection, 5.1.5), written with masks"""
    ab, ac, ap = b - a, c - a, q - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = q - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = q - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    tiny = 1e-300
    denom = (va + vb + vc).clamp_min(tiny)
    closest = a + ab * (vb / denom)[:, None] + ac * (vc / denom)[:, None]                      # the interior
    w = ((d4 - d3) / ((d4 - d3) + (d5 - d6)).clamp_min(tiny))[:, None]
    closest = torch.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], b + w * (c - b), closest)     # edge bc
    w = (d2 / (d2 - d6).clamp_min(tiny))[:, None]
    closest = torch.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], a + w * ac, closest)                    # edge ac
    w = (d1 / (d1 - d3).clamp_min(tiny))[:, None]
    closest = torch.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], a + w * ab, closest)                    # edge ab
    closest = torch.where(((d6 >= 0) & (d5 <= d6))[:, None], c, closest)
    closest = torch.where(((d3 >= 0) & (d4 <= d3))[:, None], b, closest)
    closest = torch.where(((d1 <= 0) & (d2 <= 0))[:, None], a, closest)
    return (q - closest).norm(dim=-1)


def mean_surface_distance(points, verts, tris, nearest=16, chunk=2048):
    """mean over `points` of the distance to the mesh: exact to the `nearest` triangles of the nearest centroids"""
    centre = verts.double().mean(0)                            # centred: cdist's fp32 products lose less
    corners = verts.double()[tris] - centre
    points = (points.double() - centre).float()
    centroids = corners.mean(1).float()
    total = 0.0
    for s in range(0, points.shape[0], chunk):
        q = points[s:s + chunk]
        idx = torch.cdist(q, centroids).topk(min(nearest, centroids.shape[0]), largest=False).indices        # (n, k)
        tri = corners[idx.reshape(-1)]
        d = point_triangle_distance(q.double().repeat_interleave(idx.shape[1], 0), tri[:, 0], tri[:, 1], tri[:, 2])
        total += float(d.reshape(idx.shape).amin(1).sum())
    return total / max(points.shape[0], 1)


def stages(verts, tris, h, args):
    """the rows of one mesh and cell: the stages on their own, then the whole call against torch"""
    V, T = verts.shape[0], tris.shape[0]
    _, _, hf, o = S.check_simplify_args(verts, tris, h)
    keys = S.vertex_keys(verts, hf, o, V)
    ck, vc, counts, vorder, vstart = S.cluster_vertices(keys)
    C = ck.numel()
    triples, inc = S.cluster_corners(tris, vc, V, T, C)
    sorder, sstart = S.incidence_segments(inc, C)
    slots = int(sstart[-1])
    sides = {
        "key_kernel": lambda: S.vertex_keys(verts, hf, o, V),
        "torch_sort_unique_keys": lambda: S.cluster_vertices(keys),
        "corner_kernel": lambda: S.cluster_corners(tris, vc, V, T, C),
        "torch_sort_slots": lambda: S.incidence_segments(inc, C),
        "place_kernel_quadric": lambda: S.place_clusters(verts, tris, ck, vorder, vstart, sorder, sstart, hf, o, 1e-3, True, V, T),
        "place_kernel_mean": lambda: S.place_clusters(verts, tris, ck, vorder, vstart, None, None, hf, o, 1e-3, False, V, T),
        "torch_compact_triples": lambda: S.compact_triples(triples),
    }
    ms = alternate(sides, args.runs, args.batch)
    # compulsory: every array read or written once (a vertex 12 B, an order entry 8 B, a triangle's indices 24 B, per
    # cluster key, two starts and the vertex out). The quadric placement requests more than that: every incidence slot
    # gathers its triangle's indices and nine floats again (68 B a slot), most of which the caches serve.
    traffic = {"key_kernel": 20 * V, "corner_kernel": 60 * T,
               "place_kernel_quadric": 20 * V + 8 * slots + 24 * T + 52 * C, "place_kernel_mean": 20 * V + 36 * C}
    requested = 20 * V + 68 * slots + 52 * C
    row = {"V": V, "T": T, "cell": h, "clusters": C, "slots": slots, "largest_cluster": int(counts.max()),
           "ms_per_call": ms, "launches": {k: launches(fn) for k, fn in sides.items()},
           "compulsory_MB": {k: round(b / 1e6, 2) for k, b in traffic.items()},
           "GBps": {k: round(b / ms[k][0] / 1e6, 1) for k, b in traffic.items()},
           "place_kernel_quadric_requested_MB": round(requested / 1e6, 2),
           "place_kernel_quadric_requested_GBps": round(requested / ms["place_kernel_quadric"][0] / 1e6, 1)}
    ours = lambda: ops.simplify_mesh(verts, tris, h)
    composed = lambda: torch_simplify(verts, tris, h)
    got, (tv, tt) = ours(), composed()
    whole = alternate({"simplify_mesh": ours, "torch_composition": composed}, args.runs, max(1, args.batch // 4))
    row["whole_ms_per_call"] = whole
    row["whole_launches"] = {"simplify_mesh": launches(ours), "torch_composition": launches(composed)}
    row["triangles_out"] = got.triangles.shape[0]
    row["triangles_equal_torch"] = bool(got.triangles.shape == tt.shape and torch.equal(got.triangles, tt))
    row["vertices_vs_torch_max_abs"] = float((got.vertices - tv).abs().max()) if got.vertices.shape == tv.shape else None
    row["bit_identical_twice"] = bool(torch.equal(got.vertices, ours().vertices))
    if whole["torch_composition"][0] < whole["simplify_mesh"][0]:
        row["note"] = "the torch composition is the faster one at this size"
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--voxels", default="0.02,0.003")
    ap.add_argument("--multiples", default="2,4,8")
    ap.add_argument("--quality-voxel", type=float, default=0.02)
    ap.add_argument("--atlas", type=int, default=1024)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r21_simplify.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify.py measures on the GPU; none is available (nothing was measured)")

    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    log = open(args.log, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    sc = synth.make_scene(SIZE, 1, "center_fixed", 20)
    m = TriPlaneNARF(synth.nerf_config(origin_location="center_fixed"), 20, 24, parent=sc["parents"], num_bone_param=23)
    m.register_canonical_pose(sc["canonical_pose"])
    m.load_state_dict({f"mlp.{k}": v for k, v in sc["mlp"].items()}, strict=False)
    with torch.no_grad():
        m.tri_plane.copy_(sc["tri_plane"][:1])
    m = m.cuda().eval()
    pose, bl, z = sc["pose_to_camera"].cuda(), sc["bone_length"].cuda(), sc["z_rend"].cuda()
    center, pose_parts, mi = m._mesh_inputs(pose, None, z, bl, 0.4)
    mesh_at = lambda voxel: extract_mesh(m, pose_parts, center, voxel, MESH_TH, mi)
    emit({"device": torch.cuda.get_device_name(0), "runs": args.runs, "batch": args.batch, "ms": "[median, min, max]"})
    multiples = [int(x) for x in args.multiples.split(",")]

    for voxel in (float(v) for v in args.voxels.split(",")):
        verts, tris = mesh_at(voxel)
        extract = alternate({"extract_mesh": lambda: mesh_at(voxel)}, args.runs, 1)
        emit({"voxel": voxel, "V": verts.shape[0], "T": tris.shape[0], "ms_per_call": extract})
        for k in multiples:
            row = stages(verts, tris, k * voxel, args)
            emit({"voxel": voxel, "cell_voxels": k, **row})
        del verts, tris
        torch.cuda.empty_cache()

    # quality at an equal triangle count: simplify(fine, cell) against marching cubes at a coarser voxel
    voxel = args.quality_voxel
    fine_v, fine_t = mesh_at(voxel)
    fine_volume = volume(fine_v, fine_t)
    coarse = {}
    voxel_of = lambda cube: (1.0 - 1e-9) / cube                # int(1 / voxel) == cube, whatever the division rounds to
    for cube in range(4, int(1 / voxel)):                      # the lattice is 2 cube + 1 a side: T steps with cube
        cv, ct = mesh_at(voxel_of(cube))
        coarse[cube] = ct.shape[0]
    for k in multiples:
        got = ops.simplify_mesh(fine_v, fine_t, k * voxel)
        mean = ops.simplify_mesh(fine_v, fine_t, k * voxel, placement="mean")
        cube = min(coarse, key=lambda c: abs(coarse[c] - got.triangles.shape[0]))
        cv, ct = mesh_at(voxel_of(cube))
        emit({"quality_of": f"voxel {voxel} mesh, {fine_t.shape[0]} triangles, volume {fine_volume:.6f}", "cell_voxels": k,
              "simplified": {"T": got.triangles.shape[0], "V": got.vertices.shape[0],
                             "volume_over_fine": round(volume(got.vertices, got.triangles) / fine_volume, 5),
                             "mean_distance_to_fine_surface": mean_surface_distance(got.vertices, fine_v, fine_t)},
              "simplified_mean_placement": {"T": mean.triangles.shape[0],
                                            "volume_over_fine": round(volume(mean.vertices, mean.triangles) / fine_volume, 5),
                                            "mean_distance_to_fine_surface": mean_surface_distance(mean.vertices, fine_v, fine_t)},
              "marching_cubes": {"voxel": round(1.0 / cube, 5), "T": ct.shape[0], "V": cv.shape[0],
                                 "volume_over_fine": round(volume(cv, ct) / fine_volume, 5),
                                 "mean_distance_to_fine_surface": mean_surface_distance(cv, fine_v, fine_t)}})

    # the atlas the fine mesh does not fit: simplified to its capacity, then baked
    A = args.atlas
    try:
        ops.bake_layout(fine_t.shape[0], A)
        emit({"atlas": A, "fine_mesh": "fits"})
    except NotImplementedError as e:
        capacity = 2 * (A // 6) ** 2
        best, steps = simplify_steps(fine_v, fine_t, capacity)
        cell = min(h for h, n in steps if n <= capacity)
        bake = lambda: bake_texture(m, pose_parts, best.vertices, best.triangles, mi, size=A)
        atlas = bake()
        emit({"atlas": A, "fine_mesh_T": fine_t.shape[0], "fine_mesh": "unsupported: " + str(e), "capacity": capacity,
              "simplified_T": best.triangles.shape[0], "simplified_V": best.vertices.shape[0], "cell": round(cell, 5),
              "cell_voxels": round(cell / voxel, 3), "bisection_runs": len(steps), "atlas_cell": atlas.cell,
              "owned_texels": int((atlas.texture[..., 3] == 255).sum()),
              "ms_per_call": alternate({"bake_texture": bake,
                                        "simplify_mesh": lambda: ops.simplify_mesh(fine_v, fine_t, cell)}, args.runs, 1)})
    log.close()


if __name__ == "__main__":
    main()
