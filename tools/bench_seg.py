#!/usr/bin/env python3
"""Part segmentation on one device, two comparisons, each with both sides alternating in one process:

  (a) labels of the fine samples of one C1 frame (128 x 128 rays x 64 samples, P = 23):
        seg    ops.part_labels_on_rays - one launch of seg_label_kernel, the points formed in the kernel;
        query  the only route to per-point part weights without libenarf_seg.so: ops.query_fwd(debug=True) on the same
               points (formed beforehand, outside the timing), which materialises (B, P, 3, N) canonical coordinates and
               (B, P, N) weights and runs the feature gather and the MLP, then a masked arg-max in torch.
  (b) TriPlaneNARF.render_entire_img at 128 x 128: semantic_map=True (march with taps + labels + composite) against the
      plain call.

Device events around each side, one warm-up round, the median of --runs rounds; the number of kernel launches of each
side (torch.profiler, a round of its own). Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from _helpers import DeviceScene, Scene  # noqa: E402
from enarf_gan_amd import ops, synth  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


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


def alternate(sides, runs):
    """{name: fn} -> {name: median ms}, the sides taking turns within each round"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(runs):
        for k, fn in sides.items():
            times[k].append(timed(fn)[0])
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--nc", type=int, default=48)
    ap.add_argument("--nf", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    S, Nc, Nf = args.size, args.nc, args.nf
    sc = Scene(S, 1, "center_fixed", 20)
    ds = DeviceScene(sc)
    coord = sc.raw["image_coord"].to(ds.dev)
    out = ds.render(coord, Nc, Nf, None, seed=1, debug=True)
    t = out.taps
    P = sc.P

    def seg():
        return ops.part_labels_on_rays(coord, ds.inv_K, t["depth_min"], t["depth_max"], t["bins"], ds.parts, ds.cpose, ds.tri)

    ray = torch.einsum("bij,bjn->bin", ds.inv_K, coord.reshape(1, 3, -1))
    b_ = t["bins"][:, None]
    start, end = (t["depth_min"][:, None] * ray)[..., None], (t["depth_max"][:, None] * ray)[..., None]
    pts = (start * (1 - b_) + end * b_).reshape(1, 3, -1).contiguous()
    shifts = torch.arange(P, device=ds.dev, dtype=torch.int32)[None, :, None]

    def query():
        _, _, vb, _, dw = ds.query(pts, debug=True)
        valid = ((vb[:, None] >> shifts) & 1).bool()
        w = torch.where(valid, dw, torch.full_like(dw, float("-inf")))
        top, label = w.max(dim=1)
        return torch.where(vb != 0, label.int(), torch.full_like(vb, -1)), top

    a_ms, a_runs = alternate({"seg": seg, "query": query}, args.runs)
    la, lq = seg()[0].reshape(1, -1), query()[0]
    agree = float((la == lq).float().mean())

    from enarf_gan_amd.models.narf import TriPlaneNARF
    m = TriPlaneNARF(synth.nerf_config(Nc=Nc, Nf=Nf, mlp_mode="f16x3"), 20, 24, parent=sc.raw["parents"], num_bone_param=23)
    m.register_canonical_pose(sc.raw["canonical_pose"])
    m.load_state_dict({f"mlp.{k}": v for k, v in sc.raw["mlp"].items()}, strict=False)
    with torch.no_grad():
        m.tri_plane.copy_(sc.raw["tri_plane"][:1])
    m = m.to(ds.dev).eval()
    s = sc.raw
    margs = (s["pose_to_camera"].to(ds.dev), ds.inv_K, None, s["z_rend"].to(ds.dev), s["bone_length"].to(ds.dev))

    def plain():
        return m.render_entire_img(*margs, render_size=S, Nc=Nc, Nf=Nf)

    def semantic():
        return m.render_entire_img(*margs, render_size=S, Nc=Nc, Nf=Nf, semantic_map=True)

    b_ms, b_runs = alternate({"semantic": semantic, "plain": plain}, args.runs)
    part_map = m.buffers_tensors["part_map"] if semantic() is not None else None
    print(json.dumps({"tool": "bench_seg", "size": S, "Nc": Nc, "Nf": Nf, "P": P, "points": int(pts.shape[-1]),
                      "a_label_ms": a_ms, "a_label_runs": a_runs, "a_labels_agree": agree,
                      "a_launches": {"seg": launches(seg), "query": launches(query)},
                      "b_frame_ms": b_ms, "b_frame_runs": b_runs,
                      "b_launches": {"semantic": launches(semantic), "plain": launches(plain)},
                      "labelled_rays": int((part_map >= 0).sum()), "parts_in_map": int(part_map[part_map >= 0].unique().numel())}),
          flush=True)


if __name__ == "__main__":
    main()
