"""Build recipe of libenarf_hip.so, libenarf_mesh.so, libenarf_raster.so, libenarf_pose.so, libenarf_photo.so and
libenarf_guide.so (hipcc, gfx950 only), in-tree under csrc/.

`python -m enarf_gan_amd.build` or `build()`; `__graft_entry__.build()` calls this. The .so files are
git-ignored but travel to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(CSRC, "libenarf_hip.so")
SOURCES = ["enarf_render.hip", "enarf_render_bwd.hip", "enarf_sampler.hip", "enarf_raysample.hip", "enarf_gan_ops.hip"]
# every header next to the sources is a dependency of every object (a list by name went stale when enarf_tasks.h was added)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(ROOT, "include", "enarf_hip.h")]
# marching cubes (include/enarf_mesh.h) is a library of its own: its kernels are not part of libenarf_hip.so's inventory
MESH_SOURCES = ["enarf_mesh.hip"]
MESH_LIB = os.path.join(CSRC, "libenarf_mesh.so")
MESH_HEADERS = [os.path.join(ROOT, "include", "enarf_mesh.h")]
# the mesh rasteriser (include/enarf_raster.h) is a third library, outside both inventories above
RASTER_SOURCES = ["enarf_raster.hip"]
RASTER_LIB = os.path.join(CSRC, "libenarf_raster.so")
RASTER_HEADERS = [os.path.join(ROOT, "include", "enarf_raster.h")]
# the pose prior's bone masks (include/enarf_pose.h) are a fourth library, outside all three inventories above
POSE_SOURCES = ["enarf_pose.hip"]
POSE_LIB = os.path.join(CSRC, "libenarf_pose.so")
POSE_HEADERS = [os.path.join(ROOT, "include", "enarf_pose.h")]
# the photometric loss and image metrics of the single-scene path (include/enarf_photo.h) are a fifth library
PHOTO_SOURCES = ["enarf_photo.hip"]
PHOTO_LIB = os.path.join(CSRC, "libenarf_photo.so")
PHOTO_HEADERS = [os.path.join(ROOT, "include", "enarf_photo.h")]
# the mask-guidance loss of the GAN's generator (include/enarf_guide.h) is a sixth library
GUIDE_SOURCES = ["enarf_guide.hip"]
GUIDE_LIB = os.path.join(CSRC, "libenarf_guide.so")
GUIDE_HEADERS = [os.path.join(ROOT, "include", "enarf_guide.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         "-I", os.path.join(ROOT, "include"), "-I", CSRC]


def _newer(a: str, b: str) -> bool:
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    """Build the six libraries incrementally; returns the path of libenarf_hip.so (MESH_LIB, RASTER_LIB, POSE_LIB,
    PHOTO_LIB and GUIDE_LIB are next to it)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    deps = [os.path.join(CSRC, h) if not os.path.isabs(h) else h for h in HEADERS] + [os.path.abspath(__file__)]
    libs, jobs = [], []
    for lib, sources, lib_deps in ((LIB, SOURCES, deps), (MESH_LIB, MESH_SOURCES, deps + MESH_HEADERS),
                                   (RASTER_LIB, RASTER_SOURCES, deps + RASTER_HEADERS),
                                   (POSE_LIB, POSE_SOURCES, deps + POSE_HEADERS),
                                   (PHOTO_LIB, PHOTO_SOURCES, deps + PHOTO_HEADERS),
                                   (GUIDE_LIB, GUIDE_SOURCES, deps + GUIDE_HEADERS)):
        objs, n_jobs = [], len(jobs)
        for src in sources:
            s = os.path.join(CSRC, src)
            o = os.path.join(CSRC, src.replace(".hip", ".o"))
            objs.append(o)
            if force or _newer(s, o) or any(_newer(d, o) for d in lib_deps):
                jobs.append([hipcc, *FLAGS, *extra_flags, "-c", s, "-o", o])
        libs.append((lib, objs, len(jobs) > n_jobs))

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)

    n_sources = (len(SOURCES) + len(MESH_SOURCES) + len(RASTER_SOURCES) + len(POSE_SOURCES) + len(PHOTO_SOURCES) +
                 len(GUIDE_SOURCES))
    with ThreadPoolExecutor(max_workers=n_sources) as ex:
        list(ex.map(run, jobs))
    for lib, objs, rebuilt in libs:
        if rebuilt or force or not os.path.exists(lib) or any(_newer(o, lib) for o in objs):
            run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
