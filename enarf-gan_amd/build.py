"""Build recipe of the HIP libraries (hipcc, gfx950 only), in-tree under csrc/: the tables LIBRARIES, SIDE_LIBRARIES and
LATE_LIBRARIES below are the one place a library is declared, one libenarf_<stem>.so per row.

`python -m enarf_gan_amd.build` or `build()`; `__graft_entry__.build()` calls this. The .so files are
git-ignored but travel to the GPU box with the repo snapshot. `python -m enarf_gan_amd.build --variant NAME [-DFLAG=V ...]`
is what tools/build_variant.sh runs: a second build of libenarf_hip.so under variants/.

Adding a library: a row, its public header under include/, a binding module `_<stem>_lib.py` (constants, SIGNATURES, a
`_loader.Library`, the ops) and a kernel -> GPU tests map. Rows of LIBRARIES have their maps in tests/kernel_coverage.py and
are checked by tests/test_libraries_cpu.py (ABI, inventory, disjointness, header tracking); rows of SIDE_LIBRARIES have a
registry module each (tests/<stem>_kernel_coverage.py) and get the same checks from tests/test_side_libraries_cpu.py; a row
of LATE_LIBRARIES brings its registry module, the same checks and its poison cases in test files of its own
(tests/test_<stem>_cpu.py, tests/<stem>_poison_cases.py).
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
# stem -> (sources under csrc/, public header under include/). Each library's kernel inventory is closed and checked on
# its own: no kernel of one row is part of another's.
LIBRARIES = {
    "hip": (["enarf_render.hip", "enarf_render_bwd.hip", "enarf_sampler.hip", "enarf_raysample.hip", "enarf_gan_ops.hip"],
            "enarf_hip.h"),
    "mesh": (["enarf_mesh.hip"], "enarf_mesh.h"),          # marching cubes
    "raster": (["enarf_raster.hip"], "enarf_raster.h"),    # the mesh rasteriser
    "pose": (["enarf_pose.hip"], "enarf_pose.h"),          # the pose prior's bone masks
    "photo": (["enarf_photo.hip"], "enarf_photo.h"),       # the photometric loss and image metrics of the single-scene path
    "guide": (["enarf_guide.hip"], "enarf_guide.h"),       # the mask-guidance loss of the GAN's generator
}
# Libraries whose kernel registry is not in tests/kernel_coverage.py (that file holds one map per row of LIBRARIES and
# stays as it is): same recipe, same binding conventions, built and loaded with the rest; each brings its registry and the
# checks that tests/test_libraries_cpu.py makes per row in test files of its own (tests/<stem>_kernel_coverage.py, e.g.
# tests/anim_kernel_coverage.py, and tests/test_side_libraries_cpu.py, which is parametrised over this table).
SIDE_LIBRARIES = {
    "anim": (["enarf_anim.hip"], "enarf_anim.h"),          # pose interpolation and 8-bit frames of an animation
    "seg": (["enarf_seg.hip"], "enarf_seg.h"),             # part labels of sample points and the semantic map of a frame
    "paint": (["enarf_paint.hip"], "enarf_paint.h"),       # deferred shading of a rasterised mesh: vertex colours, part labels
    "bake": (["enarf_bake.hip"], "enarf_bake.h"),          # the texture atlas of a mesh: texel points, RGBA8 texture, textured shade
    "simp": (["enarf_simp.hip"], "enarf_simp.h"),          # mesh simplification: vertex clustering with quadric placement
    "geom": (["enarf_geom.hip"], "enarf_geom.h"),          # depth, point and normal maps of a march, running depth error
    "pgrad": (["enarf_pgrad.hip"], "enarf_pgrad.h"),       # the query's gradient for the sample points and the part frames
    "scene": (["enarf_scene.hip"], "enarf_scene.h"),       # several avatars marched on the same rays, composed into one image
    "sgrad": (["enarf_sgrad.hip"], "enarf_sgrad.h"),       # the scene composite's gradient for the avatars' densities and colours
    "nrm": (["enarf_nrm.hip"], "enarf_nrm.h"),             # the density's spatial gradient: ray, pixel and vertex normals
    "skin": (["enarf_skin.hip"], "enarf_skin.h"),          # skin weights of mesh vertices, linear-blend posing of the mesh
}
ALL_LIBRARIES = {**LIBRARIES, **SIDE_LIBRARIES}
# Libraries added after the tests of the two tables above were bound to them (tests/test_skin_cpu.py names the last side
# row, tests/poison_cases.py holds a case for every function of every row of ALL_LIBRARIES, and both files stay as they
# are): the move that created SIDE_LIBRARIES, made once more. Same recipe, same binding conventions, built and loaded with
# the rest; each row brings, in test files of its own, its registry (tests/<stem>_kernel_coverage.py), the per-row checks
# of tests/test_side_libraries_cpu.py (tests/test_<stem>_cpu.py) and its poison cases (tests/<stem>_poison_cases.py).
LATE_LIBRARIES = {
    "nmap": (["enarf_nmap.hip"], "enarf_nmap.h"),          # tangent-space normal maps in the atlas: encode, normal-mapped shade
}
EVERY_LIBRARY = {**ALL_LIBRARIES, **LATE_LIBRARIES}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         "-I", os.path.join(ROOT, "include"), "-I", CSRC]


def lib_path(stem: str) -> str:
    return os.path.join(CSRC, f"libenarf_{stem}.so")


def binding(stem: str) -> str:
    """name of the module that binds the row's library"""
    return "enarf_gan_amd._lib" if stem == "hip" else f"enarf_gan_amd._{stem}_lib"


def lib_deps(stem: str) -> list:
    """What every object of the row depends on: every header next to the sources (a list by name went stale when
    enarf_tasks.h was added), include/enarf_hip.h, the row's own public header and this file."""
    include = os.path.join(ROOT, "include")
    return ([os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")] +
            [os.path.join(include, "enarf_hip.h"), os.path.join(include, EVERY_LIBRARY[stem][1]), os.path.abspath(__file__)])


LIB = lib_path("hip")
# the names earlier callers use, all read from the table
MESH_LIB, RASTER_LIB, POSE_LIB, PHOTO_LIB, GUIDE_LIB = (lib_path(s) for s in ("mesh", "raster", "pose", "photo", "guide"))
ANIM_LIB, SEG_LIB = lib_path("anim"), lib_path("seg")
SOURCES, HEADERS = LIBRARIES["hip"][0], lib_deps("hip")


def _newer(a: str, b: str) -> bool:
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def _make(targets, force, verbose, extra_flags) -> None:
    """targets: (library, object directory, sources, dependencies) each; compiles what is out of date, then links"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    libs, jobs = [], []
    for lib, obj_dir, sources, deps in targets:
        objs, n_jobs = [], len(jobs)
        for src in sources:
            s = os.path.join(CSRC, src)
            o = os.path.join(obj_dir, src.replace(".hip", ".o"))
            objs.append(o)
            if force or _newer(s, o) or any(_newer(d, o) for d in deps):
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

    with ThreadPoolExecutor(max_workers=sum(len(t[2]) for t in targets)) as ex:
        list(ex.map(run, jobs))
    for lib, objs, rebuilt in libs:
        if rebuilt or force or not os.path.exists(lib) or any(_newer(o, lib) for o in objs):
            run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs])


def build(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    """Build every library of LIBRARIES, SIDE_LIBRARIES and LATE_LIBRARIES incrementally; returns the path of libenarf_hip.so (the others
    are next to it, at lib_path(stem))."""
    _make([(lib_path(stem), CSRC, sources, lib_deps(stem)) for stem, (sources, _) in EVERY_LIBRARY.items()],
          force, verbose, extra_flags)
    return LIB


def build_variant(name: str, extra_flags=()) -> str:
    """A second build of the `hip` row with extra compiler flags: variants/libenarf_NAME.so, objects under
    variants/obj_NAME/ (git-ignored; loaded through _lib.use_variant by the measurement tools)."""
    out = os.path.join(ROOT, "variants")
    os.makedirs(os.path.join(out, "obj_" + name), exist_ok=True)
    lib = os.path.join(out, f"libenarf_{name}.so")
    _make([(lib, os.path.join(out, "obj_" + name), LIBRARIES["hip"][0], lib_deps("hip"))], True, True, extra_flags)
    return lib


if __name__ == "__main__":
    if "--variant" in sys.argv:
        at = sys.argv.index("--variant")
        print(build_variant(sys.argv[at + 1], sys.argv[at + 2:]))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
