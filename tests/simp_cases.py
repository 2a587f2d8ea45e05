"""Inputs the CPU and GPU tests of the mesh simplification share (tests/test_simp_cpu.py, tests/test_gpu_simp.py): hand
meshes of a few vertices, one per edge case of the contract, each with the result worked out by hand, and the 33^3 sphere of
tests/paint_cases.py at cells of 2, 3, 4 and 6 voxels."""
import functools

import numpy as np

import paint_cases
import simp_reference as R

_f = lambda a: np.array(a, np.float32).reshape(-1, 3)
_i = lambda a: np.array(a, np.int64).reshape(-1, 3)
_BELOW_2 = float(np.nextafter(np.float32(2.0), np.float32(0.0)))

# Three vertices in three cells of size 1 from the origin 0: cells (0,0,0), (1,0,0), (0,1,0). Keys ascend with x first, so
# the clusters are 0: (0,0,0), 1: (0,1,0), 2: (1,0,0) and the vertices go to clusters 0, 2, 1.
_ABC = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]

# name -> vertices, triangles, cell, origin and what the contract gives: vertex_cluster, cluster_size, triangles, and
# vertices (quadric placement) where they are simple enough to state; `mean` where the mean placement differs
HAND = {
    # one triangle inside one cell: one cluster, nothing left of the triangle. Its plane passes through the cell, the
    # regulariser picks the plane's point nearest the mean - the mean itself, which lies on the plane
    "one_cell": dict(vertices=_f([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [0.25, 0.75, 0.5]]), triangles=_i([[0, 1, 2]]),
                     cell=1.0, origin=(0, 0, 0), vertex_cluster=[0, 0, 0], cluster_size=[3], out_triangles=_i([]),
                     out_vertices=_f([[1.25 / 3, 1.25 / 3, 1.0 / 3]])),
    # a triangle across three cells: every cluster holds one vertex, the plane passes through it: it stays where it is
    "three_cells": dict(vertices=_f(_ABC), triangles=_i([[0, 1, 2]]), cell=1.0, origin=(0, 0, 0), vertex_cluster=[0, 2, 1],
                        cluster_size=[1, 1, 1], out_triangles=_i([[0, 2, 1]]),
                        out_vertices=_f([_ABC[0], _ABC[2], _ABC[1]])),
    # two triangles on other vertices of the same three cells, the second named from another corner: one triple
    "same_triple": dict(vertices=_f(_ABC + [[0.25, 0.25, 0.75], [1.75, 0.25, 0.25], [0.25, 1.75, 0.25]]),
                        triangles=_i([[0, 1, 2], [4, 5, 3]]), cell=1.0, origin=(0, 0, 0), vertex_cluster=[0, 2, 1, 0, 2, 1],
                        cluster_size=[2, 2, 2], out_triangles=_i([[0, 2, 1]])),
    # a triple and its reverse are two triangles; lexicographic order puts (0, 1, 2) first
    "reverse": dict(vertices=_f(_ABC), triangles=_i([[0, 1, 2], [2, 1, 0]]), cell=1.0, origin=(0, 0, 0),
                    vertex_cluster=[0, 2, 1], cluster_size=[1, 1, 1], out_triangles=_i([[0, 1, 2], [0, 2, 1]]),
                    out_vertices=_f([_ABC[0], _ABC[2], _ABC[1]])),
    # (v - origin) / h an integer: the vertex belongs to the upper cell; one ulp below it to the lower one. h = 0.25 and
    # origin -1: x = -0.5 is cell 2 exactly; x = 2 from origin 0 with h = 1 is the second case below
    "on_a_face": dict(vertices=_f([[-0.5, -1.0, -1.0], [float(np.nextafter(np.float32(-0.5), np.float32(-1.0))), -1.0, -1.0],
                                   [-1.0, -1.0, -1.0]]), triangles=_i([[0, 1, 2]]), cell=0.25, origin=(-1, -1, -1),
                      vertex_cluster=[2, 1, 0], cluster_size=[1, 1, 1], out_triangles=_i([[0, 2, 1]])),
    "on_a_face_h1": dict(vertices=_f([[2.0, 0.5, 0.5], [_BELOW_2, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 2.5, 0.5]]),
                         triangles=_i([[0, 1, 3], [1, 2, 3]]), cell=1.0, origin=(0, 0, 0), vertex_cluster=[3, 2, 0, 1],
                         cluster_size=[1, 1, 1, 1], out_triangles=_i([[0, 1, 2], [1, 3, 2]])),
    # vertex 3 is named by no triangle: a cluster of its own with trace(A) = 0, placed at the mean - itself
    "unreferenced": dict(vertices=_f(_ABC + [[2.25, 2.5, 2.75]]), triangles=_i([[0, 1, 2]]), cell=1.0, origin=(0, 0, 0),
                         vertex_cluster=[0, 2, 1, 3], cluster_size=[1, 1, 1, 1], out_triangles=_i([[0, 2, 1]]),
                         out_vertices=_f([_ABC[0], _ABC[2], _ABC[1], [2.25, 2.5, 2.75]])),
    # three collinear vertices: n = 0, trace(A) = 0 everywhere, every vertex is its cluster's mean; the triangle is kept
    # (its three clusters differ)
    "zero_area": dict(vertices=_f([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.25, 0.25, 0.25]]),
                      triangles=_i([[0, 1, 2]]), cell=1.0, origin=(0, 0, 0), vertex_cluster=[0, 1, 2, 0], cluster_size=[2, 1, 1],
                      out_triangles=_i([[0, 1, 2]]),
                      out_vertices=_f([[0.375, 0.375, 0.375], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]])),
    # triangles naming vertex V and -1 are ignored everywhere: vertex 3 (named only by them) keeps trace(A) = 0
    "bad_indices": dict(vertices=_f(_ABC + [[2.5, 2.5, 2.5]]), triangles=_i([[0, 1, 4], [0, 1, 2], [-1, 3, 2], [3, 1, 2 ** 40]]),
                        cell=1.0, origin=(0, 0, 0), vertex_cluster=[0, 2, 1, 3], cluster_size=[1, 1, 1, 1],
                        out_triangles=_i([[0, 2, 1]]), out_vertices=_f([_ABC[0], _ABC[2], _ABC[1], [2.5, 2.5, 2.5]])),
    # a wedge: cell (0,0,0) holds four vertices of two planes, y = 0.2 + 3 x and y = 0.2 + 3 (1 - x) (both extruded along z),
    # that meet at (0.5, 1.7): outside the cell. With reg = 1e-3 the solution is y = (0.11016 + l 0.5) / (0.0648 + l), l =
    # 6.48e-4: 1.68812, clamped to the cell's face y = 1. Cell (0,1,0) holds the other two vertices and sees the same two
    # planes: y = 1 + (0.04536 + l 0.4) / (0.0648 + l) = 1.69703, inside. Both triangles collapse (two corners in a cell).
    "wedge": dict(vertices=_f([[0.1, 0.5, 0.2], [0.1, 0.5, 0.8], [0.4, 1.4, 0.5], [0.9, 0.5, 0.2], [0.6, 1.4, 0.5], [0.9, 0.5, 0.8]]),
                  triangles=_i([[0, 1, 2], [3, 4, 5]]), cell=1.0, origin=(0, 0, 0), vertex_cluster=[0, 0, 1, 0, 1, 0],
                  cluster_size=[4, 2], out_triangles=_i([]), out_vertices=_f([[0.5, 1.0, 0.5], [0.5, 1.69703, 0.5]]),
                  unclamped=_f([[0.5, 1.68812, 0.5], [0.5, 1.69703, 0.5]]), clamped=[True, False],
                  mean=_f([[0.5, 0.5, 0.5], [0.5, 1.4, 0.5]])),
}

VOXEL = 0.8 / 14.3
SPHERE_CELLS = (2, 3, 4, 6)
SPHERE_RADIUS = 0.8
# what a prototype of the referee gave (the issue's table): cell in voxels -> (clusters, triangles, largest cluster)
SPHERE_TABLE = {2: (769, 1534, 11), 3: (346, 688, 21), 4: (212, 420, 38), 6: (94, 184, 72)}


def sphere_cell(m):
    return float(np.float32(m * VOXEL))


def mesh(name):
    """(vertices, triangles, cell, origin) of a hand mesh"""
    c = HAND[name]
    return c["vertices"], c["triangles"], c["cell"], c["origin"]


@functools.lru_cache(maxsize=None)
def referee(name, placement):
    """the referee's result for a hand mesh (a name of HAND) or the sphere (a cell in voxels), computed once"""
    if name in HAND:
        v, t, h, o = mesh(name)
        return R.simplify(v, t, h, origin=o, placement=placement)
    v, t = paint_cases.sphere()
    return R.simplify(v, t, sphere_cell(name), placement=placement)


ALL = list(HAND) + list(SPHERE_CELLS)
