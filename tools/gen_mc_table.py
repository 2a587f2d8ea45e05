#!/usr/bin/env python3
"""Generate csrc/enarf_mc_table.h, the marching-cubes case table of libenarf_mesh.so ("Marching cubes").

The table is derived from one rule rather than typed in:
- corner c = dx + 2 dy + 4 dz of a cube is inside when bit c of the case index is set;
- edge ids: x-edges 0-3 (base corner (0, y, z), id y + 2 z), y-edges 4-7 (base (x, 0, z), 4 + x + 2 z),
  z-edges 8-11 (base (x, y, 0), 8 + x + 2 y);
- on each face, the crossing edges are joined by segments: two crossings give one segment; four (inside corners on a
  diagonal) give two, each cutting off one INSIDE corner. The choice depends only on the face's four bits, so the two
  cubes sharing a face draw the same segments;
- each segment is directed so that (face normal) x (segment) points away from the inside side of the face. Every crossing
  edge lies on two faces, so the directed segments form closed loops; a loop's triangles (v1 - v0) x (v2 - v0) then point
  from inside to outside;
- loops are taken in the order of their lowest edge id and fan-triangulated. The fan's apex is the lowest-id edge of
  the loop from which no chord joins two edges of one face. A chord across a four-crossing face could be drawn by the
  cube on the other side of that face too, and the mesh edge would then lie in four triangles (or two flat, opposite
  triangles would cover each other). Such an apex exists for every loop (asserted); 18 of the loops need one other than
  their lowest edge.

`python tools/gen_mc_table.py` rewrites the header; `--check` exits 1 if the committed header differs.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "enarf-gan_amd", "csrc", "enarf_mc_table.h")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def edge_corners(e):
    """edge id -> (axis, base corner position, far corner position)"""
    a, b0, b1 = e >> 2, e & 1, (e >> 1) & 1
    base = [(0, b0, b1), (b0, 0, b1), (b0, b1, 0)][a]
    far = list(base)
    far[a] = 1
    return a, base, tuple(far)


EDGES = [edge_corners(e) for e in range(12)]


def edge_mid(e):
    a, base, _ = EDGES[e]
    m = [float(x) for x in base]
    m[a] = 0.5
    return m


def faces():
    """the 6 faces: (normal axis, side s in {0, 1}, outward normal, 4 corners in cyclic order, 4 edge ids)"""
    out = []
    for a in range(3):
        u, v = [x for x in range(3) if x != a]
        for s in (0, 1):
            cyc = []
            for (pu, pv) in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[a], p[u], p[v] = s, pu, pv
                cyc.append(corner_id(p))
            edges = []
            for k in range(4):
                c0, c1 = cyc[k], cyc[(k + 1) % 4]
                for e in range(12):
                    if {corner_id(EDGES[e][1]), corner_id(EDGES[e][2])} == {c0, c1}:
                        edges.append(e)
            n = [0, 0, 0]
            n[a] = 1 if s else -1
            out.append((a, s, n, cyc, edges))
    return out


FACES = faces()


def cross(p, q):
    return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])


def dot(p, q):
    return sum(x * y for x, y in zip(p, q))


def face_segments(face, inside):
    """directed segments [(from edge, to edge)] the rule draws on one face, given inside(corner) -> bool"""
    _, _, n, cyc, edges = face
    ins = [inside(c) for c in cyc]
    crossing = [edges[k] for k in range(4) if ins[k] != ins[(k + 1) % 4]]
    if not crossing:
        return []
    if len(crossing) == 2:
        pairs = [tuple(crossing)]
    else:                                     # inside corners on a diagonal: cut off each inside corner
        pairs = []
        for k in range(4):
            if ins[k]:
                pairs.append((edges[(k - 1) % 4], edges[k]))        # the two edges meeting at corner cyc[k]
    segs = []
    for (ea, eb) in pairs:
        ma, mb = edge_mid(ea), edge_mid(eb)
        d = [y - x for x, y in zip(ma, mb)]
        mid = [(x + y) / 2 for x, y in zip(ma, mb)]
        side = cross(n, d)
        sides = [dot(side, [c - m for c, m in zip(corner_pos(cc), mid)]) for cc in cyc]
        pos = [k for k in range(4) if sides[k] > 0]
        neg = [k for k in range(4) if sides[k] < 0]
        assert len(pos) + len(neg) == 4
        minority = pos if len(pos) <= len(neg) else neg
        k = minority[0]                        # a corner on the cut side (either side when the segment halves the face)
        corner_inside = ins[k]
        on_pos = sides[k] > 0
        # (n x d) must point away from the inside: an inside corner on the positive side means the segment is reversed
        if corner_inside == on_pos:
            ea, eb = eb, ea
        segs.append((ea, eb))
    return segs


def case_loops(case):
    inside = lambda c: bool((case >> c) & 1)
    nxt = {}
    for f in FACES:
        for (ea, eb) in face_segments(f, inside):
            assert ea not in nxt, (case, ea)
            nxt[ea] = eb
    crossing = sorted(e for e in range(12) if inside(corner_id(EDGES[e][1])) != inside(corner_id(EDGES[e][2])))
    assert sorted(nxt) == crossing and sorted(nxt.values()) == crossing, case
    loops, seen = [], set()
    for e in crossing:
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        loops.append(loop)
    return loops


def share_face(a, b):
    return any(a in f[4] and b in f[4] for f in FACES)


def fan_apex(loop):
    """the loop rotated to start at its lowest-id edge whose fan has no chord between two edges of one face"""
    n = len(loop)
    for e in sorted(loop):
        s = loop.index(e)
        r = loop[s:] + loop[:s]
        if not any(share_face(r[0], r[k]) for k in range(2, n - 1)):
            return r
    raise AssertionError(f"no fan apex for loop {loop}")


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        assert len(loop) >= 3
        loop = fan_apex(loop)
        for k in range(1, len(loop) - 1):
            tris.append((loop[0], loop[k], loop[k + 1]))
    return tris


def table():
    return [case_triangles(c) for c in range(256)]


def render():
    tab = table()
    assert max(len(t) for t in tab) <= 5
    lines = [
        "// enarf_mc_table.h - marching-cubes case table of libenarf_mesh.so. GENERATED by tools/gen_mc_table.py: do not edit.",
        "//",
        "// Case index: bit c = corner (dx, dy, dz), c = dx + 2 dy + 4 dz, inside (value > iso).",
        "// Edge ids: x-edges 0-3 at base (0, y, z) = y + 2 z; y-edges 4 + x + 2 z; z-edges 8 + x + 2 y.",
        "// ENARF_MC_NTRI[case] triangles; ENARF_MC_TRI[case][3 t + v] is vertex v of triangle t (an edge id), -1 past the end;",
        "// a case's 16 bytes are 16-byte aligned, so a kernel reads them with one load.",
        "// Face-consistent (four-crossing faces cut off their inside corners); (v1 - v0) x (v2 - v0) points inside -> outside;",
        "// no triangle has a chord between two edges of one face, so a face's neighbours never draw the same chord.",
        "#pragma once",
        "",
        "#ifndef ENARF_MC_TABLE_SPACE",
        "#define ENARF_MC_TABLE_SPACE",
        "#endif",
        "",
        "#define ENARF_MC_MAX_TRI 5",
        "",
        "static ENARF_MC_TABLE_SPACE const unsigned char ENARF_MC_NTRI[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(tab[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("")
    lines.append("static ENARF_MC_TABLE_SPACE const signed char ENARF_MC_TRI[256][16] __attribute__((aligned(16))) = {")
    for c in range(256):
        flat = [e for t in tab[c] for e in t]
        flat += [-1] * (16 - len(flat))
        lines.append("    {" + ", ".join(str(e) for e in flat) + "},  // " + str(c))
    lines.append("};")
    return "\n".join(lines) + "\n"


def main(argv):
    text = render()
    if "--check" in argv:
        with open(HEADER) as f:
            same = f.read() == text
        print("up to date" if same else f"{HEADER} differs from the generator's output")
        return 0 if same else 1
    if "--stdout" in argv:
        sys.stdout.write(text)
        return 0
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
