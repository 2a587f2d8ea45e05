"""The cases of libenarf_nmap.so on poisoned, guard-banded allocations, in the protocol of tests/poison_cases.py (that file
holds the rows of build.ALL_LIBRARIES and stays as it is; this row is build.LATE_LIBRARIES'): a case takes no arguments,
builds its inputs, snapshots them (poison_cases._begin), calls the public wrapper and returns (inputs, outputs, check).
POISON_CASES maps every launching function of include/enarf_nmap.h to its cases: one with every optional output, one bare.
tests/test_nmap_cpu.py requires the map and HOST_ONLY to account for every declared function; tests/test_gpu_nmap.py runs
the cases."""
import nmap_cases as NC
import nmap_reference as NR
from poison_cases import _GEO, _begin, _checked, _d, _hand_fragments

STEM = "nmap"

HOST_ONLY = {
    "enarf_nmap_abi_version": "returns a constant",
    "enarf_nmap_last_error": "returns the thread's message buffer",
}


def _encode(want_float):
    from enarf_gan_amd import ops
    from test_gpu_nmap import _check_encoded
    case = (5, 21)                                             # 441 texels: no multiple of 64; owners that name vertex V and -1
    (v, t), A = NC.mesh(case)
    face, vec = NC.texel_face(case), NC.vectors(case)
    inputs = _begin(dict(texel_face=_d(face), vectors=_d(vec), vertices=_d(v), triangles=_d(t)))
    res = ops.encode_normal_map(inputs["texel_face"], inputs["vectors"], inputs["vertices"], inputs["triangles"],
                                min_length=NC.MIN_LENGTH, want_float=want_float)
    out = {"texture": res.texture}
    if want_float:
        out["texture_f32"] = res.texture_f32
    else:
        assert res.texture_f32 is None

    def check(o):
        ref = NR.encode(face, vec, v, t, min_length=NC.MIN_LENGTH)
        _check_encoded(o["texture"].cpu().numpy(), o["texture_f32"].cpu().numpy() if want_float else None, ref, "hand mesh 21")
    return inputs, out, _checked(check)


def nmap_encode_with_float_texture():
    """nmap_encode_kernel on the five hand triangles in an atlas of 21 x 21, with the optional fp32 map"""
    return _encode(True)


def nmap_encode_bytes_only():
    return _encode(False)


def _shade(full):
    import bake_cases as BC
    from enarf_gan_amd import ops
    from test_gpu_nmap import _check_shaded
    h = _hand_fragments()                                      # 7 x 7 pixels: no multiple of 64
    normal_texture = NC.hand_normal_textures(16)[0 if full else 1]
    texture = BC.hand_textures(16)[1] if full else None
    kw = dict(lit=full, background=(0.1, 0.2, 0.3), base_color=(0.7, 0.6, 0.5))
    named = {**{k: _d(h[k]) for k in _GEO}, "normal_texture": _d(normal_texture)}
    if full:
        named["texture"] = _d(texture)
    inputs = _begin(named)
    res = ops.shade_normal_mapped(*(inputs[k] for k in _GEO), inputs["normal_texture"], texture=inputs.get("texture"), **kw)

    def check(o):
        ref = NR.shade(**{k: h[k] for k in _GEO}, normal_texture=normal_texture, texture=texture, **kw)
        _check_shaded({k: x.cpu().numpy() for k, x in o.items()}, ref, f"hand buffer, full={full}")
    return inputs, {k: getattr(res, k) for k in res._fields}, _checked(check)


def nmap_shade_lit_with_albedo_texture():
    """nmap_shade_kernel on the hand-written fragments: the RGBA8 normal map, an fp32 albedo texture, lit"""
    return _shade(True)


def nmap_shade_bare():
    """the fp32 normal map (a NaN, an inf, a zero cell), the constant base colour, not lit"""
    return _shade(False)


POISON_CASES = {
    "enarf_nmap_encode": ["nmap_encode_with_float_texture", "nmap_encode_bytes_only"],
    "enarf_nmap_shade": ["nmap_shade_lit_with_albedo_texture", "nmap_shade_bare"],
}

CASE_NAMES = sorted({c for cases in POISON_CASES.values() for c in cases})
