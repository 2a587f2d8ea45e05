"""Float64 numpy restatement of the mask-guidance loss as include/enarf_guide.h states it: the referee of
tests/test_mask_guidance_cpu.py and tests/test_gpu_mask_guidance.py. Nothing here is shared with the kernels.

    on-bone   bone_mask max-pooled by rate = S // s (stride rate, no padding, remainder dropped), > 0.5
    bone      mean of (1 - m)^2 over the on-bone pixels                                (NaN for none)
    push      mean of the squares of the k = int(N * ratio) smallest values (NaN for k == 0), left out for ratio <= 0;
              values are ordered by their fp32 bit image (NaN largest, -0 below +0) and, among equal ones, by flat index
    loss      (push + bone) * coef
    d m_i     up * coef * (2 m_i / k [i selected] - 2 (1 - m_i) / n_bone [i on the bone])
"""
import numpy as np


def key(mask32: np.ndarray) -> np.ndarray:
    """order-preserving uint32 image of fp32 values: NaN -> 0xFFFFFFFF, negative -> ~bits, else bits | 0x80000000"""
    bits = np.ascontiguousarray(mask32, dtype=np.float32).view(np.uint32)
    out = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    out[np.isnan(mask32)] = np.uint32(0xFFFFFFFF)
    return out


def pooled_on_bone(bone_mask: np.ndarray, shape) -> np.ndarray:
    """boolean on-bone map of `shape` (the mask's)"""
    bone_mask = np.asarray(bone_mask)
    if bone_mask.shape == tuple(shape):
        return bone_mask > 0.5
    if bone_mask.ndim != 3 or len(shape) != 3 or bone_mask.shape[0] != shape[0] or bone_mask.shape[1] != bone_mask.shape[2] \
            or shape[1] != shape[2]:
        raise ValueError(f"bone mask {bone_mask.shape} against mask {tuple(shape)}")
    B, s, S = shape[0], shape[-1], bone_mask.shape[-1]
    rate = S // s
    if rate < 1 or S // rate != s:
        raise ValueError(f"a {S} x {S} bone mask does not pool to {s} x {s}")
    win = bone_mask[:, :s * rate, :s * rate].reshape(B, s, rate, s, rate)
    with np.errstate(invalid="ignore"):
        return win.max(axis=(2, 4)) > 0.5                 # np.max propagates NaN, and NaN > 0.5 is False


def selection(mask: np.ndarray, ratio: float):
    """(k, boolean map of the selected values) - the k smallest by (key, flat index); (0, nothing) for ratio <= 0"""
    flat = np.asarray(mask, dtype=np.float32).reshape(-1)
    sel = np.zeros(flat.size, dtype=bool)
    if ratio <= 0:
        return 0, sel.reshape(np.shape(mask))
    k = int(flat.size * ratio)
    if k > flat.size:
        raise ValueError(f"ratio {ratio} selects more values than there are")
    order = np.argsort(key(flat), kind="stable")          # stable: equal keys stay in index order
    sel[order[:k]] = True
    return k, sel.reshape(np.shape(mask))


def terms(mask, bone_mask, ratio: float):
    """(push, bone) in float64; push is 0.0 for ratio <= 0"""
    m = np.asarray(mask, dtype=np.float32).astype(np.float64)
    on = pooled_on_bone(bone_mask, m.shape)
    k, sel = selection(mask, ratio)
    with np.errstate(invalid="ignore", divide="ignore"):
        push = np.float64(0.0) if ratio <= 0 else np.square(m[sel]).sum() / np.float64(k)
        bone = np.square(1.0 - m[on]).sum() / np.float64(on.sum())
    return float(push), float(bone)


def loss(mask, bone_mask, ratio: float = 0.3, coef: float = 10.0) -> float:
    push, bone = terms(mask, bone_mask, ratio)
    return (push + bone) * coef


def loss_grad(mask, bone_mask, ratio: float = 0.3, coef: float = 10.0, up: float = 1.0) -> np.ndarray:
    """d loss / d mask * up, float64, the mask's shape"""
    m = np.asarray(mask, dtype=np.float32).astype(np.float64)
    on = pooled_on_bone(bone_mask, m.shape)
    k, sel = selection(mask, ratio)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.float64(up) * coef * 2.0
        d_push = np.where(sel, g / np.float64(max(k, 1)) * m, 0.0)
        d_bone = (g / np.float64(on.sum())) * -(1.0 - m) * on.astype(np.float64)     # n_bone == 0: NaN everywhere
    return d_push + d_bone
