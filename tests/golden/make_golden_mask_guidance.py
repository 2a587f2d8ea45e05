"""Records tests/golden/mask_guidance.npz: inputs, loss values and autograd gradients of the reference's
`nerf_patch_loss` (models/loss.py, which imports with torch alone), evaluated in float64 on the CPU. Run once, with the
reference checkout on the path:

    python tests/golden/make_golden_mask_guidance.py /path/to/ENARF-GAN

Every case is recorded with coef 10 and an upstream gradient of 0.75. For each case the script ASSERTS how many values
equal to the selection threshold are left outside the selection, and whether that threshold is zero: `torch.topk` may
pick any of several equal values, so the reference's gradient is a function of the input only where the tied values
are all taken, or are zeros (whose gradient 2 m / k is zero whichever are picked). Only the case `quantised` has
non-zero ties left outside; its recorded gradient is therefore not stored, only its loss.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

COEF, UP = 10.0, 0.75
# case -> (ratio, values equal to the threshold left outside the selection, threshold is zero)
EXPECTED_TIES = {"uniform": (0.3, 0, False), "zeros60": (0.7, 0, False), "zeros80": (0.7, 410, True),
                 "four_d": (0.3, 0, False), "ratio0": (0.0, 0, False), "quantised": (0.3, 43, False),
                 "empty_bone": (0.3, 0, False), "k0": (0.1, 0, False)}


def ties_outside(mask: torch.Tensor, ratio: float):
    """(k, threshold, number of values equal to the threshold that the k smallest leave outside)"""
    flat = mask.reshape(-1).double()
    k = int(flat.numel() * ratio) if ratio > 0 else 0
    if k == 0:
        return k, None, 0
    low = flat.sort()[0][:k]
    thr = low[-1].item()
    return k, thr, int((flat == thr).sum()) - int((low == thr).sum())


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_models_loss", os.path.join(ref_root, "models", "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = torch.Generator().manual_seed(0)
    mask = torch.rand(2, 16, 16, generator=g)
    bone = (torch.rand(2, 32, 32, generator=g) > 0.9).float()
    z = torch.rand(4, 32, 32, generator=g)
    m60 = torch.where(torch.rand(4, 32, 32, generator=g) < 0.6, torch.zeros(()), z)
    bone1 = (torch.rand(4, 32, 32, generator=g) > 0.95).float()
    m80 = torch.where(torch.rand(4, 32, 32, generator=g) < 0.8, torch.zeros(()), z)
    bone16 = (torch.rand(2, 1, 16, 16, generator=g) > 0.9).float()
    cases = {
        "uniform": (mask, bone),                              # (2,16,16) against (2,32,32): pooled by 2
        "zeros60": (m60, bone1),                              # 60 % exact zeros, threshold above zero
        "zeros80": (m80, bone1),                              # 80 % exact zeros, threshold exactly zero
        "four_d": (mask[:, None], bone16),                    # 4-D pair at equal resolution
        "ratio0": (mask, bone),                               # no push term
        "quantised": ((mask * 8).floor() / 8, bone),          # eighths: ties at a non-zero threshold
        "empty_bone": (mask, torch.zeros(2, 32, 32)),         # NaN loss, NaN gradients
        "k0": (mask[:1, :2, :2], bone16[:1, 0, :2, :2] + torch.tensor([[1.0, 0.0], [0.0, 0.0]])),   # int(4 * 0.1) == 0
    }
    # the reference cannot pool a 4-D bone mask: 4-D exists at equal resolution only
    try:
        ref.nerf_patch_loss(mask[:, None].double(), bone[:, None].double(), 0.3, COEF)
        raise AssertionError("the reference pooled a 4-D bone mask")
    except (RuntimeError, ValueError, IndexError):
        pass
    out = {"coef": np.float64(COEF), "up": np.float64(UP), "cases": np.array(sorted(cases))}
    for name, (m, b) in cases.items():
        ratio, want_ties, want_zero = EXPECTED_TIES[name]
        k, thr, ties = ties_outside(m, ratio)
        assert ties == want_ties, (name, ties)
        assert (thr == 0.0) == want_zero, (name, thr)
        assert ties == 0 or thr == 0.0 or name == "quantised", (name, thr, ties)
        m64 = m.double().clone().requires_grad_(True)
        loss = ref.nerf_patch_loss(m64, b.double(), ratio, COEF)
        (UP * loss).backward()
        out[f"{name}_mask"] = m.numpy().astype(np.float32)
        out[f"{name}_bone"] = b.numpy().astype(np.float32)
        out[f"{name}_ratio"] = np.float64(ratio)
        out[f"{name}_k"] = np.int64(k)
        out[f"{name}_ties_outside"] = np.int64(ties)
        out[f"{name}_loss"] = np.float64(loss.item())
        if name != "quantised":
            out[f"{name}_d_mask"] = m64.grad.numpy()
        print(f"{name}: loss {loss.item()!r} k {k} threshold {thr} ties outside {ties} "
              f"gradient non-zeros {int((m64.grad != 0).sum())}")
    assert np.isnan(out["empty_bone_loss"]) and np.isnan(out["empty_bone_d_mask"]).all()
    assert np.isnan(out["k0_loss"]) and np.isfinite(out["k0_d_mask"]).all()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mask_guidance.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
