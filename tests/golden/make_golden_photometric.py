"""Records tests/golden/photometric.npz: inputs, loss values and autograd gradients of the reference's PhotometricLoss
(libraries/NeRF/loss.py), evaluated in float64 on the CPU. Run once, with the reference checkout on the path:

    python tests/golden/make_golden_photometric.py /path/to/ENARF-GAN

Cases: both loss types, with and without the real mask, B in {1, 3}, N not a multiple of 64, duplicated ray ids; the
rendered values keep |t - s| away from the truncated MAE's threshold (0.01) by at least 1e-3.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_nerf_loss", os.path.join(ref_root, "libraries", "NeRF", "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20240612)
    out = {}
    for B, S, N in ((1, 16, 200), (3, 32, 333)):
        color = rng.uniform(-1, 1, (B, 3, S, S)).astype(np.float32)
        mask = (rng.uniform(0, 1, (B, S, S)) > 0.5).astype(np.float32)
        mask[:, ::5] = rng.uniform(0, 1, mask[:, ::5].shape).astype(np.float32)      # non-binary values too
        grid = rng.integers(0, S * S, (B, N))
        grid[:, 1::7] = grid[:, 0:-1:7][:, :grid[:, 1::7].shape[1]]                  # duplicated ids
        flat = color.reshape(B, 3, -1)
        target = np.take_along_axis(flat, np.repeat(grid[:, None], 3, 1), 2)
        delta = rng.uniform(-0.5, 0.5, (B, 3, N))
        small = rng.uniform(0, 1, delta.shape) < 0.3                                  # a share below the threshold
        delta = np.where(small, rng.uniform(-0.009, 0.009, delta.shape), np.sign(delta) * (np.abs(delta) + 0.011))
        sparse_color = (target + delta).astype(np.float32)
        sparse_mask = rng.uniform(0, 1, (B, N)).astype(np.float32)
        tag = f"b{B}"
        out.update({f"{tag}_color": color, f"{tag}_mask": mask, f"{tag}_grid": grid.astype(np.int64),
                    f"{tag}_sparse_color": sparse_color, f"{tag}_sparse_mask": sparse_mask})
        margin = np.abs(np.abs(target.astype(np.float64) - sparse_color.astype(np.float64)) - 0.01).min()
        assert margin > 1e-3, margin
        for loss_type in ("mse", "mae"):
            for with_mask in (True, False):
                cfg = types.SimpleNamespace(nerf_loss_type=loss_type, color_coef=1.7, mask_coef=0.6)
                sc = torch.tensor(sparse_color, dtype=torch.float64, requires_grad=True)
                sm = torch.tensor(sparse_mask, dtype=torch.float64, requires_grad=True)
                lc, lm = ref.PhotometricLoss(cfg)(torch.from_numpy(grid), sc, sm, torch.tensor(color, dtype=torch.float64),
                                                  torch.tensor(mask, dtype=torch.float64) if with_mask else None)
                (0.75 * lc + 1.25 * lm).backward()                                   # upstream gradients 0.75, 1.25
                key = f"{tag}_{loss_type}_{'mask' if with_mask else 'nomask'}"
                out[key + "_loss_color"] = np.float64(lc.item())
                out[key + "_loss_mask"] = np.float64(float(lm))
                out[key + "_d_sparse_color"] = sc.grad.numpy()
                if with_mask:
                    out[key + "_d_sparse_mask"] = sm.grad.numpy()
                else:
                    assert sm.grad is None and lm == 0
    out["color_coef"], out["mask_coef"] = np.float64(1.7), np.float64(0.6)
    out["g_color"], out["g_mask"] = np.float64(0.75), np.float64(1.25)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "photometric.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
