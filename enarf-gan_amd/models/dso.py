"""The two loop bodies of the reference's train_DSO.py around `DSONARFGenerator`: `train_step` (its :240-258, one
optimisation step on a batch) and `validate` (its :74-158 without the image file and without DDP). Both leave their
results on the device; `validate` synchronises once, when it has scored every image."""
from typing import Dict, Iterable, Optional, Sequence

import torch

from ..libraries import metrics

_METRIC_COLUMN = {"SSIM": 0, "PSNR": 2}


def _unpack(batch: Dict[str, torch.Tensor]):
    return (batch["img"], batch["mask"], batch["pose_3d"], batch["frame_time"], batch["bone_length"],
            batch.get("camera_rotation"), torch.inverse(batch["intrinsics"]))


def train_step(gen, loss_func, batch: Dict[str, torch.Tensor], optimizer, bg_color: float):
    """One step of train_DSO.py:240-258 on a batch of device tensors (img, mask, pose_3d, frame_time, bone_length,
    camera_rotation, intrinsics): sample rays by the mask, render them over `bg_color`, photometric loss, backward,
    optimiser step. Returns (loss_color, loss_mask) as detached device scalars - nothing here synchronises."""
    gen.train()
    img, mask, pose_to_camera, frame_time, bone_length, camera_rotation, inv_intrinsic = _unpack(batch)
    optimizer.zero_grad()
    nerf_color, nerf_mask, grid = gen(pose_to_camera, camera_rotation, mask, frame_time, bone_length, inv_intrinsic,
                                      background=bg_color)
    loss_color, loss_mask = loss_func(grid, nerf_color, nerf_mask, img, mask)
    (loss_color + loss_mask).backward()
    optimizer.step()
    return loss_color.detach(), loss_mask.detach()


def train_step_posable(gen, loss_func, batch: Dict[str, torch.Tensor], optimizer, bg_color: float, correction,
                       pose_optimizer):
    """train_step with the poses of the sequence refined while the scene is learned: the batch's 24-joint poses pass
    through `correction` (models.fit.PoseCorrection; batch["frame_idx"] (B,) int64 names each image's frame, default
    image b = frame b) and the rays are rendered by render_posable, whose gradient reaches the correction's residuals as
    well as the field's parameters; `optimizer` steps the field, `pose_optimizer` the correction. The latents are formed
    from the poses as given (a pose-conditional latent does not see the correction). The gradient is that of the image
    at fixed sample positions (render_posable). Returns (loss_color, loss_mask) as detached device scalars - nothing here
    synchronises."""
    from ..libraries.NeRF.rendering import render_posable
    gen.train()
    img, mask, pose_to_camera, frame_time, bone_length, _camera_rotation, inv_intrinsic = _unpack(batch)
    optimizer.zero_grad()
    pose_optimizer.zero_grad()
    ray_idx, pixels = gen.ray_sampler(mask, gen.config.ray_batchsize)
    z_tri, z_render = gen.get_latents(frame_time, pose_to_camera)
    pose_parts, bl_parts = gen.nerf.transform_pose(correction(pose_to_camera, batch.get("frame_idx")), bone_length)
    model_input = {"z": z_tri, "z_rend": z_render, "bone_length": bl_parts, "truncation_psi": 1}
    color, alpha, _ = render_posable(gen.nerf, pixels, pose_parts, inv_intrinsic, model_input=model_input, **gen._samples)
    nerf_color = color + bg_color * (1 - alpha[:, None])
    loss_color, loss_mask = loss_func(ray_idx, nerf_color, alpha, img, mask)
    (loss_color + loss_mask).backward()
    optimizer.step()
    pose_optimizer.step()
    return loss_color.detach(), loss_mask.detach()


def _mask_bbox(mask: torch.Tensor):
    """train_DSO.py:108-119: (x_min, y_min, x_max, y_max) of the first and last foreground column / row (the last ones
    are left out of the slices, as there), or None for an empty mask. Reads the mask back: cropping needs host sizes."""
    cols, rows = torch.where(mask.any(dim=0))[0], torch.where(mask.any(dim=1))[0]
    if len(cols) == 0 or len(rows) == 0:
        return None
    return int(cols[0]), int(rows[0]), int(cols[-1]), int(rows[-1])


def validate(gen, batches: Iterable[Dict[str, torch.Tensor]], size: int, bg_color: float,
             metric: Sequence[str] = ("SSIM", "PSNR"), crop: bool = False, num_data: Optional[int] = None
             ) -> Dict[str, float]:
    """One validation set of train_DSO.py:74-158: every batch (one image each, device tensors as for `train_step`) is
    rendered whole with `render_entire_img`, composed over `bg_color` and scored against the real frame; returns
    {"color": mean MSE, "mask": mean mask MSE, "color_<metric>": mean metric} over the images, as Python floats.
    With `crop` the score is taken over the bounding box of the real mask (the frame is read in place; an image with an
    empty mask is skipped but still counted, as in the reference). Per-image results stay on the device."""
    bad = [m for m in metric if m not in _METRIC_COLUMN]
    if bad:
        if "LPIPS" in bad:
            metrics.lpips(None, None)                 # raises ImportError, as the reference does without the package
        raise ValueError(f"metric must name only {sorted(_METRIC_COLUMN)} or LPIPS, got {bad}")
    gen.eval()
    rows, count = [], 0
    with torch.no_grad():
        for i, batch in enumerate(batches):
            if num_data is not None and i >= num_data:
                break
            count += 1
            img, mask, pose_to_camera, frame_time, bone_length, camera_rotation, inv_intrinsic = _unpack(batch)
            bbox = None
            if crop:
                bbox = _mask_bbox(mask[0])
                if bbox is None:
                    continue
            gen_color, gen_mask, _ = gen.render_entire_img(pose_to_camera, inv_intrinsic, frame_time, bone_length,
                                                           camera_rotation, size, bbox=bbox)
            gen_color, gen_mask = gen_color[None], gen_mask[None]
            gen_color = gen_color + bg_color * (1 - gen_mask)
            rows.append(metrics.image_metrics(img[:1], gen_color, mask[:1], gen_mask, bbox=bbox))
    total = torch.cat(rows).double().sum(0).cpu() if rows else torch.zeros(4, dtype=torch.float64)   # the one sync
    n = max(count, 1)
    out = {"color": float(total[1]) / n, "mask": float(total[3]) / n}
    for m in metric:
        out[f"color_{m}"] = float(total[_METRIC_COLUMN[m]]) / n
    return out
