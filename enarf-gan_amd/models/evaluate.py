"""Evaluation loops on the device. `inverse_depth_error` is the loop of the reference's evaluation/compute_depth.py:22-77
- the paper's 3-D metric: the mean squared error between the generator's disparity and a ground-truth inverse-depth map
over poses drawn from the depth dataset - with the running sums kept on the device (ops.DepthError) instead of a
`.cpu()` per batch and one MSELoss over the whole set on the host."""
import torch

from .. import ops


def _accumulate(gen, batches, num_sample, truncation_psi, error, z_dim, dev, generator):
    """marches the batches into `error` until num_sample samples are in; how many went in"""
    seen, S = 0, gen.size
    for batch in batches:
        take = min(len(batch["pose_3d"]), num_sample - seen)
        on = lambda k: batch[k][:take].to(dev, non_blocking=True)
        pose, bone_length, world, K, target = on("pose_3d"), on("bone_length"), on("pose_3d_world"), on("intrinsics"), on("img")
        z = torch.randn(take, z_dim, device=dev, generator=generator)
        _, mask, disparity = gen(pose.float(), world, bone_length.float(), z, torch.linalg.inv_ex(K.float()).inverse,
                                 return_disparity=True, truncation_psi=truncation_psi)
        error.update(disparity.reshape(take, S, S).float().contiguous(), target.reshape(take, S, S).float().contiguous(),
                     mask.reshape(take, S, S).float().contiguous())
        seen += take
        if seen >= num_sample:
            break
    return seen


@torch.no_grad()
def inverse_depth_error(gen, batches, num_sample, truncation_psi=1, mask_threshold=0.5, generator=None):
    """The depth error of `gen` (a TriNARFGenerator) over the first `num_sample` samples of `batches`, an iterable of
    dicts with pose_3d (B, J, 4, 4), pose_3d_world, bone_length, intrinsics (B, 3, 3) and img (B, S, S) - the ground-truth
    inverse depth, 0 on background - as SurrealPoseDepthDataset yields them. A latent is drawn per sample from torch's
    generator (`generator`, or the device's default one), the march returns disparity and mask, and both go into the
    running error; there is no host synchronisation inside the loop and one host read at its end. Returns
    DepthError.result(): `inv_depth_mse` is the reference's number, `inv_depth_mse_fg` the same over the ground truth's
    foreground, `iou` the overlap of the generated and the true silhouette. The batches' last one is cut to num_sample;
    fewer samples than num_sample raise ValueError. The generator runs in train mode, as in the reference, and is put
    back into the mode it came in."""
    if num_sample < 1:
        raise ValueError(f"inverse_depth_error: num_sample {num_sample} < 1")
    dev = next(gen.parameters()).device
    z_dim = gen.config.z_dim * (3 if gen.black_background else 4)
    error = ops.DepthError(mask_threshold)
    was_training = gen.training
    gen.train()                                      # compute_depth.py:34: no fixed cropping of the background
    try:
        seen = _accumulate(gen, batches, num_sample, truncation_psi, error, z_dim, dev, generator)
    finally:
        gen.train(was_training)
    if seen < num_sample:
        raise ValueError(f"inverse_depth_error: the batches hold {seen} samples, {num_sample} asked for")
    return error.result()
