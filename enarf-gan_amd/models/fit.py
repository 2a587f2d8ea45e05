"""Fitting the pose of a posable field to a picture: `PoseCorrection`, per-frame residuals on the 24 joints' local rotations
and the root's translation, and `fit_pose`, Adam on one through `render_posable` and the photometric loss. The gradient
reaches the residuals through torch's own graph from the (B, P, 16) part records, whose gradient is the HIP kernel's
(ops.query_pose_bwd); nothing in the loop reads a value back from the device. `fit_scene` is the same loop for one picture
with K people in it, through `render_scene_posable`: the avatars are composed depth-correctly and the composite's own
gradient is a HIP kernel as well (ops.scene_composite_bwd)."""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from .. import ops
from ..libraries.NeRF.ray_sampler import mask_based_sampler
from ..libraries.NeRF.rendering import render_posable


def axis_angle_rotation(r: torch.Tensor) -> torch.Tensor:
    """(..., 3) axis-angle vectors -> (..., 3, 3) rotations by Rodrigues' formula, I + a K + b K^2 with a = sin t / t and
    b = (1 - cos t) / t^2 (their series below t^2 = 1e-8, so the zero vector gives the identity exactly and a finite
    gradient)."""
    t2 = (r * r).sum(dim=-1)
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)
    t = torch.sqrt(t2s)
    a = torch.where(small, 1 - t2 / 6, torch.sin(t) / t)
    b = torch.where(small, 0.5 - t2 / 24, (1 - torch.cos(t)) / t2s)
    x, y, z = r.unbind(dim=-1)
    o = torch.zeros_like(x)
    K = torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=-1).reshape(r.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=r.dtype, device=r.device)
    return eye + a[..., None, None] * K + b[..., None, None] * (K @ K)


def rigid_inverse(T: torch.Tensor) -> torch.Tensor:
    """(..., 4, 4) rigid transforms [R t; 0 1] -> their inverses [R^T  -R^T t; 0 1]"""
    Rt = T[..., :3, :3].transpose(-1, -2)
    top = torch.cat([Rt, -(Rt @ T[..., :3, 3:])], dim=-1)
    return torch.cat([top, T[..., 3:, :]], dim=-2)


class PoseCorrection(nn.Module):
    """Residuals of F frames of 24-joint poses: `rotation` (F, J, 3) axis-angle vectors applied on the right of every
    joint's local rotation (its rotation relative to its parent; the root's relative to the camera) and `translation`
    (F, 3) added to the root's position, all zero at the start. forward() splits the global joint transforms into local
    ones over `parents`, applies the residuals and recomposes the global transforms by forward kinematics, in plain torch:
    a residual at a joint turns that joint and carries its descendants, and leaves every other joint's transform bit for
    bit as zero residuals give it. Zero residuals reproduce the input to fp32 rounding. Poses are taken to be rigid (the
    inverse of a parent's transform is formed from the transpose of its rotation)."""

    def __init__(self, num_frames: int, parents: Sequence[int], num_joints: int = 24):
        super().__init__()
        par = [int(p) for p in np.asarray(parents).reshape(-1)[:num_joints]]
        if len(par) != num_joints or any(not (0 <= par[j] < j) for j in range(1, num_joints)):
            raise ValueError(f"parents must list {num_joints} joints, each after its parent, the root first, got {par}")
        self.parents = par
        self.rotation = nn.Parameter(torch.zeros(num_frames, num_joints, 3))
        self.translation = nn.Parameter(torch.zeros(num_frames, 3))

    def forward(self, pose_to_camera: torch.Tensor, frame_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pose_to_camera (B, J, 4, 4); frame_idx (B,) int64 names each image's frame (default: image b is frame b)"""
        B, J = pose_to_camera.shape[:2]
        if J != len(self.parents) or pose_to_camera.shape[2:] != (4, 4):
            raise ValueError(f"PoseCorrection takes (B, {len(self.parents)}, 4, 4) poses, got {tuple(pose_to_camera.shape)}")
        if frame_idx is None:
            if B != self.rotation.shape[0]:
                raise ValueError(f"{B} poses for {self.rotation.shape[0]} frames: pass frame_idx")
            rot, trans = self.rotation, self.translation
        else:
            rot, trans = self.rotation[frame_idx], self.translation[frame_idx]
        par = torch.as_tensor(self.parents[1:], device=pose_to_camera.device)
        local = rigid_inverse(pose_to_camera[:, par]) @ pose_to_camera[:, 1:]          # (B, J - 1, 4, 4)
        D = torch.zeros(B, J, 4, 4, dtype=pose_to_camera.dtype, device=pose_to_camera.device)
        D[:, :, :3, :3] = axis_angle_rotation(rot).to(pose_to_camera.dtype)
        D[:, :, 3, 3] = 1
        shift = torch.zeros_like(pose_to_camera[:, 0])
        shift[:, :3, 3] = trans.to(pose_to_camera.dtype)
        out = [(pose_to_camera[:, 0] + shift) @ D[:, 0]]
        for j in range(1, J):
            out.append(out[self.parents[j]] @ local[:, j - 1] @ D[:, j])
        return torch.stack(out, dim=1)


def fit_pose(gen, target_img: torch.Tensor, target_mask: torch.Tensor, pose_to_camera: torch.Tensor,
             bone_length: torch.Tensor, z, inv_intrinsics: torch.Tensor, steps: int = 100, lr: float = 1e-2,
             n_rays: int = 1024, Nc: Optional[int] = None, Nf: Optional[int] = None, background: float = -1.0,
             loss_type: str = "mse", seed: int = 0, correction: Optional[PoseCorrection] = None,
             truncation_psi: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fit the 24-joint poses pose_to_camera (B, 24, 4, 4) of a trained field to pictures: Adam on a PoseCorrection (one
    frame an image), `steps` steps of: n_rays rays by mask_based_sampler on target_mask (B, S, S), render_posable over
    `background`, ops.photometric_loss against target_img (B, 3, S, S) and target_mask. gen: a generator shell (its
    `.nerf` is used, Nc / Nf default to its configuration) or a TriPlaneNARF; z: the latent, one tensor (tri-plane and
    rendering latent alike, as the single-scene generator has them) or a pair (z, z_rend); inv_intrinsics in pixels. The
    field is held fixed (its parameters receive no gradient) and its tri-plane is produced once. The importance samples
    of step i are drawn with seed + i. No host synchronisation inside the loop. Returns (the fitted poses (B, 24, 4, 4),
    detached, and the loss of every step (steps,) as a device tensor)."""
    nerf = getattr(gen, "nerf", gen)
    samples = getattr(gen, "_samples", {}) if nerf is not gen else {}
    Nc = int(Nc if Nc is not None else samples.get("Nc", nerf.config.Nc))
    Nf = int(Nf if Nf is not None else samples.get("Nf", nerf.config.Nf))
    z_tri, z_rend = z if isinstance(z, (tuple, list)) else (z, z)
    B = pose_to_camera.shape[0]
    dev = pose_to_camera.device
    if correction is None:
        correction = PoseCorrection(B, nerf.parent_id, pose_to_camera.shape[1]).to(dev)
    optimizer = torch.optim.Adam(correction.parameters(), lr=lr)
    history = torch.zeros(steps, dtype=torch.float32, device=dev)
    frozen = [p for p in nerf.parameters() if p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    try:
        tri = None
        if not (nerf.uses_warp or nerf.constant_trimask):          # those producers emit their planes inside the render
            with torch.no_grad():
                tri = nerf.compute_tri_plane_feature(z_tri, nerf.transform_pose(pose_to_camera, bone_length)[1], truncation_psi)
        for i in range(steps):
            optimizer.zero_grad()
            ray_idx, pixels = mask_based_sampler(target_mask, n_rays)
            pose_parts, bl_parts = nerf.transform_pose(correction(pose_to_camera), bone_length)
            mi = {"z": z_tri, "z_rend": z_rend, "bone_length": bl_parts, "truncation_psi": truncation_psi}
            if tri is not None:
                mi["tri_plane_feature"] = tri
            color, mask, _ = render_posable(nerf, pixels, pose_parts, inv_intrinsics, Nc=Nc, Nf=Nf, model_input=mi, seed=seed + i)
            color = color + background * (1 - mask[:, None])
            loss_color, loss_mask = ops.photometric_loss(ray_idx, color, mask, target_img, target_mask, loss_type)
            loss = loss_color + loss_mask
            history[i] = loss.detach()
            loss.backward()
            optimizer.step()
    finally:
        for p in frozen:
            p.requires_grad_(True)
    with torch.no_grad():
        return correction(pose_to_camera).detach(), history


def fit_scene(gen, target_img: torch.Tensor, target_mask: torch.Tensor, pose_to_camera: torch.Tensor,
              bone_length: torch.Tensor, z, inv_intrinsics: torch.Tensor, steps: int = 100, lr: float = 1e-2,
              n_rays: int = 1024, Nc: Optional[int] = None, Nf: Optional[int] = None, background: float = -1.0,
              loss_type: str = "mse", seed: int = 0, correction: Optional[PoseCorrection] = None,
              target_instance: Optional[torch.Tensor] = None, instance_weight: float = 1.0,
              truncation_psi: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """fit_pose for one picture with K people in it: the 24-joint poses pose_to_camera (K, 24, 4, 4) of K avatars of a
    trained field (bone_length and z of batch K, z as fit_pose takes it) are fitted to target_img (1, 3, S, S) and
    target_mask (1, S, S), the mask of the whole scene. Adam on one PoseCorrection(K, ...) (one frame an avatar), `steps`
    steps of: n_rays rays by mask_based_sampler on target_mask, render_scene_posable over `background` (the K avatars
    composed depth-correctly, each one's gradient through the HIP backward of the composite), ops.photometric_loss.
    Where target_instance (1, S, S) is given (the avatar that owns each pixel, -1 for none), instance_weight times the
    mean squared difference between instance_mass[k] and (target_instance == k) on the sampled rays is added, in torch.
    The field is held fixed and its tri-planes are produced once per avatar. The importance samples of step i are drawn
    with seed + i. No host synchronisation inside the loop. Returns (the fitted poses (K, 24, 4, 4), detached, and the
    loss of every step (steps,) as a device tensor)."""
    from ..libraries.NeRF.rendering import render_scene_posable
    nerf = getattr(gen, "nerf", gen)
    samples = getattr(gen, "_samples", {}) if nerf is not gen else {}
    Nc = int(Nc if Nc is not None else samples.get("Nc", nerf.config.Nc))
    Nf = int(Nf if Nf is not None else samples.get("Nf", nerf.config.Nf))
    z_tri, z_rend = z if isinstance(z, (tuple, list)) else (z, z)
    K = pose_to_camera.shape[0]
    dev = pose_to_camera.device
    if target_img.shape[0] != 1 or target_mask.shape[0] != 1:
        raise ValueError(f"fit_scene takes one picture: target_img (1, 3, S, S) and target_mask (1, S, S), got "
                         f"{tuple(target_img.shape)} and {tuple(target_mask.shape)}")
    if correction is None:
        correction = PoseCorrection(K, nerf.parent_id, pose_to_camera.shape[1]).to(dev)
    owner = None
    if target_instance is not None:
        owner = target_instance.reshape(1, -1).to(dev)
        ids = torch.arange(K, device=dev)[None, :, None]
    optimizer = torch.optim.Adam(correction.parameters(), lr=lr)
    history = torch.zeros(steps, dtype=torch.float32, device=dev)
    frozen = [p for p in nerf.parameters() if p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    try:
        tri = None
        if not (nerf.uses_warp or nerf.constant_trimask):          # those producers emit their planes inside the render
            with torch.no_grad():
                tri = nerf.compute_tri_plane_feature(z_tri, nerf.transform_pose(pose_to_camera, bone_length)[1], truncation_psi)
        for i in range(steps):
            optimizer.zero_grad()
            ray_idx, pixels = mask_based_sampler(target_mask, n_rays)
            pose_parts, bl_parts = nerf.transform_pose(correction(pose_to_camera), bone_length)
            mi = {"z": z_tri, "z_rend": z_rend, "bone_length": bl_parts, "truncation_psi": truncation_psi}
            if tri is not None:
                mi["tri_plane_feature"] = tri
            color, mask, _ = render_scene_posable(nerf, pixels, pose_parts, inv_intrinsics, Nc=Nc, Nf=Nf, model_input=mi,
                                                  seed=seed + i)
            color = color + background * (1 - mask[:, None])
            loss_color, loss_mask = ops.photometric_loss(ray_idx, color, mask, target_img, target_mask, loss_type)
            loss = loss_color + loss_mask
            if owner is not None:
                wanted = (torch.gather(owner, 1, ray_idx)[:, None] == ids).to(torch.float32)           # (1, K, n)
                loss = loss + instance_weight * ((nerf.buffers_tensors["instance_mass"] - wanted) ** 2).mean()
            history[i] = loss.detach()
            loss.backward()
            optimizer.step()
    finally:
        for p in frozen:
            p.requires_grad_(True)
    with torch.no_grad():
        return correction(pose_to_camera).detach(), history
