"""The loop body of the reference's train_ENARF_GAN.py around `TriNARFGenerator` and the discriminator:
`generator_loss` (its :80-99) and `train_step` (its :102-170, one GAN iteration on a batch). Everything stays on the
device: nothing here synchronises, calls `empty_cache`, prints or writes files.

Two things differ from the reference's text, both in the gradient accumulation. Its `loss()` zeroes the gradients
inside every micro-batch, so only the last micro-batch's gradient reaches the generator's optimiser; here they are
zeroed once, before the first micro-batch, and every micro-batch's loss is divided by `n_accum_step`: the step sees
the mean over the whole batch, at the gradient scale the reference's step has. And `real_img` is not switched to
`requires_grad` in place for R1: a detached alias of it is."""
from typing import Callable, Dict, Optional, Tuple

import torch

from ..libraries.gan.loss import adv_loss_dis, adv_loss_gen, d_r1_loss
from .loss import mask_guidance_loss

R1_EVERY = 16


def generator_loss(gen, dis, fake_img: torch.Tensor, fake_mask: torch.Tensor, bone_mask: torch.Tensor,
                   background_ratio: float, *, adv_loss_type: str, bone_guided_coef: float,
                   tri_plane_reg_coef: float = 0, bone_loss_func: Callable = mask_guidance_loss, ddp: bool = False,
                   world_size: int = 1) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """train_ENARF_GAN.py:80-99 without the optimisers: adversarial term + mask guidance * `bone_guided_coef`
    (+ the mean square of the tri-planes of the generator's last forward * `tri_plane_reg_coef` when that is > 0).
    Returns the loss and {"adv_loss_gen", "bone_loss"} (attached; `train_step` detaches them)."""
    loss_bone = bone_loss_func(fake_mask, bone_mask, background_ratio) * bone_guided_coef
    loss_adv_gen = adv_loss_gen(dis(fake_img, ddp, world_size), adv_loss_type, tmp=1)
    loss_gen = loss_adv_gen + loss_bone
    if tri_plane_reg_coef > 0:
        tri = gen.nerf.buffers_tensors["tri_plane_feature"]
        if tri is None:
            raise ValueError("tri_plane_reg_coef > 0 needs the tri-planes of the generator's forward; this route "
                             "does not keep them")
        loss_gen = loss_gen + tri.square().mean() * tri_plane_reg_coef
    return loss_gen, {"adv_loss_gen": loss_adv_gen, "bone_loss": loss_bone}


def _inv_intrinsics(batch: Dict[str, torch.Tensor]) -> torch.Tensor:
    if "inv_intrinsics" in batch:
        return batch["inv_intrinsics"]
    return torch.linalg.inv_ex(batch["intrinsics"])[0]           # inv_ex: no error check, so no synchronisation


def train_step(gen, dis, gen_optimizer, dis_optimizer, batch: Dict[str, torch.Tensor], real_img: torch.Tensor,
               iteration: int, *, n_accum_step: int, adv_loss_type: str, bone_guided_coef: float, r1_loss_coef: float,
               tri_plane_reg_coef: float = 0, bone_loss_func: Callable = mask_guidance_loss,
               z: Optional[torch.Tensor] = None, ddp: bool = False, world_size: int = 1
               ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """One iteration of train_ENARF_GAN.py:102-170 on a batch of device tensors (pose_to_camera, bone_length,
    bone_mask, intrinsics or inv_intrinsics, optionally pose_to_world): the generator phase in `n_accum_step`
    micro-batches of batchsize // n_accum_step frames with the discriminator's parameters frozen, one generator step,
    the discriminator step on the detached fakes of BEFORE that step and on `real_img`, and on every 16th iteration
    the lazy R1 step with the reference's `0 * dis_real[0]` term. `z` (batch, 4 * z_dim) fixes the latents (the step is
    then repeatable up to the renderer backward's float atomics); None samples them per micro-batch as the reference
    does. Returns (fake images (batch, 3, S, S), detached) and a dict of detached device scalars: "adv_loss_gen" and
    "bone_loss" (means over the micro-batches), "adv_loss_dis" and, when R1 ran, "r1_reg"."""
    pose_to_camera, bone_length, bone_mask = batch["pose_to_camera"], batch["bone_length"], batch["bone_mask"]
    pose_to_world = batch.get("pose_to_world")
    inv_intrinsics = _inv_intrinsics(batch)
    batchsize = pose_to_camera.shape[0]
    if n_accum_step < 1 or batchsize % n_accum_step:
        raise ValueError(f"a batch of {batchsize} does not divide into {n_accum_step} micro-batches")
    forward_bs = batchsize // n_accum_step
    latent = 4 * gen.config.z_dim
    if z is not None and tuple(z.shape) != (batchsize, latent):
        raise ValueError(f"z must be ({batchsize}, {latent}), got {tuple(z.shape)}")

    # ---- generator (:105-130)
    dis.requires_grad_(False)
    gen_optimizer.zero_grad(set_to_none=True)
    dis_optimizer.zero_grad(set_to_none=True)
    fakes, log = [], {"adv_loss_gen": 0, "bone_loss": 0}
    for i in range(0, batchsize, forward_bs):
        sl = slice(i, i + forward_bs)
        z_i = torch.randn(forward_bs, latent, device=pose_to_camera.device) if z is None else z[sl]
        fake_img_i, fake_mask_i, _, _ = gen(pose_to_camera[sl], None if pose_to_world is None else pose_to_world[sl],
                                            bone_length[sl], z_i, inv_intrinsics[sl])
        loss_gen, terms = generator_loss(gen, dis, fake_img_i, fake_mask_i, bone_mask[sl], gen.background_ratio,
                                         adv_loss_type=adv_loss_type, bone_guided_coef=bone_guided_coef,
                                         tri_plane_reg_coef=tri_plane_reg_coef, bone_loss_func=bone_loss_func, ddp=ddp,
                                         world_size=world_size)
        (loss_gen / n_accum_step).backward()
        fakes.append(fake_img_i.detach())
        for name, value in terms.items():
            log[name] = log[name] + value.detach() / n_accum_step
    fake_img = torch.cat(fakes)
    gen_optimizer.step()

    # ---- discriminator (:140-153)
    gen_optimizer.zero_grad(set_to_none=True)
    dis_optimizer.zero_grad(set_to_none=True)
    dis.requires_grad_(True)
    dis_fake = dis(fake_img, ddp, world_size)
    dis_real = dis(real_img, ddp, world_size)
    loss_dis = adv_loss_dis(dis_real, dis_fake, adv_loss_type)
    log["adv_loss_dis"] = loss_dis.detach()
    loss_dis.backward()
    dis_optimizer.step()

    # ---- lazy R1 (:155-169)
    if iteration % R1_EVERY == 0:
        gen_optimizer.zero_grad(set_to_none=True)
        dis_optimizer.zero_grad(set_to_none=True)
        real = real_img.detach().requires_grad_(True)
        dis_real = dis(real, ddp, world_size)
        r1_loss = d_r1_loss(dis_real, real)
        log["r1_reg"] = r1_loss.detach()
        (1 / 2 * r1_loss * R1_EVERY * r1_loss_coef + 0 * dis_real[0]).backward()     # 0 * dis_real[0] avoids zero grad
        dis_optimizer.step()
    return fake_img, log
