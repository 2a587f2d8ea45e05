"""GPU tests of the GAN supervision (libenarf_guide.so): the mask-guidance loss, its two terms and its gradient against
the float64 referee of tests/mask_guidance_reference.py (never a kernel) and the reference's recorded values.

Bounds. The loss, a term or a gradient element is one fp64 expression over <= 2^20 terms (relative error <= 2^20 * 2^-53
= 2^-33, as the referee's) rounded to fp32 once: it lies within one fp32 ulp of the referee, |out - ref| <= 2^-23 |ref|
(ULP below), the same argument as for the photometric loss. Against the torch functions of models/loss.py in fp32 no
tolerance is set: torch-fp32's own distance from the referee is measured on the same inputs and the HIP result must be
no further away. `torch.autograd.gradcheck` does not apply in fp32; the per-element comparison is the check.
Measured on the MI355X over the cases below: every figure equals the referee rounded to fp32 bit for bit (largest
deviation 0); torch's fp32 functions sit up to 4.2e-7 (loss) and 6.9e-10 (gradient element) from the referee.
"""
import numpy as np
import pytest
import torch

import mask_guidance_reference as R
from test_mask_guidance_cpu import golden

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
COEF, UP = 10.0, 0.75                 # upstream gradient exact in fp32


def _within_ulp(out, ref, what):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert np.array_equal(np.isnan(out), np.isnan(ref)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(ref)
    ref32 = ref.astype(np.float32).astype(np.float64)              # the referee rounded to fp32
    err = np.abs(out[ok] - ref32[ok])
    tol = ULP * np.abs(ref32[ok]) + 1e-44                          # + the smallest fp32 subnormal
    worst = float((err / np.maximum(np.abs(ref32[ok]), 1e-300)).max()) if err.size else 0.0
    print(f"{what}: max relative deviation {worst:.3e} (bound {ULP:.3e})")
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} values beyond one fp32 ulp, worst {worst:.3e}"
    return worst


def _run(mask, bone, ratio, coef=COEF, up=UP, via_model=False):
    from enarf_gan_amd import ops
    from enarf_gan_amd.models.loss import mask_guidance_loss
    m = torch.as_tensor(mask).cuda().requires_grad_()
    b = torch.as_tensor(bone).cuda()
    if via_model:
        loss, push, bone_term = mask_guidance_loss(m, b, ratio, coef), None, None
    else:
        loss, push, bone_term = ops.mask_guidance_loss(m, b, ratio, coef, return_terms=True)
        assert not push.requires_grad and not bone_term.requires_grad
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    (up * loss).backward()
    assert m.grad.shape == m.shape and m.grad.dtype == torch.float32
    return loss, push, bone_term, m.grad


def _check(mask, bone, ratio, what, coef=COEF, up=UP):
    loss, push, bone_term, grad = _run(mask, bone, ratio, coef, up)
    r_push, r_bone = R.terms(mask, bone, ratio)
    _within_ulp(loss.item(), R.loss(mask, bone, ratio, coef), f"{what} loss")
    _within_ulp(push.item(), r_push, f"{what} push")
    _within_ulp(bone_term.item(), r_bone, f"{what} bone")
    _within_ulp(grad.cpu().numpy(), R.loss_grad(mask, bone, ratio, coef, up), f"{what} d fake_mask")
    return loss, grad


def _carries_push(mask, bone, ratio, grad):
    """flat boolean map of the elements whose gradient holds a push term: the bone term alone is the gradient at ratio 0
    (a push term of a non-zero eighth is >= 2 * 0.75 * 10 * 0.125 / k, orders above the four ulp allowed here)"""
    bone_only = R.loss_grad(mask, bone, 0.0, COEF, UP)
    return (np.abs(grad.cpu().numpy().astype(np.float64) - bone_only) > 4 * ULP * np.abs(bone_only)).reshape(-1)


def test_fixture_cases_match_reference_and_referee():
    """every recorded case: loss, both terms and gradient against the referee; loss and gradient against the reference's
    recorded float64 values, element by element - but for `quantised`, whose values tied at a non-zero threshold stay
    partly outside: there the reference's gradient is not a function of the input, and the tie rule's invariants stand in"""
    g = golden()
    assert float(g["coef"]) == COEF and float(g["up"]) == UP
    for name in [str(n) for n in g["cases"]]:
        mask, bone, ratio = g[f"{name}_mask"], g[f"{name}_bone"], float(g[f"{name}_ratio"])
        loss, grad = _check(mask, bone, ratio, name)
        _within_ulp(loss.item(), g[f"{name}_loss"], f"{name} loss against the reference")
        if name != "quantised":
            _within_ulp(grad.cpu().numpy(), g[f"{name}_d_mask"], f"{name} d fake_mask against the reference")
            continue
        k, flat = int(g[f"{name}_k"]), mask.reshape(-1)
        thr = np.sort(flat)[k - 1]
        carries = _carries_push(mask, bone, ratio, grad)
        # exactly k elements are selected; a selected zero's push term 2 m / k is zero, every other one shows
        below, tied = flat < thr, np.flatnonzero(flat == thr)
        taken = tied[carries[tied]]
        assert thr == 0.25 and int(below.sum()) + len(taken) == k
        assert np.array_equal(carries[flat != thr], (below & (flat != 0))[flat != thr])
        assert len(tied) - len(taken) == int(g[f"{name}_ties_outside"]) == 43
        assert np.array_equal(taken, tied[:len(taken)])                               # the lowest flat indices
    assert torch.isnan(_run(g["empty_bone_mask"], g["empty_bone_bone"], 0.3)[3]).all()
    assert torch.isnan(_run(g["k0_mask"], g["k0_bone"], 0.1)[0])


@pytest.mark.parametrize("ratio", [0.3, 0.7])
@pytest.mark.parametrize("shape,bone_shape", [((32, 128, 128), (32, 128, 128)), ((8, 64, 64), (8, 128, 128))])
def test_training_sizes_match_referee_and_are_no_further_from_it_than_torch(shape, bone_shape, ratio):
    """the sizes training uses. 2^19 uniform fp32 values hold thousands of duplicates, so the comparison is with the
    referee, whose tie rule is the kernel's; torch's fp32 functions are measured against the same referee first and the
    HIP figures must be no further from it"""
    from enarf_gan_amd.models.loss import nerf_patch_loss
    rng = np.random.default_rng(shape[0] * 1000 + int(ratio * 10))
    mask = rng.uniform(0, 1, shape).astype(np.float32)
    bone = (rng.uniform(0, 1, bone_shape) > 0.97).astype(np.float32)
    print(f"{shape}: {mask.size - len(np.unique(mask))} duplicated values of {mask.size}")
    loss, grad = _check(mask, bone, ratio, f"{shape} ratio {ratio}")
    m = torch.as_tensor(mask).cuda().requires_grad_()
    t_loss = nerf_patch_loss(m, torch.as_tensor(bone).cuda(), ratio, COEF)
    (UP * t_loss).backward()
    r_loss, r_grad = R.loss(mask, bone, ratio, COEF), R.loss_grad(mask, bone, ratio, COEF, UP)
    k, flat = int(mask.size * ratio), mask.reshape(-1)
    thr = np.sort(flat)[k - 1]
    settled = (flat != thr).reshape(shape)                          # where topk's pick among equal values cannot matter
    d_torch_loss, d_hip_loss = abs(t_loss.item() - r_loss), abs(loss.item() - r_loss)
    d_torch = np.abs(m.grad.cpu().numpy().astype(np.float64) - r_grad)[settled].max()
    d_hip = np.abs(grad.cpu().numpy().astype(np.float64) - r_grad)[settled].max()
    print(f"{shape} ratio {ratio}: loss |torch - referee| {d_torch_loss:.3e}, |hip - referee| {d_hip_loss:.3e}; "
          f"gradient max |torch - referee| {d_torch:.3e}, |hip - referee| {d_hip:.3e}")
    assert d_hip_loss <= d_torch_loss and d_hip <= d_torch


def test_mask_rendered_by_the_renderer():
    """a mask the renderer itself produced: many exact zeros (rays that miss the body) and a saturated interior"""
    from _helpers import Scene
    from test_host_cpu import Cfg, _nerf_cfg
    from enarf_gan_amd.models.generator import TriNARFGenerator
    S, B, zd = 64, 4, 32
    sc = Scene(S, B, "center_fixed", zd)
    torch.manual_seed(0)
    gen = TriNARFGenerator(Cfg(z_dim=zd, background_ratio=0.7, crop_background=True, pretrained_background=False,
                               nerf_params=_nerf_cfg(Nc=24, Nf=32, constant_triplane=False)), S, 24, sc.raw["parents"], 23,
                           black_background=True)
    gen.register_canonical_pose(sc.raw["canonical_pose"])
    gen = gen.cuda().eval()
    tri = sc.raw["tri_plane"].cuda()
    gen.nerf.tri_plane_gen = lambda z, enc, truncation_psi=1: tri
    s = sc.raw
    with torch.no_grad():
        _, alpha, _, _ = gen(s["pose_to_camera"].cuda(), None, s["bone_length"].cuda(), torch.randn(B, 3 * zd, device="cuda"),
                             s["inv_intrinsics"].cuda())
    mask = alpha.cpu().numpy()
    zeros = float((mask == 0).mean())
    print(f"rendered mask: {zeros:.3f} exact zeros, max {mask.max():.4f}")
    assert mask.shape == (B, S, S) and zeros > 0.2 and mask.max() > 0.2
    bone = np.zeros((B, 2 * S, 2 * S), np.float32)
    bone[:, S - 20:S + 20, S - 2:S + 2] = 1
    for ratio in (0.3, 0.7, float(np.nextafter(zeros, 1))):          # the last one: the threshold is the first value above zero
        _check(mask, bone, ratio, f"rendered mask ratio {ratio:.3f}")


def test_two_runs_give_identical_bits():
    rng = np.random.default_rng(1)
    mask = (np.floor(rng.uniform(0, 1, (8, 64, 64)) * 64) / 64).astype(np.float32)      # heavy ties
    bone = (rng.uniform(0, 1, (8, 128, 128)) > 0.9).astype(np.float32)
    a, b = _run(mask, bone, 0.7), _run(mask, bone, 0.7)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dim() else x.reshape(1).view(torch.int32),
                           y.view(torch.int32) if y.dim() else y.reshape(1).view(torch.int32))
    _check(mask, bone, 0.7, "sixty-fourths")


def test_stream_layout_upstream_gradient_and_model_function():
    rng = np.random.default_rng(2)
    mask = rng.uniform(0, 1, (6, 48, 48)).astype(np.float32)
    bone = (rng.uniform(0, 1, (6, 96, 96)) > 0.95).astype(np.float32)
    want_loss, want_grad = R.loss(mask, bone, 0.5, 3.0), R.loss_grad(mask, bone, 0.5, 3.0, -2.5)
    # a non-default stream
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        loss, _, _, grad = _run(mask, bone, 0.5, 3.0, -2.5)
    stream.synchronize()
    _within_ulp(loss.item(), want_loss, "side stream loss")
    _within_ulp(grad.cpu().numpy(), want_grad, "side stream, upstream -2.5, d fake_mask")
    # non-contiguous inputs: a transposed view and a strided slice
    from enarf_gan_amd import ops
    m = torch.as_tensor(np.ascontiguousarray(mask.transpose(0, 2, 1))).cuda().transpose(1, 2).requires_grad_()
    wide = torch.zeros(6, 96, 192, device="cuda")
    wide[:, :, ::2] = torch.as_tensor(bone).cuda()
    b = wide[:, :, ::2]
    assert not m.is_contiguous() and not b.is_contiguous()
    loss = ops.mask_guidance_loss(m, b, 0.5, 3.0)
    (loss * -2.5).backward()
    _within_ulp(loss.item(), want_loss, "non-contiguous loss")
    _within_ulp(m.grad.cpu().numpy(), want_grad, "non-contiguous d fake_mask")
    # the upstream gradient of a larger graph, and models.loss.mask_guidance_loss as a bone_loss_func
    loss, _, _, grad = _run(mask, bone, 0.5, 10.0, 1.0, via_model=True)
    _within_ulp(loss.item(), R.loss(mask, bone, 0.5, 10.0), "models.loss.mask_guidance_loss")
    _within_ulp(grad.cpu().numpy(), R.loss_grad(mask, bone, 0.5, 10.0, 1.0), "models.loss.mask_guidance_loss gradient")
    m = torch.as_tensor(mask).cuda().requires_grad_()
    scaled = (m * 0.5)
    (ops.mask_guidance_loss(scaled, torch.as_tensor(bone).cuda(), 0.5, 3.0) * 4.0).backward()
    half = (mask.astype(np.float64) * 0.5).astype(np.float32)
    _within_ulp(m.grad.cpu().numpy(), (R.loss_grad(half, bone, 0.5, 3.0, 4.0).astype(np.float32) * np.float32(0.5)),
                "chained d fake_mask")


def test_forward_and_backward_do_not_synchronise():
    from enarf_gan_amd import ops
    m = torch.rand(4, 32, 32, device="cuda").requires_grad_()
    b = (torch.rand(4, 64, 64, device="cuda") > 0.9).float()
    ops.mask_guidance_loss(m, b, 0.7).backward()                    # loads the library
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, push, bone = ops.mask_guidance_loss(m, b, 0.7, return_terms=True)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(m.grad).all())
