"""CPU checks of the GAN supervision (libenarf_guide.so, include/enarf_guide.h): the float64 restatement
(tests/mask_guidance_reference.py) against the reference's recorded losses and gradients and against the torch functions
of models/loss.py, the library's ABI and kernel inventory, and the refusals that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import libraries as L
import mask_guidance_reference as R

ROOT, TESTS = L.ROOT, L.TESTS
SRC = os.path.join(ROOT, "enarf-gan_amd", "csrc", "enarf_guide.hip")
HEADER = L.header("guide")

def golden():
    return np.load(os.path.join(TESTS, "golden", "mask_guidance.npz"))


def same(a, b, rel):
    """NaN where the other is NaN, elsewhere within rel of the largest magnitude"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    if not np.array_equal(np.isnan(a), nan):
        return False
    if nan.all():
        return True
    return bool(np.abs(a[~nan] - b[~nan]).max() <= rel * max(np.abs(b[~nan]).max(), 1e-300))


# ------------------------------------------------------------------------------------------------- the restatement
def test_restatement_reproduces_reference_fixture():
    g = golden()
    coef, up = float(g["coef"]), float(g["up"])
    names = [str(n) for n in g["cases"]]
    assert sorted(names) == sorted(["uniform", "zeros60", "zeros80", "four_d", "ratio0", "quantised", "empty_bone", "k0"])
    for name in names:
        mask, bone, ratio = g[f"{name}_mask"], g[f"{name}_bone"], float(g[f"{name}_ratio"])
        k, sel = R.selection(mask, ratio)
        assert k == int(g[f"{name}_k"]) == (int(mask.size * ratio) if ratio > 0 else 0), name
        assert int(sel.sum()) == k, name
        # float64 round-off of sums of <= 4096 terms taken in another order than torch's
        assert same(R.loss(mask, bone, ratio, coef), g[f"{name}_loss"], 1e-13), name
        grad = R.loss_grad(mask, bone, ratio, coef, up)
        assert grad.shape == mask.shape
        if name == "quantised":
            # values equal to a non-zero threshold stay outside: which ones the reference's topk took is not a function
            # of the input, so the gradient is the referee's alone, pinned by its invariants
            assert f"{name}_d_mask" not in g.files and int(g[f"{name}_ties_outside"]) == 43
            on = R.pooled_on_bone(bone, mask.shape)
            push_part = grad - R.loss_grad(mask, bone, 0.0, coef, up)              # what the push term adds
            carries = (push_part != 0).reshape(-1)
            flat, thr = mask.reshape(-1), np.sort(mask.reshape(-1))[k - 1]
            # exactly k values are selected and exactly they carry the push term (2 m / k, nothing for a selected zero)
            assert thr == 0.25 and int(sel.sum()) == k and int(carries.sum()) == k - int((flat[sel.reshape(-1)] == 0).sum())
            assert np.array_equal(carries, sel.reshape(-1) & (flat != 0))
            tied = np.flatnonzero(flat == thr)
            taken = tied[sel.reshape(-1)[tied]]
            assert len(tied) - len(taken) == 43 and np.array_equal(taken, tied[:len(taken)])   # the lowest indices
            assert sel.reshape(-1)[flat < thr].all() and not sel.reshape(-1)[flat > thr].any()
            assert on.any()
        else:
            assert same(grad, g[f"{name}_d_mask"], 1e-13), name                    # element by element, none left out
    assert np.isnan(g["empty_bone_loss"]) and np.isnan(g["empty_bone_d_mask"]).all()
    assert np.isnan(g["k0_loss"]) and np.isfinite(g["k0_d_mask"]).all()
    assert int(g["zeros80_ties_outside"]) == 410 and np.sort(g["zeros80_mask"].reshape(-1))[int(g["zeros80_k"]) - 1] == 0
    assert all(int(g[f"{n}_ties_outside"]) == 0 for n in names if n not in ("zeros80", "quantised"))


def test_restatement_matches_torch_functions_in_float64():
    from enarf_gan_amd.models.loss import nerf_bone_loss, nerf_patch_loss, push_to_background
    rng = np.random.default_rng(11)
    for shape, bone_shape, ratio in (((3, 8, 8), (3, 8, 8), 0.3), ((2, 8, 8), (2, 24, 24), 0.7), ((2, 5, 5), (2, 11, 11), 0.5),
                                     ((2, 2, 6, 6), (2, 2, 6, 6), 0.4), ((1, 16, 16), (1, 33, 33), 0.0)):
        mask = rng.uniform(-0.1, 1.1, shape).astype(np.float32)
        assert len(np.unique(mask)) == mask.size                                   # no ties: topk's pick is determined
        bone = (rng.uniform(0, 1, bone_shape) > 0.8).astype(np.float32) * rng.uniform(0.3, 1.0, bone_shape).astype(np.float32)
        m = torch.tensor(mask, dtype=torch.float64, requires_grad=True)
        b = torch.tensor(bone, dtype=torch.float64)
        loss = nerf_patch_loss(m, b, ratio, 7.0)
        (1.5 * loss).backward()
        push, bone_term = R.terms(mask, bone, ratio)
        assert same(push, float(push_to_background(m.detach(), ratio)), 1e-13)
        assert same(bone_term, float(nerf_bone_loss(m.detach(), b)), 1e-13)
        assert same(R.loss(mask, bone, ratio, 7.0), loss.item(), 1e-13), shape
        assert same(R.loss_grad(mask, bone, ratio, 7.0, 1.5), m.grad.numpy(), 1e-13), shape


def test_restatement_key_order_and_pooling():
    v = np.array([np.nan, np.inf, 1.0, 1e-40, 0.0, -0.0, -1e-40, -1.0, -np.inf, -np.nan], dtype=np.float32)
    k = R.key(v)
    assert k[0] == k[9] == 0xFFFFFFFF                                              # NaN of either sign is the largest
    assert list(np.argsort(k[1:9], kind="stable")) == [7, 6, 5, 4, 3, 2, 1, 0]     # strictly descending as listed
    bone = np.zeros((1, 7, 7), np.float32)
    bone[0, 6, 6] = 1                                                              # in the dropped remainder
    bone[0, 1, 2] = 0.6
    bone[0, 4, 4] = np.nan                                                         # a NaN window is not on the bone
    bone[0, 5, 5] = 1
    on = R.pooled_on_bone(bone, (1, 3, 3))
    assert on.sum() == 1 and on[0, 0, 1]
    for bad in ((1, 4, 4), (1, 8, 8)):
        with pytest.raises(ValueError):
            R.pooled_on_bone(bone, bad)


# ------------------------------------------------------------------------------------------------- the library
def test_header_symbols_exported_and_bound():
    """what is specific to this library; tests/test_libraries_cpu.py holds the checks every library gets"""
    from enarf_gan_amd import _guide_lib
    assert L.declared("guide") == ["enarf_guide_abi_version", "enarf_guide_last_error", "enarf_guide_loss_bwd",
                                   "enarf_guide_loss_fwd"]
    assert _guide_lib.ABI_VERSION == 1
    header = open(HEADER).read()
    assert f"#define ENARF_GUIDE_MAX_BLOCKS {_guide_lib.MAX_BLOCKS}" in header
    assert "#define ENARF_GUIDE_RADIX_BITS 8" in header and "#define ENARF_GUIDE_PASSES     4" in header
    assert _guide_lib.WORK_BYTES == 2 * 512 * 8 + (4 * 256 + 2 * 512) * 4 and _guide_lib.STATE_INTS == 4 + 512
    assert _guide_lib.geometry(1) == (256, 1) and _guide_lib.geometry(257) == (256, 2)
    assert _guide_lib.geometry(32 * 128 * 128) == (1024, 512) and _guide_lib.geometry(512 * 1024 + 1) == (1280, 410)
    for n in (1, 255, 256, 1000, 131072, 131073, (1 << 31) - 1):
        chunk_len, chunks = _guide_lib.geometry(n)
        assert chunk_len % 256 == 0 and chunks <= _guide_lib.MAX_BLOCKS and (chunks - 1) * chunk_len < n <= chunks * chunk_len


def test_sources_read_no_environment_and_hold_no_assembly_or_float_atomics():
    src = open(SRC).read()
    assert "getenv" not in src and "asm" not in src
    # the only atomics are the integer adds of the histograms
    atomics = re.findall(r"atomic\w*\(&(\w+)", src)
    assert atomics and set(atomics) <= {"local", "w"}, atomics
    assert re.search(r"__shared__ unsigned int local\[kBins\]", src) and re.search(r"unsigned int hist\[kPasses\]\[kBins\]", src)
    for path in ("_guide_lib.py", os.path.join("models", "loss.py"), os.path.join("models", "gan.py")):
        text = open(os.path.join(ROOT, "enarf-gan_amd", path)).read()
        assert "os.environ" not in text and "getenv" not in text, path


def test_abi_refusals_need_no_device():
    from enarf_gan_amd import _guide_lib
    L.library("guide")
    lib = _guide_lib.load()
    err = lib.enarf_guide_last_error

    def fwd(fake=8, bone=8, B=2, s=16, S=32, k=10, push=1, work=8, state=8, out=8):
        return lib.enarf_guide_loss_fwd(fake, bone, B, s, S, k, push, 10.0, work, state, out, None)
    assert fwd(B=0) == -1 and b"N == 0" in err()
    assert fwd(s=0) == -1
    assert fwd(S=15) == -1 and b"rate of 0" in err()
    assert fwd(S=40) == -1 and b"pooled by 2" in err()
    assert fwd(k=-1) == -1 and fwd(k=2 * 16 * 16 + 1) == -1 and b"outside [0, N" in err()
    assert fwd(B=1 << 20, s=64, S=64) == -1 and b"2^31" in err()
    assert fwd(fake=None) == -1 and fwd(bone=None) == -1
    assert fwd(work=None) == -1 and fwd(state=None) == -1 and fwd(out=None) == -1
    assert fwd(work=4) == -1 and b"aligned" in err()

    def bwd(B=2, s=16, S=16, k=10, state=8, up=8, d=8):
        return lib.enarf_guide_loss_bwd(8, 8, B, s, S, k, 1, 10.0, state, up, d, None)
    assert bwd(B=0) == -1 and bwd(S=8) == -1 and bwd(k=513) == -1
    assert bwd(state=None) == -1 and bwd(up=None) == -1 and bwd(d=None) == -1


def test_binding_refusals_need_no_device():
    from enarf_gan_amd import ops
    from enarf_gan_amd._lib import EnarfHipError
    from enarf_gan_amd.models.loss import mask_guidance_loss
    mask, bone = torch.rand(2, 16, 16), torch.zeros(2, 32, 32)
    for m, b in ((torch.rand(2, 16, 12), torch.zeros(2, 16, 12)),             # not square
                 (mask, torch.zeros(2, 8, 8)),                                # a rate of 0
                 (mask, torch.zeros(2, 40, 40)),                              # pools to 20 x 20
                 (mask, torch.zeros(3, 32, 32)), (mask, torch.zeros(2, 32, 48)),
                 (mask, torch.zeros(2, 1, 32, 32)),                           # the dimensions differ
                 (mask[:, None], bone[:, None]),                              # 4-D at another resolution
                 (torch.rand(0, 16, 16), torch.zeros(0, 16, 16)),             # N == 0
                 (torch.rand(16), torch.zeros(16))):
        with pytest.raises(ValueError):
            ops.mask_guidance_loss(m, b)
    with pytest.raises(ValueError):
        ops.mask_guidance_loss(mask, bone, background_ratio=1.5)              # k > N, as torch.topk refuses
    with pytest.raises(NotImplementedError):
        ops.mask_guidance_loss(mask, bone.clone().requires_grad_())
    # no CPU fallback, fp32 only
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        ops.mask_guidance_loss(mask, bone)
    with pytest.raises(EnarfHipError, match="no CPU fallback"):
        mask_guidance_loss(mask, bone, 0.7)
    if torch.cuda.is_available():
        with pytest.raises(EnarfHipError, match="fp32"):
            ops.mask_guidance_loss(mask.cuda().double(), bone.cuda().double())


def test_train_step_refuses_bad_batches_before_anything_runs():
    import types
    from enarf_gan_amd.models import gan
    gen = types.SimpleNamespace(config=types.SimpleNamespace(z_dim=8))
    batch = {"pose_to_camera": torch.zeros(4, 24, 4, 4), "bone_length": torch.zeros(4, 23, 1),
             "bone_mask": torch.zeros(4, 32, 32), "inv_intrinsics": torch.zeros(4, 3, 3)}
    kw = dict(adv_loss_type="ce", bone_guided_coef=1.0, r1_loss_coef=10.0)
    with pytest.raises(ValueError, match="micro-batches"):
        gan.train_step(gen, None, None, None, batch, None, 0, n_accum_step=3, **kw)
    with pytest.raises(ValueError, match="z must be"):
        gan.train_step(gen, None, None, None, batch, None, 0, n_accum_step=2, z=torch.zeros(4, 16), **kw)
