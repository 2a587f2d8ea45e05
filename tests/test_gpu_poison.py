"""Every launching entry point of the HIP libraries on poisoned, guard-banded allocations (tests/poison.py; the cases and the
map from C ABI functions to them are in tests/poison_cases.py). Each case runs three times - on the allocator's own memory,
with every torch.empty / empty_like / new_empty of the package filled with 0xFFFFFFFF (NaN as fp32 and fp64, -1 as a signed
integer, 255 as uint8) and with 0x7F7F7F7F (3.39e38 as fp32, a large positive integer) - and must give the same results:
what a kernel does not write shows up as the word, what it reads before writing as a NaN or a huge value that spreads, a
write past either end of a tensor as a changed guard byte. A stale value that is multiplied by zero passes under 0x7F7F7F7F
and fails under NaN, which is why both words run."""
import contextlib

import numpy as np
import pytest
import torch

import poison_cases as PC
from _helpers import assert_close
from libraries import binding
from poison import GUARD, poisoned
from test_gpu_backward_f64 import ATOMIC_TOL

pytestmark = pytest.mark.gpu

WORDS = (0xFFFFFFFF, 0x7F7F7F7F)


@contextlib.contextmanager
def recorded(calls):
    """wrap the function attributes of every loaded ctypes library: `calls` collects the names of the functions called"""
    undo = []
    for stem in PC.ALL_STEMS:
        mod = binding(stem)
        lib = mod.load()
        for name in mod.SIGNATURES:
            fn = getattr(lib, name)

            def wrapper(*a, _fn=fn, _name=name):
                calls.add(_name)
                return _fn(*a)
            setattr(lib, name, wrapper)
            undo.append((lib, name, fn))
    try:
        yield
    finally:
        for lib, name, fn in undo:
            setattr(lib, name, fn)


def _bytes(t):
    return t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy()


def _run(name, word):
    """one run of the case: (outputs on the host, check, where each output that the shim served was allocated)"""
    from enarf_gan_amd import _lib
    calls = set()
    PC.SNAPSHOT.clear()
    with recorded(calls), (poisoned(word) if word is not None else contextlib.nullcontext()) as p:
        inputs, outputs, check = getattr(PC, name)()
        torch.cuda.synchronize()
        assert _lib.device_status(clear=True) == 0, f"{name}: device status after the run"
        sites = {}
        if p is not None:
            p.check()
            assert p.records, f"{name}: no allocation of the run was served poisoned"
            for k, t in outputs.items():
                sites[k] = next((site for site, buf, *_ in p.records
                                 if t is not None and buf.data_ptr() <= t.data_ptr() < buf.data_ptr() + buf.numel()),
                                "not served by the shim")
    assert set(PC.SNAPSHOT) == set(inputs), f"{name}: the case did not snapshot its inputs before the call"
    for k, t in inputs.items():
        assert np.array_equal(_bytes(t), _bytes(PC.SNAPSHOT[k])), f"{name}: input {k} was written"
    try:
        check(outputs)
    except AssertionError as e:
        raise AssertionError(f"{name} under {'the allocator' if word is None else hex(word)}: {e}\noutputs allocated at: {sites}") from e
    missing = {fn for fn, cases in PC.POISON_CASES.items() if name in cases} - calls - set(PC.INDIRECT)
    assert not missing, f"{name} is listed under {sorted(missing)} in poison_cases.py but did not call them"
    return {k: v.detach().cpu() for k, v in outputs.items() if v is not None}, check, sites


def _wild(t):
    """where a floating tensor holds a NaN or a magnitude of 1e38 and more"""
    return torch.isnan(t) | (t.abs() >= 1e38)


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_entry_point_on_poisoned_memory(name):
    clean, check, _ = _run(name, None)
    atomic = getattr(check, "atomic", frozenset())
    assert atomic <= set(clean), name
    for word in WORDS:
        out, _, sites = _run(name, word)
        assert set(out) == set(clean), name
        for k, t in out.items():
            what = f"{name} under {word:#x}: {k} (allocated at {sites[k]})"
            assert t.shape == clean[k].shape and t.dtype == clean[k].dtype, what
            if k in atomic:             # float atomics: another order of the same sum
                assert not bool((_wild(t) & ~_wild(clean[k])).any()), f"{what}: a NaN or huge value the clean run does not have"
                assert_close(t, clean[k], what, ATOMIC_TOL)
            else:
                same = _bytes(t) == _bytes(clean[k])
                assert same.all(), (f"{what}: {int((~same).sum())} bytes differ from the clean run, the first at byte "
                                    f"{int(np.argmax(~same))} of {same.size}")


@pytest.mark.parametrize("where", ["behind", "in front"])
def test_shim_reports_a_changed_guard_byte_on_the_device(where):
    """The failure path on the device, without any out-of-bounds access: the byte written lies inside the recorded buffer."""
    from enarf_gan_amd import ops
    real = torch.empty, torch.empty_like, torch.Tensor.new_empty
    with pytest.raises(AssertionError) as e:
        with poisoned(0x7F7F7F7F) as p:
            feat = ops.triplane_pack(torch.zeros(1, 96 + 3 * 23, 3, 5, device="cuda"))        # 3 * 3 * 5 * 32 floats
            site, buf, nbytes, shape, dtype = p.records[-1]
            assert tuple(feat.shape) == shape and feat.data_ptr() == buf.data_ptr() + GUARD and feat.data_ptr() % 512 == 0
            p.check()
            buf[GUARD + nbytes if where == "behind" else GUARD - 1] = 0
    msg = str(e.value)
    assert "ops.py:" in msg and "(1, 3, 3, 5, 32)" in msg and "torch.float32" in msg, msg
    assert ("byte +0 behind" if where == "behind" else "byte -1 in front") in msg, msg
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
