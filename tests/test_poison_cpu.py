"""The allocator shim of tests/poison.py on CPU tensors (where = everything), and the map of tests/poison_cases.py against
the public headers: every declared function is a key of the map, host-only, indirect or recorded as not run."""
import inspect
import struct

import numpy as np
import pytest
import torch

import poison_cases as PC
from libraries import declared
from poison import ALIGN, GUARD, is_cuda, poisoned

NAN_WORD, BIG_WORD = 0xFFFFFFFF, 0x7F7F7F7F
DTYPES = (torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64)     # what the bindings allocate


def everywhere(*_):
    return True


# ------------------------------------------------------------------------------------------------- the shim
@pytest.mark.parametrize("shape,dtype", [((3, 5), torch.float32), ((64,), torch.float32), ((7,), torch.uint8), ((2, 3, 11), torch.float64),
                                         ((1,), torch.int64)])
def test_layout_and_alignment_of_the_view(shape, dtype):
    with poisoned(BIG_WORD, everywhere) as p:
        t = torch.empty(*shape, dtype=dtype)
        (site, buf, nbytes, rshape, rdtype), = p.records
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and (rshape, rdtype) == (shape, dtype)
    assert nbytes == t.numel() * t.element_size()
    assert buf.dtype == torch.uint8 and buf.dim() == 1
    assert buf.numel() == GUARD + -(-nbytes // ALIGN) * ALIGN + GUARD and buf.numel() % ALIGN == 0
    assert t.data_ptr() == buf.data_ptr() + GUARD            # the base's alignment is kept: GUARD is a multiple of 512
    assert GUARD == 4096 and ALIGN == 256 and GUARD % 512 == 0
    assert site.startswith("test_poison_cpu.py:")           # no frame inside the package: the first frame outside the shim
    raw = buf.numpy()
    assert (raw.view(np.uint32) == BIG_WORD).all()           # the whole buffer, the tensor's bytes included


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_words_read_as_documented_in_every_dtype(dtype):
    with poisoned(NAN_WORD, everywhere):
        a = torch.empty(5, dtype=dtype)
    with poisoned(BIG_WORD, everywhere):
        b = torch.empty(5, dtype=dtype)
    if dtype.is_floating_point:
        assert bool(torch.isnan(a).all())
        want = struct.unpack("<f", struct.pack("<I", BIG_WORD))[0] if dtype == torch.float32 else \
            struct.unpack("<d", struct.pack("<II", BIG_WORD, BIG_WORD))[0]
        assert bool((b == want).all()) and (dtype != torch.float32 or abs(want - 3.39e38) < 0.01e38) and want >= 1e38
    elif dtype == torch.uint8:
        assert bool((a == 255).all()) and bool((b == 0x7F).all())
    else:
        assert bool((a == -1).all())
        assert bool((b == int.from_bytes(b"\x7f" * dtype.itemsize, "little")).all()) and int(b[0]) > 2 ** 30


def _site_line():
    return inspect.currentframe().f_back.f_lineno


@pytest.mark.parametrize("where,offset", [("one element past the end", "+0"), ("slack", "+37"), ("back guard", None),
                                          ("front guard", "-1"), ("far front", "-4096")])
def test_a_write_outside_the_tensor_is_reported_with_its_site(where, offset):
    with pytest.raises(AssertionError) as e:
        with poisoned(NAN_WORD, everywhere) as p:
            line = _site_line() + 1
            t = torch.empty(3, 5, dtype=torch.float32)                  # 60 bytes, 196 of slack
            buf, nbytes = p.records[0][1], p.records[0][2]
            p.check()                                                   # untouched so far
            t.fill_(1.0)
            p.check()                                                   # writing the tensor itself is what it is for
            if where == "one element past the end":
                buf[GUARD + nbytes:GUARD + nbytes + 4].view(torch.float32)[0] = 1.0
            elif where == "slack":
                buf[GUARD + nbytes + 37] = 0
            elif where == "back guard":
                buf[GUARD + ALIGN + 5] = 0
                offset = f"+{ALIGN - nbytes + 5}"
            elif where == "front guard":
                buf[GUARD - 1] = 0
            else:
                buf[0] = 0
    msg = str(e.value)
    assert f"test_poison_cpu.py:{line}" in msg and "(3, 5)" in msg and "torch.float32" in msg, msg
    assert f"byte {offset} " in msg and ("behind" if offset[0] == "+" else "in front") in msg, msg


def test_a_write_of_the_pattern_s_own_bytes_at_another_phase_is_seen():
    """the comparison is bytewise against the pattern at the byte's own offset, not against any byte of the word"""
    with pytest.raises(AssertionError, match=r"byte \+1 behind"):
        with poisoned(0x11223344, everywhere) as p:
            torch.empty(3, dtype=torch.uint8)
            buf = p.records[0][1]
            buf[GUARD + 3 + 1] = int(buf[GUARD + 3])


def test_explicit_check_reports_and_keeps_reporting():
    with poisoned(BIG_WORD, everywhere) as p:
        torch.empty(4, dtype=torch.int32)
        p.records[0][1][GUARD + 16] = 0
        for _ in range(2):
            with pytest.raises(AssertionError, match=r"byte \+0 behind"):
                p.check()
        p.records[0][1][GUARD + 16] = 0x7F                                # put back: the exit's check passes


def test_what_passes_through():
    real = torch.empty, torch.empty_like, torch.Tensor.new_empty
    with poisoned(NAN_WORD, everywhere) as p:
        assert torch.empty(0, 3).shape == (0, 3) and torch.empty((2, 0), dtype=torch.int64).numel() == 0
        base = torch.zeros(4, 6)
        like = torch.empty_like(base.t())                                 # non-contiguous: torch chooses the strides
        assert like.shape == (6, 4)
        assert torch.empty_like(base, memory_format=torch.contiguous_format).shape == (4, 6)
        assert torch.empty(2, 2, pin_memory=False).shape == (2, 2)
        assert torch.empty(2, 2, memory_format=torch.contiguous_format).shape == (2, 2)
        out = torch.zeros(3)
        assert torch.empty(3, out=out) is out
        assert base.new_empty((0,)).numel() == 0
        assert not p.records
        # and what is served: the three functions, positional and keyword sizes, dtype and device keywords
        served = [torch.empty(2, 3), torch.empty((2, 3)), torch.empty(size=(2, 3)), torch.empty(torch.Size([2, 3]), dtype=torch.float64),
                  torch.empty_like(base), torch.empty_like(base, dtype=torch.int32), base.new_empty((2, 3)), base.new_empty(2, 3),
                  base.new_empty((5,), dtype=torch.uint8), torch.empty(2, 3, device="cpu"), torch.empty(3, requires_grad=True)]
        assert len(p.records) == len(served)
        assert [tuple(t.shape) for t in served] == [(2, 3)] * 4 + [(4, 6)] * 2 + [(2, 3)] * 2 + [(5,), (2, 3), (3,)]
        assert [t.dtype for t in served] == [torch.float32] * 3 + [torch.float64, torch.float32, torch.int32] + [torch.float32] * 2 + \
            [torch.uint8] + [torch.float32] * 2
        assert served[-1].requires_grad and not served[0].requires_grad
        assert all(bool(torch.isnan(t).all()) for t in served if t.dtype.is_floating_point)
    with poisoned(NAN_WORD) as p:                                         # the default `where`: CPU requests are not served
        assert not bool(torch.isnan(torch.zeros(3) + torch.empty(3).fill_(0)).any())
        torch.empty_like(torch.zeros(2))
        torch.zeros(2).new_empty(3)
        assert not p.records
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    assert is_cuda("cuda") and is_cuda("cuda:1") and is_cuda(torch.device("cuda", 0)) and is_cuda(0)
    assert not is_cuda("cpu") and not is_cuda(torch.device("cpu")) and not is_cuda(None)


def test_the_three_functions_are_restored():
    real = torch.empty, torch.empty_like, torch.Tensor.new_empty
    in_dict = "new_empty" in torch.Tensor.__dict__
    with poisoned(BIG_WORD, everywhere):
        assert torch.empty is not real[0] and torch.empty_like is not real[1] and torch.Tensor.new_empty is not real[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    with pytest.raises(KeyError):
        with poisoned(BIG_WORD, everywhere) as p:
            torch.empty(3)
            p.records[0][1][0] = 0              # a changed guard: the body's own exception is the one that is seen
            raise KeyError("body")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    assert ("new_empty" in torch.Tensor.__dict__) == in_dict
    with pytest.raises(AssertionError, match="guard bands changed"):
        with poisoned(BIG_WORD, everywhere) as p:
            torch.empty(3)
            p.records[0][1][0] = 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real


def test_allocations_inside_the_package_are_named_by_their_own_line():
    """the site is the first frame inside enarf-gan_amd/: synth.py allocates with torch.empty on the host"""
    import os

    from enarf_gan_amd import synth
    src = inspect.getsource(synth)
    assert "torch.empty" in src
    with poisoned(BIG_WORD, everywhere) as p:
        synth.make_scene(8, 1, "center_fixed", 4)
    sites = {r[0] for r in p.records}
    assert sites and all(s.startswith("enarf-gan_amd" + os.sep) for s in sites), sites
    assert any(s.startswith(os.path.join("enarf-gan_amd", "synth.py") + ":") for s in sites), sites


# ------------------------------------------------------------------------------------------------- the map
def test_the_map_accounts_for_every_declared_function():
    everything = set()
    for stem in PC.ALL_STEMS:
        names = set(declared(stem))
        assert names, stem
        everything |= names
        launching = names - set(PC.HOST_ONLY) - set(PC.NOT_RUN)
        missing = launching - set(PC.POISON_CASES)
        assert not missing, f"{stem}: no poison case calls {sorted(missing)}: add one to tests/poison_cases.py"
    extra = (set(PC.POISON_CASES) | set(PC.HOST_ONLY) | set(PC.NOT_RUN) | set(PC.INDIRECT)) - everything
    assert not extra, f"not declared in any public header: {sorted(extra)}"
    assert not set(PC.POISON_CASES) & set(PC.HOST_ONLY) and not set(PC.POISON_CASES) & set(PC.NOT_RUN)
    assert set(PC.INDIRECT) <= set(PC.POISON_CASES)
    assert all(isinstance(r, str) and r for r in list(PC.HOST_ONLY.values()) + list(PC.NOT_RUN.values()) + list(PC.INDIRECT.values()))


def test_the_rows_of_build_libraries_are_all_there():
    from enarf_gan_amd import build
    assert PC.ALL_STEMS == list(build.LIBRARIES) + list(build.SIDE_LIBRARIES)


def test_every_case_exists_and_every_case_is_listed():
    for fn, cases in PC.POISON_CASES.items():
        assert cases and len(set(cases)) == len(cases), fn
        for c in cases:
            f = getattr(PC, c, None)
            assert inspect.isfunction(f) and not inspect.signature(f).parameters, f"{fn}: {c} is not a case of poison_cases.py"
    listed = {c for cases in PC.POISON_CASES.values() for c in cases}
    assert sorted(listed) == PC.CASE_NAMES
    cases_defined = {n for n, f in vars(PC).items() if inspect.isfunction(f) and not n.startswith("_")
                     and f.__module__ == PC.__name__ and not inspect.signature(f).parameters}
    assert cases_defined == listed, f"defined but not in the map, or the reverse: {sorted(cases_defined ^ listed)}"
