"""Poisoned, guard-banded allocations for the GPU tests (tests/test_gpu_poison.py; tests/test_poison_cpu.py checks the shim).

All device memory of the HIP libraries comes from Python: the bindings and ops.py hand them torch.empty / torch.empty_like /
Tensor.new_empty tensors as outputs and workspaces, and the kernels must write whatever they later read or return. Under
`poisoned(word)` each such request is served from a flat uint8 buffer

    GUARD bytes | the request's nbytes | slack up to the next multiple of 256 | GUARD bytes

filled with the 32-bit `word` repeated; the caller gets the middle as a tensor of its dtype and shape (its data pointer keeps
the allocator's 512-byte alignment, so every vector path is taken as usual). check() then compares the front guard and
everything behind the tensor with the pattern: an entry a kernel does not write shows up as the word in the results, a write
past either end as a changed guard byte, reported with the allocation site inside the package."""
import contextlib
import os
import sys

import torch

GUARD = 4096
ALIGN = 256
_PACKAGE = os.sep + "enarf-gan_amd" + os.sep
_HERE = os.path.abspath(__file__)


def is_cuda(device):
    """the default `where`: a CUDA device (torch.device, string, index or None for the default device)"""
    if device is None:
        get = getattr(torch, "get_default_device", None)
        device = get() if get else "cpu"
    if isinstance(device, int):
        return True
    return torch.device(device).type == "cuda"


def _site():
    """file:line of the first stack frame inside the package (else of the first frame outside this file)"""
    f, outside = sys._getframe(1), None
    while f is not None:
        name = f.f_code.co_filename
        if _PACKAGE in name:
            return "%s:%d" % (name[name.index(_PACKAGE) + 1:], f.f_lineno)
        if outside is None and os.path.abspath(name) != _HERE:
            outside = "%s:%d" % (os.path.basename(name), f.f_lineno)
        f = f.f_back
    return outside or "?"


def _shape_of(args, kwargs):
    if "size" in kwargs:
        args = (kwargs["size"],)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    return tuple(int(a) for a in args)


class Poison:
    """The allocations served under one `poisoned` context: records of (site, base buffer, nbytes, shape, dtype)."""

    def __init__(self, word, where, real_empty):
        assert 0 <= word < 1 << 32
        self.word, self.where, self._empty = word, where, real_empty
        self.signed = word - (1 << 32) if word >= 1 << 31 else word
        self.records = []
        self._patterns = {}

    # ---- serving
    def serve(self, shape, dtype, device, requires_grad=False):
        dtype = dtype or torch.get_default_dtype()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * dtype.itemsize
        total = GUARD + -(-nbytes // ALIGN) * ALIGN + GUARD
        buf = self._empty(total, dtype=torch.uint8, device=device)
        buf.view(torch.int32).fill_(self.signed)
        self.records.append((_site(), buf, nbytes, tuple(shape), dtype))
        out = buf[GUARD:GUARD + nbytes].view(dtype).view(shape)
        return out.requires_grad_() if requires_grad else out

    # ---- checking
    def _pattern(self, device, phase, length):
        """`length` bytes of the repeated word as they stand at a byte offset of `phase` mod 4"""
        key = str(device)
        if key not in self._patterns:
            p = self._empty(2 * GUARD + ALIGN + 8, dtype=torch.uint8, device=device)
            p.view(torch.int32).fill_(self.signed)
            self._patterns[key] = p
        return self._patterns[key][phase % 4:phase % 4 + length]

    def _changed(self, rec):
        """(front, back): bool tensors, True where a guard byte no longer holds the pattern"""
        _, buf, nbytes, _, _ = rec
        back = buf[GUARD + nbytes:]
        return (buf[:GUARD] != self._pattern(buf.device, 0, GUARD),
                back != self._pattern(buf.device, GUARD + nbytes, back.numel()))

    def check(self):
        """Raise AssertionError if any byte in front of or behind a served tensor changed: names the allocation site, the
        tensor's shape and dtype and the offset of the first changed byte from the tensor's end (+0 is the byte right
        behind it) or start (-1 is the byte right in front of it)."""
        if not self.records:
            return
        flags = [torch.stack([f.any(), b.any()]) for f, b in map(self._changed, self.records)]
        if not bool(torch.stack(flags).any()):
            return
        msgs = []
        for rec in self.records:
            site, _, _, shape, dtype = rec
            front, back = self._changed(rec)
            if bool(back.any()):
                at = int(back.nonzero()[0])
                msgs.append(f"{site}: {shape} {dtype}: byte +{at} behind the tensor's end was written ({int(back.sum())} changed)")
            if bool(front.any()):
                at = int(front.nonzero()[-1]) - GUARD
                msgs.append(f"{site}: {shape} {dtype}: byte {at} in front of the tensor's start was written "
                            f"({int(front.sum())} changed)")
        raise AssertionError("guard bands changed:\n  " + "\n  ".join(msgs))


@contextlib.contextmanager
def poisoned(word, where=is_cuda):
    """Serve torch.empty, torch.empty_like and Tensor.new_empty from poisoned, guard-banded buffers for requests whose device
    `where` accepts; everything else - CPU tensors, zero-size requests, non-contiguous empty_like, calls with memory_format,
    pin_memory, out, names or a layout - passes through. Yields the Poison (records, check()); check() runs on a normal exit."""
    real_empty, real_like = torch.empty, torch.empty_like
    had_new = "new_empty" in torch.Tensor.__dict__
    real_new = torch.Tensor.new_empty
    p = Poison(word, where, real_empty)
    plain = {"dtype", "device", "requires_grad", "size"}

    def ok(kwargs, shape, device):
        return set(kwargs) <= plain and all(s > 0 for s in shape) and bool(where(device))

    def empty(*args, **kwargs):
        try:
            shape = _shape_of(args, kwargs)
        except (TypeError, ValueError):
            return real_empty(*args, **kwargs)
        if not ok(kwargs, shape, kwargs.get("device")):
            return real_empty(*args, **kwargs)
        return p.serve(shape, kwargs.get("dtype"), kwargs.get("device"), kwargs.get("requires_grad", False))

    def empty_like(t, *args, **kwargs):
        device = kwargs.get("device", t.device)
        if args or not t.is_contiguous() or t.layout != torch.strided or not ok(kwargs, tuple(t.shape), device):
            return real_like(t, *args, **kwargs)
        return p.serve(tuple(t.shape), kwargs.get("dtype", t.dtype), device, kwargs.get("requires_grad", False))

    def new_empty(self, *args, **kwargs):
        try:
            shape = _shape_of(args, kwargs)
        except (TypeError, ValueError):
            return real_new(self, *args, **kwargs)
        device = kwargs.get("device", self.device)
        if not ok(kwargs, shape, device):
            return real_new(self, *args, **kwargs)
        return p.serve(shape, kwargs.get("dtype", self.dtype), device, kwargs.get("requires_grad", False))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield p
    finally:
        torch.empty, torch.empty_like = real_empty, real_like
        if had_new:
            torch.Tensor.new_empty = real_new
        else:
            del torch.Tensor.new_empty
    p.check()
