"""A model of the operand roundings of the two bf16 MLP modes (csrc/enarf_query.h, mlp_tile_split<false, 3 | 1, false>), as a
drop-in for oracle.enarf_oracle.styled_mlp. Each layer's weights and activations are split as the kernel's split8 splits
them - hi = bf16_rne(x), lo = bf16_rne(x - hi) - the products are hi*hi + hi*lo + lo*hi (`bf16x3`) or hi*hi alone (`bf16`),
summed in float64, the bias added, the result rounded to fp32; LeakyReLU * sqrt(2) in fp32.

It is a calibration aid and a source of corruptions for tests/test_fwd_modes_cpu.py: it says how far the modes' operand
roundings alone take a render from float64, and what a defect in them looks like. It does not restate the kernel's
accumulation order, and no kernel is ever compared with it."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import enarf_oracle as O

TERMS = {"bf16x3": 3, "bf16": 1}


def _rne(v):
    return v.to(torch.bfloat16).to(torch.float32)


def _rtz(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split(x, truncate=None):
    """x (fp32) -> (hi, lo) as fp32 tensors holding bf16 values. truncate (a corruption): "lo" rounds the lo half toward
    zero instead of to nearest even, "both" the hi half too."""
    hi = (_rtz if truncate == "both" else _rne)(x)
    return hi, (_rtz if truncate else _rne)(x - hi)


def styled_mlp(mode, corrupt=None, truncate=None):
    """-> styled_mlp(feature (B,32,N), weights [(W (B,out,in), bias (out,))]) in `mode`. corrupt(layer, halves) may change
    the halves dict(wh, wl, xh, xl) of a layer in place before its products are formed."""
    def run(feature, weights):
        h = feature.float()
        for layer, (w, bias) in enumerate(weights):
            wh, wl = split(w.float(), truncate)
            xh, xl = split(h, truncate)
            p = dict(wh=wh.double(), wl=wl.double(), xh=xh.double(), xl=xl.double())
            if corrupt is not None:
                corrupt(layer, p)
            acc = torch.bmm(p["wh"], p["xh"])
            if TERMS[mode] == 3:
                acc = acc + torch.bmm(p["wh"], p["xl"]) + torch.bmm(p["wl"], p["xh"])
            h = (acc + bias.double()[None, :, None]).float()
            h = F.leaky_relu(h, 0.2) * 2 ** 0.5
        return h.to(feature.dtype)
    return run


@contextlib.contextmanager
def installed(mode, **kw):
    """the oracle's styled_mlp replaced by the model while the block runs"""
    keep = O.styled_mlp
    O.styled_mlp = styled_mlp(mode, **kw)
    try:
        yield
    finally:
        O.styled_mlp = keep
