"""Test-time augmentation restated from the code table's torch expressions (independent of unet_amd/tta.py): oriented inputs through a
model (the CPU oracle in fp32, or its fp64 copy as the arbiter), the output mapped back, summed in code order, divided by k."""
import torch

TABLE = {
    0: lambda x: x,
    1: lambda x: torch.flip(x, [-1]),
    2: lambda x: torch.flip(x, [-2]),
    3: lambda x: torch.flip(x, [-2, -1]),
    4: lambda x: x.transpose(-2, -1),
    5: lambda x: torch.rot90(x, 1, (-2, -1)),
    6: lambda x: torch.rot90(x, -1, (-2, -1)),
    7: lambda x: torch.flip(x.transpose(-2, -1), [-2, -1]),
}
INVERSE = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 5, 7: 7}


def g(x, code):
    return TABLE[code](x)


def g_inv(x, code):
    return TABLE[INVERSE[code]](x)


def passes(net, x, codes, regression=False):
    """{code: g^-1(softmax(net(g(x))))} (regression: g^-1(net(g(x)))) for x [N, C, H, W] in the net's dtype"""
    out = {}
    with torch.no_grad():
        for c in codes:
            z = net(g(x, c).contiguous())
            out[c] = g_inv(z if regression else torch.softmax(z, dim=1), c)
    return out


def compose(per_code, codes):
    """sum in code order, starting from 0, then one division by k"""
    s = torch.zeros_like(per_code[codes[0]])
    for c in codes:
        s = s + per_code[c]
    return s / len(codes)


def tta(net, x, codes, regression=False):
    return compose(passes(net, x, codes, regression), codes)
