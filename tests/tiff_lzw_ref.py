"""The LZW code stream of the GeoTIFF writer in plain Python: the oracle of the host encoder (csrc/tiff_codecs.hip) and of the device
encoder (csrc/tiff_encode.hip).  TIFF 6.0 section 13 as libtiff writes it, minus libtiff's compression-ratio checkpoint:

  codes MSB-first, 9..12 bits; every strip starts with Clear (256) at 9 bits and next = 258; greedy longest match; when (prefix, byte)
  is not in the table: emit prefix at the current width, add the pair as code `next`, next += 1, then if next == 4094 emit Clear at the
  current width (12), empty the table, next = 258, width = 9 -- otherwise, if next > 2^width - 1, width += 1 (the early change); at
  the end of the strip emit the pending prefix, apply the same step once more, emit EOI (257), pad the last byte with zero bits.  An
  empty strip is Clear, EOI.
"""
import numpy as np

CLEAR, EOI, LAST = 256, 257, 4094


def cap(n: int) -> int:
    """bytes that always suffice for a strip of n bytes: at most one 12-bit code per byte, one Clear per 3836 additions, the frame"""
    return (3 * (n + n // 3836 + 4) + 1) // 2


def encode(data) -> bytes:
    data = bytes(data)
    out = bytearray()
    acc = nbits = 0

    def put(code, width):
        nonlocal acc, nbits
        acc = (acc << width) | code
        nbits += width
        while nbits >= 8:
            out.append((acc >> (nbits - 8)) & 0xFF)
            nbits -= 8
        acc &= (1 << nbits) - 1

    table = {}
    width, nxt = 9, 258

    def step():
        nonlocal width, nxt
        nxt += 1
        if nxt == LAST:
            put(CLEAR, width)
            table.clear()
            nxt, width = 258, 9
        elif nxt > (1 << width) - 1:
            width += 1

    put(CLEAR, 9)
    if data:
        prefix = data[0]
        for c in data[1:]:
            key = (prefix << 8) | c
            code = table.get(key)
            if code is not None:
                prefix = code
                continue
            put(prefix, width)
            table[key] = nxt
            step()
            prefix = c
        put(prefix, width)
        step()
    put(EOI, width)
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    return bytes(out)


def blob_mask(H: int, W: int, classes: int = 5, noise: float = 0.0, seed: int = 0) -> np.ndarray:
    """a class mask of smooth blobs (the argmax of a few low-frequency fields), optionally with salt noise on a fraction of the pixels"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.stack([np.sin(x / g.uniform(9, 31) + g.uniform(0, 6)) + np.cos(y / g.uniform(9, 31) + g.uniform(0, 6)) for _ in range(classes)])
    m = f.argmax(axis=0).astype(np.uint8)
    if noise > 0:
        salt = g.random((H, W)) < noise
        m[salt] = g.integers(0, classes, int(salt.sum()), dtype=np.uint8)
    return m
