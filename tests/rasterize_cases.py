"""Inputs of the rasterizer tests (plain NumPy, seeded): class masks with blobs and salt noise, and feature sets for the comparison with
tests/rasterize_ref.py.  A feature set is [(value, [ring, ...]), ...] with rings as [(X, Y), ...] in fixed point (1/256 pixel)."""
import math

import numpy as np

ONE, HALF = 256, 128


def mask(H: int, W: int, seed: int, classes: int = 5, salt: float = 0.06) -> np.ndarray:
    """uint8 [H, W]: coarse random blocks, a few rectangles with a hole and an island in it, some on the frame, then salt noise -- holes,
    saddles (diagonal neighbours), islands inside holes and components on the frame all occur once the raster is a few pixels wide"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, classes, (-(-H // 6), -(-W // 7)), dtype=np.uint8)
    m = np.kron(coarse, np.ones((6, 7), dtype=np.uint8))[:H, :W].copy()
    for _ in range(max(1, H * W // 900)):
        h, w = int(rng.integers(5, 14)), int(rng.integers(5, 14))
        y, x = int(rng.integers(-3, max(H - 3, 1))), int(rng.integers(-3, max(W - 3, 1)))
        c = int(rng.integers(0, classes))
        m[max(y, 0):y + h, max(x, 0):x + w] = c
        m[max(y + 2, 0):max(y + h - 2, 0), max(x + 2, 0):max(x + w - 2, 0)] = (c + 1) % classes          # a hole ...
        if 0 <= y + h // 2 < H and 0 <= x + w // 2 < W:
            m[y + h // 2, x + w // 2] = (c + 2) % classes                                               # ... with an island
    noise = rng.random((H, W)) < salt
    m[noise] = rng.integers(0, classes, int(noise.sum()), dtype=np.uint8)
    return m


def _star(rng, cx, cy, r_out, r_in, points):
    ring, phase = [], rng.random() * math.pi
    for i in range(2 * points):
        r = r_out if i % 2 == 0 else r_in
        a = phase + math.pi * i / points
        ring.append((int(round((cx + r * math.cos(a)) * ONE)), int(round((cy + r * math.sin(a)) * ONE))))
    return ring


def _random_ring(rng, n, x_lo, x_hi, y_lo, y_hi):
    return [(int(rng.integers(x_lo * ONE, x_hi * ONE + 1)), int(rng.integers(y_lo * ONE, y_hi * ONE + 1))) for _ in range(n)]


def _centres(rng, n, W, H):
    """vertices exactly on pixel centres"""
    return [(int(rng.integers(-2, W + 2)) * ONE + HALF, int(rng.integers(-2, H + 2)) * ONE + HALF) for _ in range(n)]


def _box(x0, y0, x1, y1):
    return [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]


def feature_sets(H: int = 40, W: int = 56, seed: int = 11) -> dict:
    rng = np.random.default_rng(seed)
    sets = {}
    sets["stars"] = [(int(rng.integers(1, 250)), [_star(rng, rng.uniform(5, W - 5), rng.uniform(5, H - 5), rng.uniform(6, 16), rng.uniform(1, 5),
                                                        int(rng.integers(3, 8)))]) for _ in range(6)]
    sets["self_intersecting"] = [(int(rng.integers(1, 250)), [_random_ring(rng, int(rng.integers(4, 10)), 0, W, 0, H)]) for _ in range(8)]
    # the tie rules: vertices on pixel centres, horizontal edges on centre rows, vertical edges on centre columns
    ties = [(int(rng.integers(1, 250)), [_centres(rng, int(rng.integers(3, 8)), W, H)]) for _ in range(8)]
    ties.append((77, [_box(3 * ONE + HALF, 4 * ONE + HALF, 30 * ONE + HALF, 21 * ONE + HALF)]))
    ties.append((78, [[(10 * ONE + HALF, 2 * ONE + HALF), (40 * ONE + HALF, 2 * ONE + HALF), (25 * ONE + HALF, 30 * ONE + HALF)]]))
    sets["ties"] = ties
    # the clamps: vertices outside the raster on all four sides
    sets["outside"] = [(int(rng.integers(1, 250)), [_random_ring(rng, int(rng.integers(3, 8)), -25, W + 25, -25, H + 25)]) for _ in range(8)] + [
        (91, [_box(-9 * ONE, -7 * ONE, (W + 9) * ONE, (H + 7) * ONE), _box(5 * ONE + 3, 6 * ONE + 200, (W - 4) * ONE - 17, (H - 5) * ONE)]),
        (92, [_box(-30 * ONE, 10 * ONE, -5 * ONE, 20 * ONE)]), (93, [_box((W + 1) * ONE, 10 * ONE, (W + 30) * ONE, 20 * ONE)]),
        (94, [_box(10 * ONE, -30 * ONE, 20 * ONE, -2 * ONE)]), (95, [_box(10 * ONE, (H + 2) * ONE, 20 * ONE, (H + 30) * ONE)])]
    # rings that burn nothing: two vertices, zero area (there and back), a repeated point, no vertex at all
    sets["degenerate"] = [
        (5, [[(2 * ONE, 3 * ONE), (40 * ONE, 30 * ONE)]]),
        (6, [[(2 * ONE, 3 * ONE), (40 * ONE, 30 * ONE), (2 * ONE, 3 * ONE + 0)], _star(rng, 20, 20, 12, 4, 5)]),
        (7, [[(7 * ONE, 1 * ONE), (7 * ONE, 35 * ONE), (7 * ONE, 20 * ONE)]]),
        (8, [[], _box(30 * ONE, 5 * ONE, 50 * ONE + 77, 17 * ONE + 130), [(1, 1)]]),
        (9, [[(12 * ONE, 12 * ONE), (12 * ONE, 12 * ONE), (12 * ONE, 12 * ONE)]]),
        (10, [])]
    # one feature of 3 disjoint rings, one of them with a hole (a MultiPolygon's rings)
    sets["multi"] = [(200, [_box(2 * ONE + 9, 2 * ONE + 9, 15 * ONE + 100, 14 * ONE + 40), _box(5 * ONE, 5 * ONE, 10 * ONE + 128, 9 * ONE + 128),
                            _star(rng, 38, 12, 10, 3, 6), _random_ring(rng, 3, 5, 50, 22, 38)]), (3, [_box(0, 0, 4 * ONE, 4 * ONE)])]
    # the painter's order
    sets["overlap50"] = [(int(rng.integers(0, 256)), [_star(rng, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(4, 20), rng.uniform(1, 6),
                                                            int(rng.integers(3, 7)))]) for _ in range(50)]
    sets["none"] = []
    return sets


def oblique_halves(s: int, n: int = 64):
    """two rings that share the edge P0 -> P1 on the line X = s (Y - 128) + 128, which runs through the pixel centres (128 + 256 s i, 128 + 256 i)
    of an n x n raster at slope dy / dx = 1 / s: the part of the raster left of the line and the part right of it.  The shared vertices lie
    on the rows Y = 0 and Y = 256 n, at or outside the raster's sides"""
    S = n * ONE
    P0, P1 = (s * (0 - HALF) + HALF, 0), (s * (S - HALF) + HALF, S)
    return [P0, (P0[0], S), P1], [P0, P1, (P1[0], 0)]
