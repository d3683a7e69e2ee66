"""fp64 numpy restatement of the non-rigid warps (``unet_warp_field`` / ``unet_warp_field_mask`` / ``unet_elastic_field``) used by the
field-augmentation tests: the three maps of unet_amd.augment's ElasticTransform, GridDistortion and OpticalDistortion, the elastic noise
and its smoothing, and a remap that takes explicit per-pixel source coordinates.  Border handling is warp_ref.border_interpolate."""
import numpy as np

from unet_amd import augment as A
from warp_ref import border_interpolate

LIM = 16777216.0


def _taps(plane, ix, iy, W, H, border, fill):
    jx, vx = border_interpolate(ix, W, border)
    jy, vy = border_interpolate(iy, H, border)
    return np.where(vx & vy, plane[jy, jx], fill)


def pre_mapped(sx, sy, pre=None):
    """the displaced points sx, sy [n, H, W], clamped as the kernel clamps, under the 2 x 3 maps pre [n, 6] (D4 maps of the grid)"""
    sx, sy = np.clip(sx, -LIM, LIM), np.clip(sy, -LIM, LIM)
    if pre is None:
        return sx, sy
    m = np.asarray(pre, dtype=np.float64).reshape(-1, 6)[:, :, None, None]
    return m[:, 0] * sx + m[:, 1] * sy + m[:, 2], m[:, 3] * sx + m[:, 4] * sy + m[:, 5]


def remap_ref(img: np.ndarray, sx: np.ndarray, sy: np.ndarray, interp: int, border: int, fill: float = 0.0) -> np.ndarray:
    """img [n, C, H, W] sampled at the source coordinates sx, sy [n, H, W] (fp64) -> fp64 [n, C, H, W]"""
    n, C, H, W = img.shape
    out = np.empty((n, C, H, W), np.float64)
    for j in range(n):
        planes = img[j].astype(np.float64)

        def taps(ix, iy):                                   # [C, H, W]: the tap of every plane
            jx, vx = border_interpolate(ix, W, border)
            jy, vy = border_interpolate(iy, H, border)
            return np.where((vx & vy)[None], planes[:, jy, jx], fill)

        if interp == 0:
            out[j] = taps(np.floor(sx[j] + 0.5), np.floor(sy[j] + 0.5))
            continue
        x0, y0 = np.floor(sx[j]), np.floor(sy[j])
        fx, fy = sx[j] - x0, sy[j] - y0
        out[j] = ((1 - fx) * (1 - fy) * taps(x0, y0) + fx * (1 - fy) * taps(x0 + 1, y0)
                  + (1 - fx) * fy * taps(x0, y0 + 1) + fx * fy * taps(x0 + 1, y0 + 1))
    return out


def remap_mask_ref(mask: np.ndarray, sx: np.ndarray, sy: np.ndarray, border: int, fill=0) -> np.ndarray:
    """mask [n, H, W] (any dtype) -> same dtype, nearest"""
    n, H, W = mask.shape
    out = np.empty_like(mask)
    for j in range(n):
        out[j] = _taps(mask[j], np.floor(sx[j] + 0.5), np.floor(sy[j] + 0.5), W, H, border, fill)
    return out


def tie_coords(sx: np.ndarray, sy: np.ndarray, tol: float = 1e-3) -> np.ndarray:
    """bool, the shape of sx: the source coordinate is within tol of a nearest-neighbour rounding tie (k + 0.5) on either axis"""
    near = lambda s: np.abs(s - (np.floor(s) + 0.5)) <= tol
    return near(sx) | near(sy)


def pixel_grid(H: int, W: int):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return x, y


# ---------------------------------------------------------------------------------------------------------------------- the maps
def dense_coords(field: np.ndarray):
    """field [n, 2, H, W] -> (x + dx, y + dy), each [n, H, W] fp64"""
    x, y = pixel_grid(*field.shape[-2:])
    return x + field[:, 0].astype(np.float64), y + field[:, 1].astype(np.float64)


def linspace_loop(N: int, num_steps: int, factors) -> np.ndarray:
    """albumentations' GridDistortion loop along one axis of N pixels (fp64); a step of 0 pixels (N < num_steps) counts as 1"""
    step = max(N // num_steps, 1)
    xx = np.zeros(N, np.float64)
    prev = 0.0
    for idx, start in enumerate(range(0, N, step)):
        end = start + step
        if end > N:
            end = N
            cur = float(N)
        else:
            cur = prev + step * factors[idx]
        xx[start:end] = np.linspace(prev, cur, end - start)
        prev = cur
    return xx


def grid_table(nodes, step: int, N: int) -> np.ndarray:
    """the table the kernel evaluates from the fp32 node values of one axis: cell c from nodes[c] to nodes[c + 1]"""
    nodes = np.asarray(nodes, dtype=np.float64)
    xx = np.empty(N, np.float64)
    for c, start in enumerate(range(0, N, step)):
        end = min(start + step, N)
        xx[start:end] = np.linspace(nodes[c], nodes[c + 1], end - start)
    return xx


def grid_coords(step_x: int, step_y: int, nodes: np.ndarray, H: int, W: int):
    """nodes [n, 2, 17] -> (xx[x], yy[y]), each [n, H, W]"""
    sx = np.stack([np.broadcast_to(grid_table(nd[0], step_x, W)[None, :], (H, W)) for nd in nodes])
    sy = np.stack([np.broadcast_to(grid_table(nd[1], step_y, H)[:, None], (H, W)) for nd in nodes])
    return sx, sy


def optical_coords(prm: np.ndarray, H: int, W: int):
    """prm [n, 3] = (k, dx, dy) -> (W u' kappa + c_x + dx, H v' kappa + c_y + dy) with kappa - 1 = k (r^2 + r^4), each [n, H, W]"""
    x, y = pixel_grid(H, W)
    ax, ay = x - (W - 1) / 2.0, y - (H - 1) / 2.0
    r2 = (ax / W) ** 2 + (ay / H) ** 2
    sx, sy = [], []
    for k, dx, dy in np.asarray(prm, dtype=np.float64):
        g = k * (r2 + r2 * r2)
        sx.append(x + ax * g + dx)
        sy.append(y + ay * g + dy)
    return np.stack(sx), np.stack(sy)


# --------------------------------------------------------------------------------------------------------------- the elastic field
def elastic_noise(key, q: int, H: int, W: int) -> np.ndarray:
    """noise plane q [H, W] fp64: 2 u - 1 with u = ((w >> 8) + 0.5) 2^-24, w = word e % 4 of Philox4x32-10 at counter (e / 4, q, 0, 0)"""
    e = np.arange(H * W, dtype=np.int64)
    ctr = np.zeros((H * W, 4), dtype=np.uint32)
    ctr[:, 0] = e // 4
    ctr[:, 1] = q
    w = A.philox4x32_10(ctr, key)[e, e % 4]
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    return (2.0 * u - 1.0).reshape(H, W)


def gauss_taps(sigma: float, ksize: int) -> np.ndarray:
    i = np.arange(ksize, dtype=np.float64) - ksize // 2
    g = np.exp(-i * i / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def smooth(plane: np.ndarray, taps) -> np.ndarray:
    """plane [H, W] filtered along rows, then along columns, border reflect-101 at any distance (fp64 sums of the fp32 taps)"""
    H, W = plane.shape
    t = np.asarray(taps, dtype=np.float64)
    r = len(t) // 2
    off = np.arange(-r, r + 1)
    cols, _ = border_interpolate(np.arange(W)[:, None] + off[None], W, 4)      # [W, k]
    rows, _ = border_interpolate(np.arange(H)[:, None] + off[None], H, 4)      # [H, k]
    p = plane.astype(np.float64)
    x = np.zeros((H, W), np.float64)
    for k in range(len(t)):
        x += t[k] * p[:, cols[:, k]]
    out = np.zeros((H, W), np.float64)
    for k in range(len(t)):
        out += t[k] * x[rows[:, k], :]
    return out


def elastic_field_ref(key, alpha: float, taps, same_dxdy: bool, H: int, W: int) -> np.ndarray:
    """[2, H, W] fp64: the displacement planes (dx, dy) of one image; alpha as the fp32 value the kernel gets"""
    a = float(np.float32(alpha))
    dx = a * smooth(elastic_noise(key, 0, H, W), taps)
    dy = dx if same_dxdy else a * smooth(elastic_noise(key, 1, H, W), taps)
    return np.stack([dx, dy])


# ------------------------------------------------------------------------------------------------------- inputs of the remap tests
SHAPES = [(3, 4, 48, 80), (2, 1, 7, 5), (2, 5, 32, 32), (1, 4, 1, 9), (2, 4, 512, 512)]
KINDS = ("dense", "grid", "optical")
SEED = 2           # chosen so that no case has a tied row or column of a grid map (test_augment_field_cpu checks the 1 % cap)


def remap_case(shape, kind: str):
    """the inputs of one remap test: (params for ops.warp_field, fired, pre-maps [n, 6], source coordinates sx, sy [n, H, W] in fp64).
    The last image of a batch of several did not fire, the first one sits behind a horizontal flip (a transposition too when the grid
    is square); dense fields reach +-1.5 W and hold whole-pixel displacements in their first rows."""
    n, _, H, W = shape
    g = np.random.default_rng(1000 * KINDS.index(kind) + H * W + n + SEED)
    fired = [not (n > 1 and j == n - 1) for j in range(n)]
    pre = np.tile(np.array(A.IDENTITY_MAP, np.float32), (n, 1))
    flip = A.HorizontalFlip().matrix(None, H, W)
    pre[0] = A.inverse_map(A.Transpose().matrix(None, H, W) @ flip if H == W else flip)
    if kind == "dense":
        params = g.uniform(-1.5 * W, 1.5 * W, (n, 2, H, W)).astype(np.float32)
        params[:, :, :max(H // 8, 1)] = np.round(params[:, :, :max(H // 8, 1)])
        sx, sy = dense_coords(params)
    elif kind == "grid":
        steps = 5 if min(H, W) >= 10 else max(H, W)         # tiny grids: cells of one pixel
        nodes = np.stack([np.stack([A.grid_nodes(W, steps, 1.0 + g.uniform(-0.6, 0.6, steps + 1))[1],
                                    A.grid_nodes(H, steps, 1.0 + g.uniform(-0.6, 0.6, steps + 1))[1]]) for _ in range(n)])
        params = (max(W // steps, 1), max(H // steps, 1), nodes)
        sx, sy = grid_coords(params[0], params[1], nodes, H, W)
    else:
        params = np.stack([g.uniform(-2.0, 2.0, n), g.uniform(-0.7, 0.7, n) * W, g.uniform(-0.7, 0.7, n) * H], axis=1).astype(np.float32)
        sx, sy = optical_coords(params, H, W)
    x, y = pixel_grid(H, W)
    for j in range(n):
        if not fired[j]:
            sx[j], sy[j] = x, y
    sx, sy = pre_mapped(sx, sy, pre)
    return params, fired, pre, sx, sy
