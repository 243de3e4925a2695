"""numpy restatement of the trajectory unwrap (include/mdapy_amd.h, the ``_unwrap`` section) and the inputs its tests share.

Every product and sum is written out in the library's order — no ``@``, whose BLAS may fuse or reorder — so that on the same
input the restatement and the kernel run the same binary64 operations:

    frac[f, i, d]      = (x * inv[f][0][d] + y * inv[f][1][d]) + z * inv[f][2][d]
    k[f, i, d]         = np.round(frac[f-1, i, d] - frac[f, i, d]) on a periodic axis for f >= 1, else 0
    s                  = the running sum of k over the frames (int64), or the image flags
    unwrapped[f, i, d] = p_d + ((sx * cell[f][0][d] + sy * cell[f][1][d]) + sz * cell[f][2][d])

``unwrap`` has the signature of ``mdapy_amd._unwrap.unwrap``: the host tests install this module as ``kernels.unwrap``."""
import functools

import numpy as np

U = 2.0 ** -53


def restate(pos, cells, pbc, row_of=None, image=None):
    """(unwrapped (F, N, 3) float64, shifts (F, N, 3) int64)"""
    pos = np.asarray(pos, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.float64)
    F, N = pos.shape[:2]
    if row_of is not None:
        frames = np.arange(F)[:, None]
        pos = pos[frames, np.asarray(row_of)]
        if image is not None:
            image = np.asarray(image)[frames, np.asarray(row_of)]
    x, y, z = pos[:, :, 0], pos[:, :, 1], pos[:, :, 2]
    if image is not None:
        shifts = np.asarray(image).astype(np.int64)
    else:
        inv = np.linalg.inv(cells)
        steps = np.zeros((F, N, 3), np.int64)
        for d in range(3):
            if not pbc[d]:
                continue
            frac = (x * inv[:, 0, d][:, None] + y * inv[:, 1, d][:, None]) + z * inv[:, 2, d][:, None]
            jump = frac[:-1] - frac[1:]
            if not np.all(np.abs(jump) < 2.0 ** 31):  # (a NaN compares false)
                raise ValueError("unwrap restatement: a step in fractional coordinates is not finite or reaches 2^31")
            steps[1:, :, d] = np.round(jump).astype(np.int64)
        shifts = np.cumsum(steps, axis=0)
    sx, sy, sz = (shifts[:, :, k].astype(np.float64) for k in range(3))
    unwrapped = np.empty((F, N, 3), np.float64)
    for d in range(3):
        unwrapped[:, :, d] = pos[:, :, d] + ((sx * cells[:, 0, d][:, None] + sy * cells[:, 1, d][:, None]) + sz * cells[:, 2, d][:, None])
    return unwrapped, shifts


def unwrap(pos, cells, pbc, unwrapped, row_of=None, image=None, shifts=None, chunks=0):
    got, s = restate(np.asarray(pos), cells, np.asarray(pbc), None if row_of is None else np.asarray(row_of),
                     None if image is None else np.asarray(image))
    unwrapped[...] = got
    if shifts is not None:
        shifts[...] = s


def bound(wrapped, shifts, cells):
    """8 u (|p_d| + sum over k of |s_k| |cell[k][d]|): three products and three sums on each side, in any order and with any
    fusing, doubled"""
    reach = np.einsum("fnk,fkd->fnd", np.abs(shifts).astype(np.float64), np.abs(cells))
    return 8.0 * U * (np.abs(wrapped) + reach)


# ---- inputs
SHEAR = np.array([[10.3, 0.0, 0.0], [2.7, 9.1, 0.0], [1.3, -2.2, 11.7]])
DYADIC_SHEAR = np.array([[10.0, 0.0, 0.0], [2.5, 9.0, 0.0], [1.5, -2.0, 11.0]])


def cells_of(kind, F):
    """(F, 3, 3): "cubic", "sheared", "npt" (the sheared cell breathing and leaning a little more in every frame), and their
    "dyadic_" twins, whose entries are small binary fractions: an integer combination of their rows is exact"""
    f = np.arange(F, dtype=np.float64)[:, None, None]
    if kind == "cubic":
        return np.repeat(np.diag([10.3, 10.3, 10.3])[None], F, axis=0)
    if kind == "sheared":
        return np.repeat(SHEAR[None], F, axis=0)
    if kind == "npt":
        lean = np.zeros((3, 3))
        lean[1, 0], lean[2, 1] = 0.013, -0.007
        return SHEAR[None] * (1.0 + 0.0021 * f) + lean[None] * f
    if kind == "dyadic_cubic":
        return np.repeat(np.diag([8.0, 8.0, 8.0])[None], F, axis=0)
    if kind == "dyadic_sheared":
        return np.repeat(DYADIC_SHEAR[None], F, axis=0)
    if kind == "dyadic_npt":
        return DYADIC_SHEAR[None] * (1.0 + f / 1024.0)
    raise KeyError(kind)


def heights(cell):
    return 1.0 / np.linalg.norm(np.linalg.inv(cell), axis=0)


def continuous_walk(cells, N, seed, start_boxes=1):
    """(F, N, 3) a walk that never wraps: starting points spread over ``start_boxes`` cells either side of the first, steps shorter
    than 0.245 of the shortest cell height of any frame; even atoms drift up the x axis and odd ones down it, so that an atom
    crosses a boundary several times"""
    rng = np.random.default_rng(seed)
    F = len(cells)
    h = min(float(heights(c).min()) for c in cells)
    start = rng.uniform(-start_boxes, 1 + start_boxes, (1, N, 3)) @ cells[0]
    steps = rng.uniform(-0.1 * h, 0.1 * h, (F, N, 3))
    steps[:, 0::2, 0] += 0.1 * h
    steps[:, 1::2, 0] -= 0.1 * h
    steps[0] = 0.0
    return start + np.cumsum(steps, axis=0)


def wrap(walk, cells):
    """(wrapped, the count n of cells taken off: wrapped = walk - n @ cell)"""
    n = np.floor(np.einsum("fnk,fkd->fnd", walk, np.linalg.inv(cells)))
    return walk - np.einsum("fnk,fkd->fnd", n, cells), n.astype(np.int64)


def margin(wrapped, cells, row_of=None):
    """the smallest distance of a step frac[f-1] - frac[f] from a half-integer (inf for one frame): what makes equal integer
    shifts a fair demand of two formulations that round differently"""
    if row_of is not None:
        wrapped = wrapped[np.arange(len(wrapped))[:, None], row_of]
    frac = np.einsum("fnk,fkd->fnd", wrapped, np.linalg.inv(cells))
    jump = frac[:-1] - frac[1:]
    return float(np.abs(np.abs(jump - np.floor(jump)) - 0.5).min()) if jump.size else float("inf")


@functools.lru_cache(maxsize=None)
def case(kind, F, N):
    """(walk, wrapped, n, cells) of a named input, made once; all read-only"""
    cells = cells_of(kind, F)
    walk = continuous_walk(cells, N, 100000 * len(kind) + 1000 * F + N)
    wrapped, n = wrap(walk, cells)
    for a in (walk, wrapped, n, cells):
        a.setflags(write=False)
    return walk, wrapped, n, cells


def permutations(F, N, seed):
    """(F, N) int64: another random order of the rows for every frame"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(N) for _ in range(F)]).astype(np.int64)
