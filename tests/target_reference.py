"""Reference of the target screens (axtrack_amd/csrc/target.hip), independent of the package: SciPy's Dijkstra on the
reversed grid graph with the weights of AxonDetections.py:598 (1 on the mask, 65536 off it), the walk rule of the target
paths in numpy, and the masks the tests use. The reference project has no code for this feature.

A move costs the weight of the cell moved into. For the distance of every cell TO the targets the graph is reversed:
the edge u -> v (v a neighbour of u) weighs w(u), so that the distance from the targets to c in the reversed graph is
the cost of the cheapest path from c to a target, the target cell included. With d = 65536 off + on (on < 65536):
off = d // 65536 cells entered off the mask, moves = off + on = d - 65535 off."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

DY8 = (-1, 1, 0, 0, -1, -1, 1, 1)          # up, down, left, right, then the diagonals in csrc/grid.h's order
DX8 = (0, 0, -1, 1, -1, 1, -1, 1)
OFF_WEIGHT = 65536


def target_cells(target, W):
    """(y, x) pairs -> cells y*W + x."""
    yx = np.asarray(target, np.int64).reshape(-1, 2)
    return yx[:, 0] * W + yx[:, 1]


def field(mask, cells, conn8=False):
    """(off, moves) i32 [H, W] of the minimum-cost paths from every cell to the nearest of `cells` (y*W + x)."""
    mask = np.asarray(mask) == 1
    H, W = mask.shape
    w = np.where(mask, 1, OFF_WEIGHT).astype(np.float64)
    idx = np.arange(H * W).reshape(H, W)
    rows, cols, data = [], [], []
    for dy, dx in list(zip(DY8, DX8))[:8 if conn8 else 4]:
        ys = slice(max(0, -dy), H - max(0, dy))
        xs = slice(max(0, -dx), W - max(0, dx))
        yd = slice(max(0, dy), H - max(0, -dy))
        xd = slice(max(0, dx), W - max(0, -dx))
        rows.append(idx[ys, xs].ravel())              # u
        cols.append(idx[yd, xd].ravel())              # v = u + (dy, dx)
        data.append(w[ys, xs].ravel())                # leaving u (in reverse) is what is paid for
    g = csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(H * W, H * W))
    d = dijkstra(g, directed=True, indices=np.unique(np.asarray(cells, np.int64)), min_only=True)
    assert np.isfinite(d).all()
    d = d.astype(np.int64)
    off = d // OFF_WEIGHT
    assert ((d - OFF_WEIGHT * off) < OFF_WEIGHT).all()
    return off.reshape(H, W).astype(np.int32), (d - (OFF_WEIGHT - 1) * off).reshape(H, W).astype(np.int32)


def walk(mask, off, moves, y, x, conn8=False):
    """The target path of the cell (y, x): cells y*W + x, (y, x) first; every step to the first neighbour n (DY8 / DX8
    order) with key(c) == key(n) + (mask[n] ? 0 : 1, 1). Empty outside the grid."""
    mask = np.asarray(mask) == 1
    H, W = mask.shape
    if not (0 <= y < H and 0 <= x < W):
        return np.zeros(0, np.int64)
    out = [y * W + x]
    nn = 8 if conn8 else 4
    while moves[y, x] > 0:
        for q in range(nn):
            ny, nx = y + DY8[q], x + DX8[q]
            if not (0 <= ny < H and 0 <= nx < W):
                continue
            if off[ny, nx] + (0 if mask[ny, nx] else 1) == off[y, x] and moves[ny, nx] + 1 == moves[y, x]:
                break
        else:
            raise AssertionError(f'no step from ({y}, {x}): not a fixed point')
        y, x = ny, nx
        out.append(y * W + x)
    return np.array(out, np.int64)


def path_key(mask, cells):
    """(off, moves) recomputed along a path of cells y*W + x: the cells entered after the first."""
    m = (np.asarray(mask) == 1).ravel()
    return int((~m[cells[1:]]).sum()), len(cells) - 1


def sample(off, moves, x, y):
    """The field at detections (x, y): -1 outside the grid."""
    H, W = off.shape
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    inb = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, H - 1)
    return np.where(inb, off[yc, xc], -1), np.where(inb, moves[yc, xc], -1)


# ------------------------------------------------------------------------------------------------------- masks
def serpentine_mask(H, W, channel=12, pitch=24):
    """Horizontal channels of `channel` px every `pitch` px, consecutive channels joined at alternating ends: one long
    meander from the top-left to the bottom."""
    m = np.zeros((H, W), bool)
    k = 0
    for y0 in range(0, H - channel + 1, pitch):
        m[y0:y0 + channel] = True
        if y0 + pitch + channel <= H:
            xs = slice(W - channel, W) if k % 2 == 0 else slice(0, channel)
            m[y0:y0 + pitch + channel, xs] = True
        k += 1
    return m


def blob_mask(H, W, seed=0, n_blobs=14, n_holes=10):
    """Union of seeded discs minus smaller discs: several components, with holes."""
    rng = np.random.default_rng(seed)
    Y, X = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    for _ in range(n_blobs):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(10, 34)
        m |= (Y - cy) ** 2 + (X - cx) ** 2 <= r * r
    for _ in range(n_holes):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(4, 12)
        m &= (Y - cy) ** 2 + (X - cx) ** 2 > r * r
    return m
