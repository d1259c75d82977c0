"""Row-distinct initial data and the case table of the slab / strip bitwise
tests (not a test module; imported like slab_worker, by the tests and by the
worker scripts).

From w0 = 1 a short march stays nearly constant in y away from row 0: the row
handed across a 64-row strip boundary, or across a rank boundary over the halo
ring, then has the same bits as its neighbours, and a kernel that hands over
the wrong row still passes.  wavy_state() varies in x and y everywhere;
identical_fraction() measures, on the oracle's trajectory, whether a case
could see a wrong row; tests/test_case_power.py holds every case below to
that (no GPU), and the GPU tests read the same table.
"""
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STRIP = 64  # rows of a strip (one wave per strip row block; pipe.hip kWave)
MU = (5.19, 0.026)
SWEEP_MUS = [(4.25, 0.015), (5.19, 0.026), (5.5, 0.03)]
BLIND_CAP = 0.01  # a condition on the inputs: at most 1 % of a handed-over row may repeat


def wavy_state(nx, ny):
    """[u.ravel(), v.ravel()] (reference layout, u row-major (ny, nx)), positive,
    with both y-derivatives non-zero on every row: the phase offsets keep them
    from vanishing at y = 1/4 and 3/4, the 4-rank boundaries."""
    x = ((np.arange(nx) + 0.5) / nx)[None, :]
    y = ((np.arange(ny) + 0.5) / ny)[:, None]
    u = 1 + 0.25 * np.sin(2 * np.pi * (3 * x + 0.1)) * np.cos(2 * np.pi * (2 * y + 0.13))
    v = 1 + 0.25 * np.cos(2 * np.pi * (2 * x + 0.2)) * np.sin(2 * np.pi * (5 * y + 0.07))
    return np.concatenate((u.ravel(), v.ravel()))


def slab_rows(ny, world, rank):
    from finitedifference_amd.dist import slab_rows as f
    return f(ny, world, rank)


def boundary_rows(ny, world=1):
    """Every row r > 0 that starts a 64-row strip inside some rank's slab
    (slab starts included): row r - 1 is handed over to it, through a
    mailbox inside a slab, through the halo ring between slabs."""
    out = []
    for rank in range(world):
        row0, rows = slab_rows(ny, world, rank)
        out += [row0 + k for k in range(0, rows, STRIP) if row0 + k > 0]
    return out


def identical_fraction(S, nx, ny, world=1):
    """S: step-major states (ncols, 2 nx ny).  Over every boundary row r, the
    pairs (r - 1, r - 2) and (r - 1, r), and every stored step: the largest
    fraction of columns at which the two rows agree in u and in v.  0: a
    handed-over row can be told from both neighbours everywhere."""
    S = np.asarray(S).reshape(-1, 2, ny, nx)
    rows = boundary_rows(ny, world)
    assert rows, f"no strip or slab boundary in {ny} rows over {world} ranks"
    worst = 0.0
    for r in rows:
        for o in (r - 2, r):
            if not 0 <= o < ny:
                continue
            same = (S[:, 0, r - 1] == S[:, 0, o]) & (S[:, 1, r - 1] == S[:, 1, o])
            worst = max(worst, float(same.mean(axis=1).max()))
    return worst


Slab = collections.namedtuple("Slab", "id nx ny world W T every mu dt")
Strip = collections.namedtuple("Strip", "nx ny W T mu dt")
Sweep = collections.namedtuple("Sweep", "nx ny W T mus dt")


def _wide(id, nx, ny, world, W, T, every, mu):
    return Slab(id, nx, ny, world, W, T, every, mu, 0.05 * 1024 / nx)


CASES = {
    # multi-rank slabs on one GPU (slab_worker); W = 0: the planner's width
    "slab": [
        # 64 rows per rank: every strip is a halo strip, middle ranks read and write a ring
        _wide("C1", 8192, 256, 4, 256, 40, 8, (5.19, 0.026)),
        # 83/83/82/82 rows: partial second strip, rank boundaries off the 64-row grid,
        # partial last tile (8092 = 31 * 256 + 156) against a halo ring row of ntj * W
        _wide("C2", 8092, 330, 4, 256, 40, 8, (4.25, 0.015)),
        # configs[4]'s rank count and width
        _wide("C3", 16384, 512, 8, 512, 24, 8, (5.19, 0.026)),
        # 96 rows per rank: one full strip feeding a partial halo strip
        _wide("C4", 16384, 768, 8, 512, 16, 8, (5.5, 0.03)),
        Slab("S1", 128, 128, 2, 0, 9, 1, MU, 0.05),
        Slab("S2", 150, 150, 3, 0, 7, 1, MU, 0.05),
        _wide("S3", 1024, 1024, 2, 128, 12, 1, MU),  # steady blocks
        _wide("S4", 768, 768, 3, 128, 10, 1, MU),    # half-full second workgroup
    ],
    # C1's grid through the reference API job path (job_worker slabwide)
    "job": [_wide("J1", 8192, 256, 4, 256, 40, 10, (4.25, 0.015))],
    # one process, strip boundaries inside the grid
    "strip": [
        Strip(520, 300, 64, 20, MU, 0.05),
        Strip(700, 200, 256, 20, (4.25, 0.015), 0.05),
        Strip(2100, 130, 512, 20, MU, 0.05),
        Strip(333, 129, 16, 20, (5.5, 0.03), 0.05),
        Strip(300, 300, 8, 20, MU, 0.05),
    ],
    # a sweep from a non-uniform w0: the unpaired sweep kernel
    "sweep": [Sweep(96, 200, 16, 5, SWEEP_MUS[:3], 0.05)],
}


def case_id(c):
    return c.id if hasattr(c, "id") else f"{c.nx}x{c.ny}-W{c.W}"


def problem(orc, c, mu=None):
    """The oracle's Problem of a case (Ly = 100 ny / nx: square cells)."""
    return orc.Problem(c.nx, c.ny, dt=c.dt, mu=c.mu if mu is None else mu,
                       Ly=100.0 * c.ny / c.nx, allow_nonsquare=(c.nx != c.ny))


def first_difference(snaps, ref, nx, ny, world=1):
    """None if every column of the (2 nx ny, ncols) matrix `snaps` equals the
    step-major `ref` (np.array_equal per column); else a message naming the
    first differing stored column, field, rank, slab row and column."""
    for j in range(ref.shape[0]):
        col = np.asarray(snaps[:, j])
        if np.array_equal(col, ref[j]):
            continue
        bad = np.flatnonzero(col != ref[j])
        f, rem = divmod(int(bad[0]), nx * ny)
        r, c = divmod(rem, nx)
        rank = max(k for k in range(world) if slab_rows(ny, world, k)[0] <= r)
        rows_bad = np.unique((bad % (nx * ny)) // nx)
        return (f"stored column {j}: {bad.size} entries differ, first in {'uv'[f]} at global row "
                f"{r} (rank {rank}, slab row {r - slab_rows(ny, world, rank)[0]}), column {c}: "
                f"got {col[bad[0]]!r}, want {ref[j][bad[0]]!r}; rows affected "
                f"{rows_bad[0]}..{rows_bad[-1]} ({rows_bad.size})")
    return None
