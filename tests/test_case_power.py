"""CPU: the discriminating power of the slab / strip bitwise cases
(tests/fields.py), on the oracle's trajectory -- no GPU.

A bitwise test sees a kernel that hands the wrong row across a strip or rank
boundary only if that row differs from its neighbours.  For every case of the
table: the oracle's states are finite, and at most 1 % of the columns of a
handed-over row repeat in a neighbouring row at any stored step (a condition
on the inputs, not a measurement: the wavy field gives 0).  The controls show
the metric at work on the data the older tests start from (w0 = 1).
"""
import numpy as np
import pytest

import fields

ALL = [c for kind in ("slab", "job", "strip") for c in fields.CASES[kind]]


@pytest.mark.parametrize("c", ALL, ids=fields.case_id)
def test_case_rows_are_distinct(orc, c):
    world = getattr(c, "world", 1)
    S = fields.problem(orc, c).march_traj(fields.wavy_state(c.nx, c.ny), c.T,
                                          getattr(c, "every", 1))
    assert np.isfinite(S).all()
    frac = fields.identical_fraction(S, c.nx, c.ny, world)
    print(f"{fields.case_id(c)}: identical fraction {frac:.5f}")
    assert frac <= fields.BLIND_CAP, frac


@pytest.mark.parametrize("c", fields.CASES["sweep"], ids=fields.case_id)
def test_sweep_case_rows_are_distinct(orc, c):
    for mu in c.mus:
        S = fields.problem(orc, c, mu).march_traj(fields.wavy_state(c.nx, c.ny), c.T)
        assert np.isfinite(S).all(), mu
        frac = fields.identical_fraction(S, c.nx, c.ny)
        assert frac <= fields.BLIND_CAP, (mu, frac)


def test_boundary_rows():
    assert fields.boundary_rows(300) == [64, 128, 192, 256]
    assert fields.boundary_rows(64) == []
    assert fields.boundary_rows(256, 4) == [64, 128, 192]
    # 83/83/82/82 rows: slab starts off the 64-row grid, a partial second strip each
    assert fields.boundary_rows(330, 4) == [64, 83, 147, 166, 230, 248, 312]
    assert fields.boundary_rows(128, 2) == [64]


def test_first_difference_names_the_cell():
    nx, ny, world = 8, 12, 3
    ref = np.arange(3 * 2 * nx * ny, dtype=np.float64).reshape(3, -1)
    snaps = ref.T.copy()
    assert fields.first_difference(snaps, ref, nx, ny, world) is None
    snaps[nx * ny + 9 * nx + 5, 2] += 1  # v, global row 9 = rank 2's slab row 1, column 5
    msg = fields.first_difference(snaps, ref, nx, ny, world)
    assert "stored column 2" in msg and "in v at global row 9 (rank 2, slab row 1), column 5" in msg


def test_control_uniform_start_is_blind(orc):
    """The metric on the older tests' data, after the initial state (which is
    all ones and so trivially identical): the 128^2 two-rank case (9 steps
    from w0 = 1) repeats the halo row in every column at every step; 8192 x
    256 on two ranks (3 steps) in more than 90 % of them."""
    S = orc.Problem(128).march_traj(np.ones(2 * 128 * 128), 9)
    assert fields.identical_fraction(S[1:], 128, 128, 2) == 1.0
    nx, ny = 8192, 256
    P = orc.Problem(nx, ny, dt=0.05 * 1024 / nx, Ly=100.0 * ny / nx, allow_nonsquare=True)
    S = P.march_traj(np.ones(P.m), 3)
    frac = min(fields.identical_fraction(S[j:j + 1], nx, ny, 2) for j in range(1, 4))
    print(f"8192 x 256 from w0 = 1: identical fraction {frac:.3f}")
    assert frac >= 0.9, frac
