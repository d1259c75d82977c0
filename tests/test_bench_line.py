"""CPU: the committed N = 2 rehearsal line (two slab ranks sharing one GPU,
tools/gpu_r6.sh -> profiles/r06/) carries the per-rank diagnostics a
multi-GPU bench line must explain itself with: kernel
time, the ramp and the wait for the rank below, south-inflow waits at the
slab boundary against the in-GPU ones, both halo placements and the note,
the resolved snap_every, and the bounds-guard counters.
Below: what bench.py --dump-outputs writes (on a stub context)."""
import glob
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_RANK = ("rank", "kernel_ms_last", "kernel_ms_avg", "ramp_ms", "halo_wait_ms", "south_waits_halo",
            "south_wait_ms_halo", "south_waits_local", "south_wait_ms_local", "halo_in", "halo_out",
            "halo_note", "snap_every", "bounds_guard")


def _lines():
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r06", "*", "bench_rehearse_n2.json")))
    assert paths, "no committed N = 2 rehearsal line under profiles/r06/"
    return [(p, json.loads(open(p).read().strip().splitlines()[-1])) for p in paths]


def test_rehearsal_line_has_per_rank_diagnostics():
    for path, line in _lines():
        assert line["n_gpus"] == 2 and len(line["per_rank"]) == 2, path
        for r, d in enumerate(line["per_rank"]):
            assert tuple(d) == PER_RANK or set(PER_RANK) <= set(d), (path, d)
            assert d["rank"] == r
            assert d["kernel_ms_last"] > 0 and d["ramp_ms"] > 0
            assert d["bounds_guard"]["hits"] == 0
        r0, r1 = line["per_rank"]
        # rank 0 has no inbound halo; rank 1 reads the ring rank 0 writes
        assert r0["halo_in"] is None and r0["halo_wait_ms"] == -1 and r0["south_waits_halo"] == 0
        assert r1["halo_out"] is None and r1["halo_wait_ms"] >= 0
        assert r0["halo_out"] == r1["halo_in"] is not None
        assert r0["snap_every"] == r1["snap_every"] == line["config"]["snap_every"]


def test_bench_line_reports_bounds_guard_and_build_flags():
    for path, line in _lines():
        assert line["build_id"]["flags"].endswith("knobs: none"), path
        assert line["engine"]["bounds_guard"]["hits"] == 0


# ------------------------------------------------ bench.py --dump-outputs --
class _StubCtx:
    """The three calls dump_outputs makes, on a made-up (m, count) trajectory:
    state j holds j + row / m."""

    def __init__(self, m, first, count, stride):
        self.m, self._ret = m, (first, count, stride)

    def _state(self, q):
        return q + np.arange(self.m) / self.m

    def download(self):
        f, n, k = self._ret
        return self._state(f + (n - 1) * k)

    def retained(self):
        return self._ret

    def trajectory_snaps(self, col0, ncols):
        f, n, k = self._ret
        assert 0 <= col0 and col0 + ncols <= n
        return np.stack([self._state(f + (col0 + j) * k) for j in range(ncols)], axis=1)


@pytest.mark.parametrize("m,first,count,stride", [
    (1000, 0, 4, 1),                  # small: every row, fewer states than DUMP_COLS
    ((1 << 19) + 12345, 20, 49, 10),  # sampled rows, a capped ring's strided window
])
def test_dump_outputs_files(tmp_path, m, first, count, stride):
    """--dump-outputs writes float64 .npy files well under 64 MB: the rows
    (all, or the same seeded sample every time), the final state and evenly
    spaced retained states -- first and last included -- at those rows."""
    import bench
    ctx = _StubCtx(m, first, count, stride)
    for d in ("a", "b"):
        bench.dump_outputs(ctx, str(tmp_path / d), 0, True)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["final_state", "rows", "snap_states", "snapshots"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 40e6
    for k, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{k}.npy")), k
    rows = a["rows"].astype(np.int64)
    assert len(rows) == min(m, bench.DUMP_ROWS) and np.all(np.diff(rows) > 0)
    assert 0 <= rows[0] and rows[-1] < m
    states = a["snap_states"]
    assert len(states) == min(count, bench.DUMP_COLS)
    assert states[0] == first and states[-1] == first + (count - 1) * stride
    assert np.all((states - first) % stride == 0) and np.all(np.diff(states) > 0)
    assert np.array_equal(a["snapshots"], states[None, :] + rows[:, None] / m)
    assert np.array_equal(a["final_state"], a["snapshots"][:, -1])
    # a sweep step and a rank above 0: rows and final state only, suffixed names
    bench.dump_outputs(ctx, str(tmp_path / "c"), 3, False)
    assert sorted(os.listdir(tmp_path / "c")) == ["final_state_rank3.npy", "rows_rank3.npy"]

