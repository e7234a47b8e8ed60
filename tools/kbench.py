#!/usr/bin/env python3
"""Per-task A/B timing in one process (cdna guide §5.4 rule 24): builds the benchmark
workload once and runs interleaved rounds of full RK3 steps under each option set,
reporting the median per-task device time (HIP events on the task stream).

usage: python tools/kbench.py [--ncells 163842] [--levels 56] [--rounds 5] [--physics N] [--transport]
       [--sigma-levels N] [--microphysics] [--pbl] --variants "xcd=1" "xcd=0"

--sigma-levels N (physics 2) configures N sigma targets of the sigma-level statistics first (the driver's
default list at 20), so that a variant may set stats_every=1 and the task's row appears.

--microphysics times the Kessler warm-rain task (physics 2) per direct launch instead of the step's rows, on two
states in interleaved rounds: "jw", the driver's moist JW state as initialised (n = 1 everywhere, the floor), and
"rain", the same with qc = qr = 2e-3 below 5 km.  What the task writes is uploaded again before every timed call,
so every round sees the same state.  Per state: the median time, the distribution of the subcycle count n, the
algorithmic bytes and TB/s, and the time per subcycle of the slowest wavefront (ms / max n).

--pbl times the surface-flux and boundary-layer task (physics 2) per direct launch on the driver's moist JW state
with MPAS-A's initial diagnostics (the cell-centre winds), over the sea-surface temperature of Thatcher &
Jablonowski (2016), in rounds interleaved with the Held-Suarez forcing task and the Kessler task on the same state
(the rows it is reported beside).  What the three tasks write is uploaded again before every timed call.  Per task:
the median time, the algorithmic bytes and the rate B_alg / time in TB/s.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mpas-regent_amd")]

import bench  # noqa: E402
from mpasdyn import lib  # noqa: E402
from mpasdyn import tasks as T  # noqa: E402


def microphysics(a):
    from mpasdyn import mesh, moist, roofline
    m = mesh.zero_based(mesh.icosahedral(bench.LEVEL_OF[a.ncells]))
    st = moist.moist_jw_state(m, a.levels)
    dt = bench.dt_for(a.ncells)
    nC, L = m.nCells, a.levels
    dry_scalars = st["scalars"].copy()
    wet_scalars = moist.add_rain(st, 2e-3, 2e-3, 5000.0)["scalars"].copy()
    out = {}
    with lib.Context(m.nCells, m.nEdges, m.nVertices, L) as ctx:
        ctx.set_option("physics", 2)
        ctx.upload(st)
        res = {"jw": [], "rain": []}
        for r in range(a.rounds + 1):  # (round 0 untimed: first launches)
            for name, sc in (("jw", dry_scalars), ("rain", wet_scalars)):
                st["scalars"][...] = sc
                ctx.upload(st, names=list(moist.KESSLER_FIELDS))
                ctx.sync()
                ctx.timing(True)
                ctx.timing_reset()
                T.atm_kessler_microphysics(ctx, dt)
                ctx.sync()
                if r:
                    res[name].append(ctx.timing_report()["atm_kessler_microphysics"][1])
                ctx.timing(False)
        b = roofline.b_alg("atm_kessler_microphysics", (m.nCells, m.nEdges, m.nVertices, L))
        for name, sc in (("jw", dry_scalars), ("rain", wet_scalars)):
            st["scalars"][...] = sc
            n = moist.subcycles(st, dt)
            ms = statistics.median(res[name])
            out[name] = {"ms": round(ms, 4), "min_ms": round(min(res[name]), 4), "rounds": len(res[name]),
                         "b_alg": b, "TBps": round(b / (ms * 1e-3) / 1e12, 3),
                         "n": {"min": int(n.min()), "median": float(np.median(n)), "mean": round(float(n.mean()), 3),
                               "max": int(n.max()), "columns_n1": int((n == 1).sum())},
                         "ms_per_subcycle_of_max_n": round(ms / int(n.max()), 5)}
    out["workload"] = f"x1.{a.ncells} x {L}, dt {dt:g}"
    print(json.dumps(out, indent=1))


def pbl(a):
    from mpasdyn import jw, mesh, moist, roofline, surface
    m = mesh.zero_based(mesh.icosahedral(bench.LEVEL_OF[a.ncells]))
    st = jw.jw_state(m, a.levels, perturb=True, subset=True,
                     extra_names=("scalars", "rt_diabatic_tend", "tend_ru_physics", "tend_rtheta_physics"))
    jw.add_moisture(st, m)
    dt = bench.dt_for(a.ncells)
    L = a.levels
    written = sorted(set(moist.KESSLER_FIELDS) | {"tend_ru_physics", "tend_rtheta_physics"})
    calls = {"atm_surface_pbl": lambda c: T.atm_surface_pbl(c, dt),
             "atm_held_suarez_forcing": T.atm_held_suarez_forcing,
             "atm_kessler_microphysics": lambda c: T.atm_kessler_microphysics(c, dt)}
    out = {}
    with lib.Context(m.nCells, m.nEdges, m.nVertices, L) as ctx:
        ctx.set_option("physics", 2)
        T.surface_set_temperature(ctx, surface.sst_tj16(np.asarray(m.latCell)))
        ctx.upload(st)
        T.atm_compute_solve_diagnostics(ctx, False, -1)
        T.mpas_reconstruct_2d(ctx, False, True)
        res = {k: [] for k in calls}
        for r in range(a.rounds + 1):  # (round 0 untimed: first launches)
            for name, fn in calls.items():
                ctx.upload(st, names=written)
                ctx.sync()
                ctx.timing(True)
                ctx.timing_reset()
                fn(ctx)
                ctx.sync()
                if r:
                    res[name].append(ctx.timing_report()[name][1])
                ctx.timing(False)
        for name in calls:
            b = roofline.b_alg(name, (m.nCells, m.nEdges, m.nVertices, L))
            ms = statistics.median(res[name])
            out[name] = {"ms": round(ms, 4), "min_ms": round(min(res[name]), 4), "rounds": len(res[name]),
                         "b_alg": b, "TBps": round(b / (ms * 1e-3) / 1e12, 3)}
    out["workload"] = f"x1.{a.ncells} x {L}, dt {dt:g}, moist JW state"
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncells", type=int, default=163842)
    ap.add_argument("--levels", type=int, default=56)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", nargs="+", default=["xcd=1", "xcd=0"])
    ap.add_argument("--physics", type=int, default=0)
    ap.add_argument("--transport", action="store_true", help="physics 1 + the scalar transport (bench --transport)")
    ap.add_argument("--sigma-levels", type=int, default=0, help="configure N sigma targets (physics 2): stats_every usable")
    ap.add_argument("--microphysics", action="store_true",
                    help="time the Kessler task per launch on the moist JW state and its rainy variant (see above)")
    ap.add_argument("--pbl", action="store_true",
                    help="time the surface-flux and boundary-layer task per launch beside the forcing and Kessler tasks (see above)")
    a = ap.parse_args()
    if a.pbl:
        return pbl(a)
    if a.microphysics:
        return microphysics(a)
    physics = max(a.physics, 1 if a.transport else 0)
    m, st = bench.build_inputs(a.ncells, a.levels, zero_based=physics)
    ctx = lib.Context(m.nCells, m.nEdges, m.nVertices, a.levels)
    ctx.set_option("physics", physics)
    ctx.set_option("transport", int(a.transport))
    if a.sigma_levels:  # N targets evenly spaced in (0, 1): 0.975, 0.925, ... at N = 20
        T.sigma_stats_configure(ctx, [1.0 - (j + 0.5) / a.sigma_levels for j in range(a.sigma_levels)])
    bench.upload_inputs(ctx, st)
    dt = bench.dt_for(a.ncells)
    T.atm_srk3(ctx, dt, 1)
    res = {v: {} for v in a.variants}
    keys = {kv.split("=")[0] for v in a.variants for kv in v.split(",")}
    base = {k: ctx.get_option(k) for k in keys}  # (a variant lists only what it changes)
    for r in range(a.rounds):
        for v in a.variants:
            for k, val in base.items():
                ctx.set_option(k, val)
            for kv in v.split(","):
                k, val = kv.split("=")
                ctx.set_option(k, int(val))
            T.atm_srk3(ctx, dt, 1)  # untimed: one-time work an option change triggers (tile builds)
            ctx.timing(True)
            ctx.timing_reset()
            T.atm_srk3(ctx, dt, 1)
            ctx.sync()
            for name, (calls, ms) in ctx.timing_report().items():
                res[v].setdefault(name, []).append(ms)
            ctx.timing(False)
    out = {}
    for v in a.variants:
        out[v] = {n: round(statistics.median(x), 4) for n, x in res[v].items()}
        out[v]["step_ms"] = round(sum(out[v].values()), 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
