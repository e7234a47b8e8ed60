"""End-to-end run on the GPU, the reference's `main` (main.rg:47-76): mesh -> JW initial
state -> atm_core_init's one-time precompute -> time steps -> atm_compute_output_diagnostics
-> timestep_output.nc.

    python -m mpasdyn.driver [--grid x1.N.grid.nc] [--levels 26] [--steps 10] [--dt 720]
                             [--schedule 1] [--physics {0,1,2}] [--transport] [--day]
                             [--transport-scheme {single,rk3}] [--out timestep_output.nc]
                             [--forcing held-suarez] [--days N]
                             [--stats OUT.npz] [--stats-every N] [--stats-after-days D]
                             [--sigma-levels S0,S1,...] [--stats-bands B]
                             [--microphysics kessler] [--pbl simple] [--sst tj16|KELVIN]

Without --grid the reference's own x1.2562 mesh (tests/golden fixture) is used.  The mesh
is taken in mpas-mode (0-based) ids, the ids the JW state (mpasdyn/jw.py) is defined on.
`--schedule 0 --dt-from-step` reproduces main.rg's call literally: dt = the step index j
(Q3; j = 0 gives rdts = inf in the acoustic step, the reference's NaN).  Prints one line
per step with the reference's global min/max of w and u (summarize_timestep).
`--physics 2` runs the MPAS dynamics (every quirk of the path fixed, include/mpas_dyn.h):
the JW state then evolves as a dynamical core; the run starts from MPAS-A's initial
diagnostics (solve_diagnostics at rk_step -1 and the cell-centre winds, atm_core.rg:30-33)
and reports the surface pressure (min/max/mean, hPa) and the global dry mass after the
last step; `--day` sets the steps to one simulated day (86400 / dt).  `--transport` advects the
8 scalars: `--transport-scheme single` (default) with one monotonic update over dt, `rk3` with
MPAS-A's three-stage RK3 (option "transport" = 2, include/mpas_dyn.h).  `--forcing held-suarez`
(implies `--physics 2`) runs the Held-Suarez forcing in every step (option "forcing" = 1): Newtonian
relaxation of temperature and boundary-layer friction, the long forced integration of a dry core;
the final report then also gives the global mean temperature of the lowest level and the largest
|uReconstructZonal|.  `--days N` sets the steps to N simulated days.  `--stats OUT.npz` (needs the MPAS
dynamics: `--physics 2` or `--forcing`) accumulates time-mean statistics on sigma levels on the device
(include/mpas_dyn.h, mpas_atm_sigma_stats_accumulate): a sample after every `--stats-every`-th step (default
1) at the levels `--sigma-levels` (default 0.975, 0.925, ..., 0.025), zeroed once more after
`--stats-after-days` D simulated days of spin-up; after the last step mpasdyn.stats.zonal_means turns them
into `--stats-bands` latitude bands (default 36) of [u], [v], [T], [ps] and the eddy terms, written to
OUT.npz, and one line reports the largest [u] with its latitude and sigma and the range of [T] at the lowest
sampled level.  `--microphysics kessler` (needs `--physics 2`; implies `--transport --transport-scheme rk3`)
runs the moist baroclinic wave of DCMIP-2016: mpasdyn.jw.add_moisture puts the analytic humidity on the JW state
(here with the test case's zonal-wind perturbation, so that the wave grows),
rt_diabatic_tend starts at 0, and every step ends with the Kessler warm-rain task (option "microphysics" = 1,
include/mpas_dyn.h).  The final report gives the accumulated precipitation (min / max / area mean, mm) and the
water budget sum(area m (qv + qc + qr)) + sum(area rain) relative to its initial value; the accumulated rain goes
into the output file as `rain`.  The dynamics do not yet feel water loading, and the log says so: a smoke run,
not a validation of the DCMIP case.  `--pbl simple` (needs `--physics 2`, excludes `--forcing`; the moist JW state and
the RK3 transport with it, as `--microphysics`) ends every step with the surface-flux and boundary-layer task
(option "pbl" = 1, include/mpas_dyn.h: the simple physics of Reed & Jablonowski 2012 without its large-scale
condensation) over the sea-surface temperature `--sst`: `tj16` (default), 271 + 29 exp(-lat^2 / (2 (26 deg)^2)) of
Thatcher & Jablonowski (2016), or one temperature in kelvin.  The final report then gives the accumulated evaporation
beside the rain and the budget sum(area m (qv + qc + qr)) + sum(area (rain - evaporation)) relative to the initial
water; the accumulated evaporation goes into the output file as `evaporation`."""
import argparse
import os
import sys

import numpy as np


def run(m, L, steps, dt, schedule=1, physics=0, transport=False, dt_from_step=False, out=None, device=0,
        log=print, forcing=None, stats=None, stats_every=1, stats_after_days=0.0, sigma_levels=None, stats_bands=36,
        microphysics=None, pbl=None, sst="tj16"):
    """transport: False / 0 none, True / 1 one monotonic update per step, 2 the RK3 transport;
    forcing: None or "held-suarez" (the MPAS dynamics: physics becomes 2);
    stats: None or the .npz path the zonal-mean sigma-level statistics are written to (physics 2);
    microphysics: None or "kessler" (needs physics 2; the RK3 transport and the moist JW state with it);
    pbl: None or "simple" (needs physics 2, no forcing; the same state and transport) over the surface temperature
    sst: "tj16" or kelvin"""
    from . import build_state as bs
    from . import jw, lib, moist, surface
    from . import mesh as M
    from . import tasks as T
    from .stats import DEFAULT_SIGMA, zonal_means
    if np.asarray(m.cellsOnEdge).min() != 0:
        m = M.zero_based(m)
    st = bs.build_state(m, L, "physical", vertical=False)
    # (the moist run is the baroclinic wave: with the test case's zonal-wind perturbation, which the dry runs leave out)
    jw.init_atm_case_jw(m, st, perturb=bool(microphysics or pbl))
    if forcing not in (None, "held-suarez"):
        raise ValueError(f"unknown forcing {forcing!r}")
    if microphysics not in (None, "kessler"):
        raise ValueError(f"unknown microphysics {microphysics!r}")
    if microphysics and not forcing and int(physics or 0) != 2:
        raise ValueError("--microphysics kessler needs the MPAS dynamics (--physics 2)")
    if pbl not in (None, "simple"):
        raise ValueError(f"unknown pbl {pbl!r}")
    if pbl and (forcing or int(physics or 0) != 2):
        raise ValueError("--pbl simple needs the MPAS dynamics (--physics 2) and excludes --forcing (both write "
                         "tend_ru_physics: Rayleigh friction or the boundary layer)")
    physics = 2 if forcing else int(physics) if physics else (1 if transport else 0)
    rain = evap = None
    if microphysics or pbl:
        transport = 2
        jw.add_moisture(st, m)
        st["rt_diabatic_tend"][...] = 0.0
        water0 = moist.total_water(st)
        log(f"{'microphysics kessler' if microphysics else 'pbl simple'}: the dynamics do not feel water loading yet (qtot, cqw, cqu stay constants): "
            "a smoke run, not a validation of the DCMIP-2016 case")
    if stats and physics != 2:
        raise ValueError("--stats needs the MPAS dynamics (--physics 2 or --forcing held-suarez)")
    sigma = list(sigma_levels) if sigma_levels is not None else list(DEFAULT_SIGMA)
    reset_at = int(round(stats_after_days * 86400.0 / dt)) if stats else -1
    acc = None
    nC = m.nCells
    vol = 1.0 / (st["invAreaCell"][:nC, 0][:, None] * st["rdzw"][:L][None, :])
    mass0 = float(np.sum(st["rho_zz"][:nC, :L] * vol))
    with lib.Context(m.nCells, m.nEdges, m.nVertices, L, device=device) as ctx:
        ctx.set_option("physics", physics)
        ctx.set_option("transport", int(transport))
        if forcing:
            ctx.set_option("forcing", 1)
        if microphysics:
            ctx.set_option("microphysics", 1)
        if pbl:
            T.surface_set_temperature(ctx, surface.sst_tj16(np.asarray(m.latCell)) if sst == "tj16"
                                      else surface.sst_constant(float(sst)))
            ctx.set_option("pbl", 1)
        ctx.upload(st)
        if physics == 2:  # MPAS-A's atm_core_init diagnostics of the initial state
            T.atm_compute_solve_diagnostics(ctx, False, -1)
            T.mpas_reconstruct_2d(ctx, False, True)
        if stats:
            T.sigma_stats_configure(ctx, sigma)
            ctx.set_option("stats_every", stats_every)
        for j in range(steps):
            if j == reset_at and j > 0:  # the spin-up is over: from zero, the step count too
                T.sigma_stats_reset(ctx)
                ctx.set_option("stats_every", stats_every)
            T.atm_do_timestep(ctx, float(j) if dt_from_step else dt) if schedule == 0 else \
                T.atm_srk3(ctx, float(j) if dt_from_step else dt, schedule)
            s = T.summarize_timestep(ctx, False, True)
            log(f"step {j}: w in [{s[27]:.6g}, {s[28]:.6g}]  u in [{s[29]:.6g}, {s[30]:.6g}]")
        T.atm_compute_output_diagnostics(ctx)
        ctx.sync()
        if stats:
            acc = T.sigma_stats_read(ctx)
            samples = ctx.get_option("stats_samples")
        if microphysics:
            rain = T.precip_read(ctx)["rain"]
        if pbl:
            evap = T.surface_flux_read(ctx)["evap"]
        ctx.download(st)
    if physics == 2:
        sp = st["surface_pressure"][:nC, 0] / 100.0
        mass = float(np.sum(st["rho_zz"][:nC, :L] * vol))
        log(f"after {steps} steps ({steps * dt / 3600.0:g} h): surface pressure [{sp.min():.4f}, {sp.max():.4f}] "
            f"mean {sp.mean():.6f} hPa; dry mass change {mass / mass0 - 1.0:.3e}")
    if forcing:  # (dry: theta_m is theta, T = theta exner; the mean weighted by the cell areas)
        area = 1.0 / st["invAreaCell"][:nC, 0]
        t0 = st["theta_m"][:nC, 0] * st["exner"][:nC, 0]
        uz = np.abs(st["uReconstructZonal"][:nC, :L])
        log(f"{forcing}: lowest-level temperature mean {float(np.sum(t0 * area) / np.sum(area)):.4f} K; "
            f"max |uReconstructZonal| {float(uz.max()):.4f} m/s")
    if microphysics:
        lo, hi, mean = moist.precip_summary(st, rain)
        q = st["scalars"][:nC, :L, :3]
        log(f"kessler: accumulated precipitation min {lo:.6g} max {hi:.6g} area mean {mean:.6g} mm; "
            f"water budget change {moist.total_water(st, rain) / water0 - 1.0:.3e}; smallest qv, qc, qr "
            f"{q[..., 0].min():.3g}, {q[..., 1].min():.3g}, {q[..., 2].min():.3g}")
    if pbl:
        lo, hi, mean = surface.evap_summary(st, evap)
        uz = np.abs(st["uReconstructZonal"][:nC, :L])
        log(f"pbl: accumulated evaporation min {lo:.6g} max {hi:.6g} area mean {mean:.6g} mm; "
            f"E - P budget change {moist.total_water_budget(st, rain, evap) / water0 - 1.0:.3e}; "
            f"max |uReconstructZonal| {float(uz.max()):.4f} m/s; smallest qv {st['scalars'][:nC, :L, 0].min():.3g}")
    if stats:
        z = zonal_means(acc, st["lat"][:nC, 0], 1.0 / st["invAreaCell"][:nC, 0], stats_bands)
        np.savez(stats, sigma=np.array(sigma), samples=samples, **z)
        if np.isfinite(z["u"]).any():
            b, jm = np.unravel_index(np.nanargmax(z["u"]), z["u"].shape)
            low = int(np.nonzero(np.isfinite(z["T"]).any(axis=0))[0][0])  # (the levels decrease: the first sampled one)
            log(f"stats: {samples} samples; max [u] {z['u'][b, jm]:.4f} m/s at {np.degrees(z['lat'][b]):.1f} deg, sigma "
                f"{sigma[jm]:g}; [T] at sigma {sigma[low]:g} in [{np.nanmin(z['T'][:, low]):.4f}, "
                f"{np.nanmax(z['T'][:, low]):.4f}] K -> {stats}")
        else:
            log(f"stats: {samples} samples, no sigma level sampled -> {stats}")
    if out:
        from .meshio import write_output_plotting
        extra = dict({"rain": rain} if microphysics else {}, **({"evaporation": evap} if pbl else {}))
        write_output_plotting(out, m, st, extra=extra or None)
    return st


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--grid")
    ap.add_argument("--levels", type=int, default=26)
    ap.add_argument("--steps", type=int, default=10)  # constants.NUM_TIMESTEPS
    ap.add_argument("--dt", type=float, default=720.0)
    ap.add_argument("--schedule", type=int, default=1)
    ap.add_argument("--dt-from-step", action="store_true")
    ap.add_argument("--physics", type=int, default=0, choices=[0, 1, 2])
    ap.add_argument("--day", action="store_true", help="one simulated day: steps = 86400 / dt")
    ap.add_argument("--transport", action="store_true")
    ap.add_argument("--transport-scheme", choices=["single", "rk3"], default="single",
                    help="with --transport: one monotonic update over dt, or MPAS-A's RK3 (two unlimited stages first)")
    ap.add_argument("--forcing", choices=["held-suarez"], default=None,
                    help="held-suarez: Newtonian relaxation and boundary-layer friction in every step (implies --physics 2)")
    ap.add_argument("--days", type=float, default=None, help="N simulated days: steps = N 86400 / dt")
    ap.add_argument("--out", default="timestep_output.nc")
    ap.add_argument("--stats", default=None, metavar="OUT.npz",
                    help="time-mean zonal means and eddy terms on sigma levels, written after the last step")
    ap.add_argument("--stats-every", type=int, default=1, help="steps per sample")
    ap.add_argument("--stats-after-days", type=float, default=0.0, help="spin-up: the accumulators are zeroed after D days")
    ap.add_argument("--sigma-levels", default=None, help="comma-separated, in (0, 1], decreasing (default 0.975, ..., 0.025)")
    ap.add_argument("--stats-bands", type=int, default=36, help="latitude bands of the zonal means")
    ap.add_argument("--microphysics", choices=["kessler"], default=None,
                    help="kessler: the moist JW state and the warm-rain task at the end of every step (needs --physics 2; "
                         "implies --transport --transport-scheme rk3)")
    ap.add_argument("--pbl", choices=["simple"], default=None,
                    help="simple: bulk surface fluxes and boundary-layer mixing at the end of every step (needs --physics 2, "
                         "excludes --forcing; the moist JW state and the RK3 transport with it)")
    ap.add_argument("--sst", default="tj16", help="with --pbl: tj16 (271 + 29 exp(-lat^2 / (2 (26 deg)^2))) or kelvin")
    a = ap.parse_args(argv)
    from . import mesh as M
    if a.grid:
        from .meshio import read_grid
        m = read_grid(a.grid)
    else:
        m = M.load_x1_2562()
    steps = int(round(86400.0 / a.dt)) if a.day else a.steps
    if a.days is not None:
        steps = int(round(a.days * 86400.0 / a.dt))
    transport = (2 if a.transport_scheme == "rk3" else 1) if a.transport else 0
    sigma = [float(x) for x in a.sigma_levels.split(",")] if a.sigma_levels else None
    run(m, a.levels, steps, a.dt, a.schedule, a.physics, transport, a.dt_from_step, a.out, forcing=a.forcing,
        stats=a.stats, stats_every=a.stats_every, stats_after_days=a.stats_after_days, sigma_levels=sigma,
        stats_bands=a.stats_bands, microphysics=a.microphysics, pbl=a.pbl, sst=a.sst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
