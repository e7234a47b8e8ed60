"""Host-side mirror of the reference's task interface for the RK3 hot path.

Same names, same scalar arguments in the same order as the Regent tasks
(dynamics/dynamics_tasks.rg, dynamics/rk_timestep.rg); the region arguments
(cr, cpr, er, vr, vert_r) are the device-resident state of a Context.  Errors raise
MpasError (the reference's tasks return nothing and abort on failure).
"""
from .lib import HORIZ_MIXING, MpasError


def _mix(config_horiz_mixing):
    if isinstance(config_horiz_mixing, int):
        return config_horiz_mixing
    return HORIZ_MIXING.get(config_horiz_mixing, 2)


def atm_rk_integration_setup(ctx):
    """dynamics_tasks.rg:747"""
    ctx._check(ctx.lib.mpas_atm_rk_integration_setup(ctx.h), "atm_rk_integration_setup")


def atm_compute_moist_coefficients(ctx):
    """dynamics_tasks.rg:460"""
    ctx._check(ctx.lib.mpas_atm_compute_moist_coefficients(ctx.h), "atm_compute_moist_coefficients")


def atm_compute_vert_imp_coefs(ctx, dts):
    """dynamics_tasks.rg:513"""
    ctx._check(ctx.lib.mpas_atm_compute_vert_imp_coefs(ctx.h, float(dts)), "atm_compute_vert_imp_coefs")


def atm_compute_dyn_tend_work(ctx, rk_step, dt, config_horiz_mixing="2d_smagorinsky", config_mpas_cam_coef=0.0,
                              config_mix_full=False, config_rayleigh_damp_u=False):
    """dynamics_tasks.rg:814 (constants.rg:57-60 defaults)"""
    ctx._check(ctx.lib.mpas_atm_compute_dyn_tend_work(ctx.h, int(rk_step), float(dt), _mix(config_horiz_mixing),
                                                       float(config_mpas_cam_coef), int(bool(config_mix_full)),
                                                       int(bool(config_rayleigh_damp_u))), "atm_compute_dyn_tend_work")


atm_compute_dyn_tend = atm_compute_dyn_tend_work  # :1484 wrapper


def atm_set_smlstep_pert_variables_work(ctx):
    """dynamics_tasks.rg:1503; the cpr sub-region is the cprMask field"""
    ctx._check(ctx.lib.mpas_atm_set_smlstep_pert_variables_work(ctx.h), "atm_set_smlstep_pert_variables_work")


atm_set_smlstep_pert_variables = atm_set_smlstep_pert_variables_work  # :1530 wrapper


def atm_advance_acoustic_step_work(ctx, dts, small_step):
    """dynamics_tasks.rg:1546"""
    ctx._check(ctx.lib.mpas_atm_advance_acoustic_step_work(ctx.h, float(dts), int(small_step)),
               "atm_advance_acoustic_step_work")


atm_advance_acoustic_step = atm_advance_acoustic_step_work  # :1707 wrapper


def atm_divergence_damping_3d(ctx, dts):
    """dynamics_tasks.rg:1726"""
    ctx._check(ctx.lib.mpas_atm_divergence_damping_3d(ctx.h, float(dts)), "atm_divergence_damping_3d")


def atm_compute_solve_diagnostics(ctx, hollingsworth, rk_step):
    """dynamics_tasks.rg:328"""
    ctx._check(ctx.lib.mpas_atm_compute_solve_diagnostics(ctx.h, int(bool(hollingsworth)), int(rk_step)),
               "atm_compute_solve_diagnostics")


def atm_rk_dynamics_substep_finish(ctx, dynamics_substep, dynamics_split):
    """dynamics_tasks.rg:1951"""
    ctx._check(ctx.lib.mpas_atm_rk_dynamics_substep_finish(ctx.h, int(dynamics_substep), int(dynamics_split)),
               "atm_rk_dynamics_substep_finish")


def atm_recover_large_step_variables_work(ctx, ns, rk_step, dt):
    """dynamics_tasks.rg:1766 (not called by atm_srk3: rk_timestep.rg:460, Q7)"""
    ctx._check(ctx.lib.mpas_atm_recover_large_step_variables_work(ctx.h, int(ns), int(rk_step), float(dt)),
               "atm_recover_large_step_variables_work")


atm_recover_large_step_variables = atm_recover_large_step_variables_work  # :1876 wrapper


def mpas_reconstruct_2d(ctx, includeHalos=False, on_a_sphere=True):
    """dynamics_tasks.rg:1893 (atm_core.rg:33 calls it with false, true)"""
    ctx._check(ctx.lib.mpas_reconstruct_2d(ctx.h, int(bool(includeHalos)), int(bool(on_a_sphere))),
               "mpas_reconstruct_2d")


def atm_compute_output_diagnostics(ctx):
    """dynamics_tasks.rg:729 (main.rg:70, after the time loop): rho, pressure"""
    ctx._check(ctx.lib.mpas_atm_compute_output_diagnostics(ctx.h), "atm_compute_output_diagnostics")


def atm_compute_damping_coefs(ctx, config_zd=22000.0, config_xnutr=0.2):
    """dynamics_tasks.rg:274 (atm_core_init, atm_core.rg:41; constants.rg defaults)"""
    ctx._check(ctx.lib.mpas_atm_compute_damping_coefs(ctx.h, float(config_zd), float(config_xnutr)),
               "atm_compute_damping_coefs")


def atm_init_coupled_diagnostics(ctx):
    """dynamics_tasks.rg:651 (atm_core_init, atm_core.rg:31)"""
    ctx._check(ctx.lib.mpas_atm_init_coupled_diagnostics(ctx.h), "atm_init_coupled_diagnostics")


def atm_compute_signs(ctx):
    """dynamics_tasks.rg:46 (atm_core_init, atm_core.rg:22)"""
    ctx._check(ctx.lib.mpas_atm_compute_signs(ctx.h), "atm_compute_signs")


def atm_adv_coef_compression(ctx):
    """dynamics_tasks.rg:133 (atm_core_init, atm_core.rg:24)"""
    ctx._check(ctx.lib.mpas_atm_adv_coef_compression(ctx.h), "atm_adv_coef_compression")


def atm_couple_coef_3rd_order(ctx, config_coef_3rd_order=0.25):
    """dynamics_tasks.rg:303 (atm_core_init, atm_core.rg:27; namelist 0.25)"""
    ctx._check(ctx.lib.mpas_atm_couple_coef_3rd_order(ctx.h, float(config_coef_3rd_order)),
               "atm_couple_coef_3rd_order")


def atm_compute_mesh_scaling(ctx, config_h_ScaleWithMesh=True):
    """dynamics_tasks.rg:595 (atm_core_init, atm_core.rg:39)"""
    ctx._check(ctx.lib.mpas_atm_compute_mesh_scaling(ctx.h, int(bool(config_h_ScaleWithMesh))),
               "atm_compute_mesh_scaling")


def atm_core_init(ctx):
    """atm_core.rg:22: every task of atm_core_init in order, on the device"""
    ctx._check(ctx.lib.mpas_atm_core_init(ctx.h), "atm_core_init")


def atm_advance_scalars_mono(ctx, dt):
    """Monotonic scalar transport of scalars_old into scalars over dt (SURVEY §8.7 row 4;
    no reference task exists, Q26 -- MPAS-A's atm_advance_scalars_mono; include/mpas_dyn.h)"""
    ctx._check(ctx.lib.mpas_atm_advance_scalars_mono(ctx.h, float(dt)), "atm_advance_scalars_mono")


def atm_advance_scalars(ctx, dt):
    """One unlimited stage of MPAS-A's atm_advance_scalars: scalars_old advanced over dt with the
    high-order fluxes of scalars, into scalars (the RK3 transport's first two stages;
    include/mpas_dyn.h)"""
    ctx._check(ctx.lib.mpas_atm_advance_scalars(ctx.h, float(dt)), "atm_advance_scalars")


def atm_advance_scalars_mono_rk(ctx, dt):
    """atm_advance_scalars_mono with its high-order fluxes taken on scalars, the previous stage's
    estimate (the RK3 transport's last stage; include/mpas_dyn.h)"""
    ctx._check(ctx.lib.mpas_atm_advance_scalars_mono_rk(ctx.h, float(dt)), "atm_advance_scalars_mono_rk")


def atm_held_suarez_forcing(ctx):
    """The Held-Suarez forcing: tend_rtheta_physics and tend_ru_physics from the state as found (no
    reference task; include/mpas_dyn.h, restated by tests/forcing_ref.py)"""
    ctx._check(ctx.lib.mpas_atm_held_suarez_forcing(ctx.h), "atm_held_suarez_forcing")


# ---- time-mean statistics on sigma levels (k_stats.hip; include/mpas_dyn.h, restated by tests/stats_ref.py)
STATS = ("n", "u", "v", "T", "uu", "vv", "TT", "uv", "vT")  # mpas_sigma_stats_read's stat 0..8; 9: "ps"


def sigma_stats_configure(ctx, sigma):
    """allocate and zero the accumulators for the targets `sigma` (in (0, 1], strictly decreasing, at
    most 64); an empty list frees them"""
    import numpy as np
    s = np.ascontiguousarray(sigma, dtype=np.float64).reshape(-1)
    ctx._check(ctx.lib.mpas_sigma_stats_configure(ctx.h, len(s), s.ctypes.data), "sigma_stats_configure")
    ctx._stats_ns = len(s)


def sigma_stats_reset(ctx):
    ctx._check(ctx.lib.mpas_sigma_stats_reset(ctx.h), "sigma_stats_reset")


def atm_sigma_stats_accumulate(ctx):
    """one sample of the state as found, added to the accumulators of every owned cell"""
    ctx._check(ctx.lib.mpas_atm_sigma_stats_accumulate(ctx.h), "atm_sigma_stats_accumulate")


def sigma_stats_read(ctx, n_owned=None):
    """the accumulators of the owned cells (the first n_owned local cells; default: all): a dict of
    [n_owned, nsigma] arrays under the names of STATS, and "ps" [n_owned, 3] = sum ps, sum ps^2, calls"""
    import numpy as np
    n = ctx.dims[0] if n_owned is None else int(n_owned)
    out = {}
    for i, name in enumerate(STATS + ("ps",)):
        a = np.zeros((n, 3 if name == "ps" else ctx._stats_ns))
        ctx._check(ctx.lib.mpas_sigma_stats_read(ctx.h, i, a.ctypes.data, a.strides[0], a.strides[1]),
                   f"sigma_stats_read {name}")
        out[name] = a
    return out


# ---- Kessler warm-rain microphysics (k_kessler.hip; include/mpas_dyn.h, restated by tests/kessler_ref.py)
PRECIP = ("rain", "rain_last", "calls")  # mpas_precip_read's accumulator 0..2


def atm_kessler_microphysics(ctx, dt):
    """the Kessler task over dt on the state as found: theta_m, rtheta_p, exner, pressure_p, rt_diabatic_tend
    and scalars 0..2 (qv, qc, qr) of every owned cell; the surface rain goes to the accumulators"""
    ctx._check(ctx.lib.mpas_atm_kessler_microphysics(ctx.h, float(dt)), "atm_kessler_microphysics")


def precip_read(ctx, n_owned=None):
    """the precipitation accumulators of the owned cells (the first n_owned local cells; default: all): a
    dict of [n_owned] arrays "rain" (accumulated, mm), "rain_last" (the last call's, mm) and
    "calls" (the number of calls)"""
    import numpy as np
    n = ctx.dims[0] if n_owned is None else int(n_owned)
    out = {}
    for i, name in enumerate(PRECIP):
        a = np.zeros(ctx.dims[0])  # (the call writes every owned cell)
        ctx._check(ctx.lib.mpas_precip_read(ctx.h, i, a.ctypes.data, a.strides[0]), f"precip_read {name}")
        out[name] = a[:n].copy()
    return out


def precip_reset(ctx):
    ctx._check(ctx.lib.mpas_precip_reset(ctx.h), "precip_reset")


# ---- surface fluxes and boundary layer (k_pbl.hip; include/mpas_dyn.h, restated by tests/pbl_ref.py)
SURFACE_FLUX = ("evap", "evap_last", "calls")  # mpas_surface_flux_read's accumulator 0..2


def surface_set_temperature(ctx, ts):
    """the surface temperature of the owned cells, kelvin: an array of at least the owned cells (the first
    ctx.dims[0] entries are passed; a decomposed context reads its owned ones), or one number for every cell"""
    import numpy as np
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(ts, dtype=np.float64), (ctx.dims[0],))
                             if np.ndim(ts) == 0 else np.asarray(ts, dtype=np.float64)[:ctx.dims[0]])
    if a.shape[0] < ctx.dims[0]:
        raise ValueError(f"surface_set_temperature: {a.shape[0]} values for {ctx.dims[0]} cells")
    ctx._check(ctx.lib.mpas_surface_set_temperature(ctx.h, a.ctypes.data, a.strides[0]), "surface_set_temperature")


def atm_surface_pbl(ctx, dt):
    """the surface-flux and boundary-layer task over dt on the state as found: theta_m, rtheta_p, exner,
    pressure_p and scalar 0 (qv) of every owned cell, tend_ru_physics of every owned edge; the evaporation goes
    to the accumulators"""
    ctx._check(ctx.lib.mpas_atm_surface_pbl(ctx.h, float(dt)), "atm_surface_pbl")


def surface_flux_read(ctx, n_owned=None):
    """the surface-flux accumulators of the owned cells (the first n_owned local cells; default: all): a dict
    of [n_owned] arrays "evap" (accumulated evaporation, mm), "evap_last" (the last call's, mm) and "calls" (the number of calls)"""
    import numpy as np
    n = ctx.dims[0] if n_owned is None else int(n_owned)
    out = {}
    for i, name in enumerate(SURFACE_FLUX):
        a = np.zeros(ctx.dims[0])  # (the call writes every owned cell)
        ctx._check(ctx.lib.mpas_surface_flux_read(ctx.h, i, a.ctypes.data, a.strides[0]), f"surface_flux_read {name}")
        out[name] = a[:n].copy()
    return out


def surface_flux_reset(ctx):
    ctx._check(ctx.lib.mpas_surface_flux_reset(ctx.h), "surface_flux_reset")


def summarize_timestep(ctx, config_print_detailed_minmax_vel=False, config_print_global_minmax_vel=False,
                       config_print_global_minmax_sca=False):
    """rk_timestep.rg:29; returns the 31 values the reference prints (layout: include/mpas_dyn.h)"""
    import ctypes

    import numpy as np
    out = np.zeros(31)
    ctx._check(ctx.lib.mpas_summarize_timestep(ctx.h, int(bool(config_print_detailed_minmax_vel)),
                                               int(bool(config_print_global_minmax_vel)),
                                               int(bool(config_print_global_minmax_sca)),
                                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
               "summarize_timestep")
    return out


def atm_srk3(ctx, dt, schedule=0):
    """rk_timestep.rg:361; schedule 0 = the reference's driver, 1 = rk_step 0,1,2 into dyn_tend"""
    ctx._check(ctx.lib.mpas_atm_srk3(ctx.h, float(dt), int(schedule)), "atm_srk3")


def atm_timestep(ctx, dt):
    """rk_timestep.rg:503"""
    ctx._check(ctx.lib.mpas_atm_timestep(ctx.h, float(dt)), "atm_timestep")


def atm_do_timestep(ctx, dt):
    """atm_core.rg:46; the physics stubs (atm_core.rg:64-65) write nothing the dynamics reads"""
    atm_timestep(ctx, dt)


__all__ = [n for n in dir() if n.startswith("atm_")] + ["mpas_reconstruct_2d", "summarize_timestep", "MpasError"]
