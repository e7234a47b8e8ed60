"""Host layer of the Kessler warm-rain microphysics (include/mpas_dyn.h, mpas_atm_kessler_microphysics): what
the driver and the tools report around the device task -- the water budget, the precipitation summary, the
sedimentation subcycle count of a state, and the rainy variant of the moist JW state the measurements use."""
import numpy as np

RGAS = 287.0


def layer_mass(st):
    """m = rho_zz / rdzw per owned cell and level, kg/m2: the metric the transport conserves"""
    nC, L = st.nCells, st.L
    return st["rho_zz"][:nC, :L] / st["rdzw"][:L][None, :]


def total_water(st, rain=None):
    """sum(area m (qv + qc + qr)) + sum(area rain), kg: the budget the task and the transport close"""
    nC, L = st.nCells, st.L
    area = 1.0 / st["invAreaCell"][:nC, 0]
    q = st["scalars"][:nC, :L, 0] + st["scalars"][:nC, :L, 1] + st["scalars"][:nC, :L, 2]
    w = float(np.sum(area * np.sum(layer_mass(st) * q, axis=1)))
    return w + (float(np.sum(area * np.asarray(rain))) if rain is not None else 0.0)


def total_water_budget(st, rain=None, evap=None):
    """sum(area m (qv + qc + qr)) + sum(area (rain - evap)), kg: the budget with the surface source of the
    boundary-layer task (mpas_atm_surface_pbl) -- the water in the air, plus what rained out, minus what evaporated
    from the surface (E - P enters with its sign: a closed run keeps this sum)"""
    nC = st.nCells
    area = 1.0 / st["invAreaCell"][:nC, 0]
    w = total_water(st, rain)
    return w - (float(np.sum(area * np.asarray(evap))) if evap is not None else 0.0)


def precip_summary(st, rain):
    """(min, max, area mean) of the accumulated rain, mm"""
    nC = st.nCells
    area = 1.0 / st["invAreaCell"][:nC, 0]
    rain = np.asarray(rain)
    return float(rain.min()), float(rain.max()), float(np.sum(area * rain) / np.sum(area))


def add_rain(st, qc, qr, below):
    """cloud water qc and rain qr in every cell whose layer centre lies below `below` metres; returns st"""
    nC, L = st.nCells, st.L
    z = 0.5 * (st["zgrid"][:nC, 1:L + 1] + st["zgrid"][:nC, :L])
    low = z < below
    st["scalars"][:nC, :L, 1] = np.where(low, qc, st["scalars"][:nC, :L, 1])
    st["scalars"][:nC, :L, 2] = np.where(low, qr, st["scalars"][:nC, :L, 2])
    return st


def subcycles(st, dt):
    """the sedimentation subcycle count n the task takes per column of st at step dt (the header's x and n)"""
    nC, L = st.nCells, st.L
    zz, rz = st["zz"][:nC, :L], st["rho_zz"][:nC, :L]
    rho_d = zz * rz
    dz = 1.0 / (st["rdzw"][:L][None, :] * zz)
    y = 0.001 * rho_d * st["scalars"][:nC, :L, 2]
    lg = np.where(y > 0.0, np.log(np.where(y > 0.0, y, 1.0)), -np.inf)
    vt = 36.34 * np.exp(0.1364 * lg) * np.sqrt(rho_d[:, :1] / rho_d)
    x = np.max(vt * float(dt) / (0.8 * dz), axis=1)
    return np.where(x > 1.0, np.minimum(np.ceil(x), 4096.0), 1.0).astype(np.int64)


KESSLER_FIELDS = ("theta_m", "rtheta_p", "exner", "pressure_p", "rt_diabatic_tend", "scalars")  # what the task writes


def moist_jw_state(m0, L, subset=True):
    """the moist JW state of the driver on the 0-based mesh m0 (mpasdyn.jw.add_moisture on the perturbed JW state,
    rt_diabatic_tend = 0); subset: only the fields the state defines (large meshes)"""
    from . import jw
    st = jw.jw_state(m0, L, perturb=True, subset=subset, extra_names=("scalars", "rt_diabatic_tend"))
    jw.add_moisture(st, m0)
    st["rt_diabatic_tend"][...] = 0.0
    return st
