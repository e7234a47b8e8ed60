"""Host layer of the surface fluxes and the boundary layer (include/mpas_dyn.h, mpas_atm_surface_pbl): the
prescribed sea-surface temperatures the driver and the tools configure (mpasdyn.tasks.surface_set_temperature) and
the evaporation summary they report."""
import numpy as np


def sst_constant(T, n=None):
    """one temperature everywhere, kelvin: the number itself (tasks.surface_set_temperature takes it for every
    cell), or with n an [n] array of it"""
    T = float(T)
    if not (np.isfinite(T) and T > 0.0):
        raise ValueError(f"sst_constant: {T!r} is not a positive finite temperature")
    return T if n is None else np.full(int(n), T)


def sst_tj16(lat):
    """the sea-surface temperature of the moist Held-Suarez case of Thatcher & Jablonowski (2016), kelvin, at the
    latitudes lat (radians): 271 + 29 exp(-lat^2 / (2 (26 pi / 180)^2))"""
    lat = np.asarray(lat, dtype=np.float64)
    return 271.0 + 29.0 * np.exp(-(lat * lat) / (2.0 * (26.0 * np.pi / 180.0) ** 2))


def evap_summary(st, evap):
    """(min, max, area mean) of the accumulated evaporation, mm"""
    nC = st.nCells
    area = 1.0 / st["invAreaCell"][:nC, 0]
    evap = np.asarray(evap)
    return float(evap.min()), float(evap.max()), float(np.sum(area * evap) / np.sum(area))
