"""NumPy restatement of the Held-Suarez (1994) forcing task, mpas_atm_held_suarez_forcing
(include/mpas_dyn.h; kernels: mpas-regent_amd/csrc/k_forcing.hip).  The authority for the task: the
two formulas in the kernels' operand order, every operation an IEEE double one, so the edge
tendency -- whose path holds no libm call -- is the kernel's bit for bit, and the cell tendency
differs by the device's log alone.  The cosine is libm's, taken per cell as the library takes it on
the host at upload.

The oracle is not touched: its mpas_srk3(physics=2) already reads the two fields, so a forced
oracle step is held_suarez_forcing(state) followed by mpas_srk3."""
import math

import numpy as np

SIGMA_B = 0.7
K_F = 1.0 / 86400.0
K_A = 1.0 / (40.0 * 86400.0)
K_S = 1.0 / (4.0 * 86400.0)
DELTA_T_Y = 60.0
DELTA_TH_Z = 10.0
T_FLOOR = 200.0
P0 = 100000.0
GRAVITY = 9.80616


def surface_pressure(st):
    """ps of the task per cell: the expression of atm_compute_output_diagnostics under physics = 2
    (level 1 of rho_zz and qtot as found: level L at L = 1)"""
    nC = st.nCells
    dz0 = 1.0 / st["rdzw"][0]
    rq0 = st["rho_zz"][:nC, 0] * (1.0 + st["qtot"][:nC, 0])
    rq1 = st["rho_zz"][:nC, 1] * (1.0 + st["qtot"][:nC, 1])
    return 0.5 * dz0 * GRAVITY * (1.25 * rq0 - 0.25 * rq1) + st["pressure_p"][:nC, 0] + st["pressure_base"][:nC, 0]


def held_suarez_forcing(st):
    """write tend_rtheta_physics and tend_ru_physics (levels 0..L-1 of the cells and edges) into st
    from the state as found; nothing else is written.  Returns the intermediates per cell and level
    (ps per cell): dict(ps, sigma, kv, kT, theq)."""
    nC, nE, L = st.nCells, st.nEdges, st.L
    c2 = np.array([math.cos(x) for x in st["lat"][:nC, 0]])
    c2 = (c2 * c2)[:, None]
    p = st["pressure_base"][:nC, :L] + st["pressure_p"][:nC, :L]
    ps = surface_pressure(st)
    sigma = p / ps[:, None]
    x = (sigma - SIGMA_B) / (1.0 - SIGMA_B)
    w = np.where(x > 0.0, x, 0.0)
    kv = K_F * w
    kT = K_A + (K_S - K_A) * w * c2 * c2
    tfl = T_FLOOR / st["exner"][:nC, :L]
    trd = 315.0 - DELTA_T_Y * (1.0 - c2) - DELTA_TH_Z * np.log(p / P0) * c2
    theq = np.where(tfl > trd, tfl, trd)
    st["tend_rtheta_physics"][:nC, :L] = -kT * st["rho_zz"][:nC, :L] * (st["theta_m"][:nC, :L] - theq)
    # kv at the two cells of each edge, ids as the library holds them (an id outside [0, n] is n; row
    # n, the zero slot that raw 1-based ids equal to n resolve to, holds zeros)
    kvz = np.zeros((nC + 1, L))
    kvz[:nC] = kv
    coe = st["cellsOnEdge"][:nE]
    coe = np.where((coe < 0) | (coe > nC), nC, coe)
    st["tend_ru_physics"][:nE, :L] = -(0.5 * (kvz[coe[:, 0]] + kvz[coe[:, 1]])) * st["ru"][:nE, :L]
    return {"ps": ps, "sigma": sigma, "kv": kv, "kT": kT, "theq": theq}
