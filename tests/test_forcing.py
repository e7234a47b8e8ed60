"""The Held-Suarez forcing on the CPU: the library exports the task, the NumPy restatement
(tests/forcing_ref.py, the authority the GPU tests compare with) has the properties the formulas
promise on the Jablonowski-Williamson state, and a forced day on the oracle -- restatement writes
the two physics tendencies, then mpas_srk3(physics=2) reads them -- conserves dry mass, stays
finite and loses boundary-layer kinetic energy against its unforced twin (the run
tests/test_mpas_dynamics.py makes)."""
import ctypes

import numpy as np

import forcing_ref as F
import oracle as O
from helpers import SCRATCH
from mpasdyn import jw, lib
from mpasdyn import mesh as M
from mpasdyn.registry import FIELDS

L = 26
DT = 720.0


def test_abi_exports_the_task():
    assert "mpas_atm_held_suarez_forcing" in lib.EXPORTS
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "mpas_atm_held_suarez_forcing")


def jw_oracle(x1_2562):
    st = jw.jw_state(M.zero_based(x1_2562), L)
    o = O.Oracle(st)
    o.mpas_solve_diagnostics(0, -1)
    o.mpas_reconstruct_2d(False, True)
    return st, o


def test_restatement_properties_on_jw(x1_2562):
    st, o = jw_oracle(x1_2562)
    nC, nE = st.nCells, st.nEdges
    before = st.copy()
    d = F.held_suarez_forcing(st)
    # ps is the oracle's surface pressure, bit for bit
    o.mpas_surface_pressure()
    assert np.array_equal(d["ps"], st["surface_pressure"][:nC, 0])
    # only the two tendencies are written, on levels 0..L-1 of the cells / edges
    for f in FIELDS:
        if f.name not in ("tend_rtheta_physics", "tend_ru_physics", "surface_pressure"):
            assert np.array_equal(st[f.name], before[f.name], equal_nan=f.dtype == np.float64), f.name
    for name, n in (("tend_rtheta_physics", nC), ("tend_ru_physics", nE)):
        assert np.array_equal(st[name][:, L], before[name][:, L]) and np.array_equal(st[name][n], before[name][n])
    # friction: exactly zero where both cells lie above the boundary layer, elsewhere against ru
    coe = st["cellsOnEdge"][:nE]
    low = (d["sigma"][coe[:, 0]] > F.SIGMA_B) | (d["sigma"][coe[:, 1]] > F.SIGMA_B)
    tru, ru = st["tend_ru_physics"][:nE, :L], st["ru"][:nE, :L]
    assert low.any() and (~low).any()
    assert np.all(tru[~low] == 0.0)
    assert np.array_equal(np.sign(tru[low]), -np.sign(ru[low]))
    assert np.any(tru[low] != 0.0)
    # the thermal rate lies between the free-atmosphere and the surface rate
    assert d["kT"].min() >= F.K_A and d["kT"].max() <= F.K_S and d["kT"].max() > 2 * F.K_A
    # the equilibrium: at least the stratospheric floor, and a fixed point of the relaxation
    assert np.all(d["theq"] * st["exner"][:nC, :L] >= F.T_FLOOR * (1 - 1e-15))
    assert np.any(st["tend_rtheta_physics"][:nC, :L] != 0.0)
    st["theta_m"][:nC, :L] = d["theq"]
    F.held_suarez_forcing(st)
    assert np.all(st["tend_rtheta_physics"][:nC, :L] == 0.0)


def test_forced_day_on_the_oracle(x1_2562):
    """120 steps of 720 s on x1.2562 x 26.  The boundary layer: edges whose sigma_e = 0.5 (sigma(c1) +
    sigma(c2)) of the initial state exceeds sigma_b (one mask for both runs); the density at an edge
    is the mean of its two cells'."""
    st, o = jw_oracle(x1_2562)
    stu, ou = jw_oracle(x1_2562)
    nC, nE = st.nCells, st.nEdges
    vol = 1.0 / (st["invAreaCell"][:nC, 0][:, None] * st["rdzw"][:L][None, :])
    mass0 = np.sum(st["rho_zz"][:nC, :L] * vol)
    coe = st["cellsOnEdge"][:nE]
    sigma = F.held_suarez_forcing(st.copy())["sigma"]
    layer = 0.5 * (sigma[coe[:, 0]] + sigma[coe[:, 1]]) > F.SIGMA_B
    assert layer.any()

    def ke(s):
        rho = 0.5 * (s["rho_zz"][coe[:, 0], :L] + s["rho_zz"][coe[:, 1], :L])
        return float(np.sum((rho * s["u"][:nE, :L] ** 2)[layer]))
    for _ in range(int(86400 / DT)):
        F.held_suarez_forcing(st)
        o.mpas_srk3(DT, 1, physics=2)
        ou.mpas_srk3(DT, 1, physics=2)
    mass = np.sum(st["rho_zz"][:nC, :L] * vol)
    assert abs(mass / mass0 - 1.0) < 1e-12  # the forcing never touches rho
    for f in FIELDS:
        if f.dtype == np.float64 and f.name not in SCRATCH:
            assert np.isfinite(st[f.name]).all(), f.name
    ke_f, ke_u = ke(st), ke(stu)
    print(f"day 1 kinetic energy sum(rho_zz u^2) below sigma_b: forced {ke_f:.6e}, unforced {ke_u:.6e}")
    assert ke_f < ke_u
