"""The RK3 scalar transport (option transport = 2: two unlimited atm_advance_scalars stages over
dt/3 and dt/2, then the monotonic task with its high-order fluxes taken on the stage before) on
the CPU: tests/transport_ref.py, the NumPy restatement the GPU tests compare against, pinned
against the oracle's monotonic task and by the properties of the scheme -- a constant stays
constant for any flow, sum(rho s volume) is conserved, the unlimited stage overshoots and the
limited one does not, and three unlimited stages are third order in time."""
import os
import re

import numpy as np
import pytest

import oracle as O
import transport_ref as R
from helpers import make_state, transport_state
from test_transport import neighbourhood_bounds

DT = 600.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def only_scalars_written(out, st):
    for name, a in out.arrays.items():
        if name != "scalars":
            assert np.array_equal(a, st.arrays[name], equal_nan=True), name
    nC, L = st.nCells, st.L
    assert np.array_equal(out["scalars"][nC], st["scalars"][nC])
    assert np.array_equal(out["scalars"][:, L], st["scalars"][:, L])


def mass(rho, vol, s):
    return np.einsum("ck,cki->i", rho * vol, s)


@pytest.mark.parametrize("L", [1, 2, 5, 56])
def test_mono_rk_on_old_fluxes_matches_oracle(x1_2562, L):
    check_mono_rk_on_old_fluxes_matches_oracle(x1_2562, L)


# (each check takes the mesh: tests/test_irregular_mesh.py runs them on 4- to 8-sided cells)
def check_mono_rk_on_old_fluxes_matches_oracle(mesh, L):
    """flux source = scalars_old: the oracle's monotonic task (1e-13 normwise)"""
    st, _ = transport_state(mesh, L, DT)
    ref = st.copy()
    O.Oracle(ref).mpas_advance_scalars_mono(DT)
    got = R.advance_scalars_mono_rk(st, DT, flux_from_old=True)
    err = np.max(np.abs(got["scalars"] - ref["scalars"]))
    print(f"L={L}: max|restatement - oracle| = {err:.3e} (max|s| = {np.max(np.abs(ref['scalars'])):.3e})")
    assert err <= 1e-13 * np.max(np.abs(ref["scalars"]))
    only_scalars_written(got, st)
    # and with scalars a bit-for-bit copy of scalars_old the RK form is the same task
    st2 = st.copy()
    st2["scalars"][...] = st2["scalars_old"]
    got2 = R.advance_scalars_mono_rk(st2, DT)
    assert np.array_equal(got2["scalars"][:st.nCells, :L], got["scalars"][:st.nCells, :L])


@pytest.mark.parametrize("L", [5, 56])
def test_unlimited_stage_keeps_a_constant(x1_2562, L):
    check_unlimited_stage_keeps_a_constant(x1_2562, L)


def check_unlimited_stage_keeps_a_constant(mesh, L):
    st, _ = transport_state(mesh, L, DT, const=0.0123)
    st["scalars"][...] = st["scalars_old"]
    st["rho_zz"][...] = 1.0  # (not read: rho_int is the stage's own density)
    out, _ = R.advance_scalars(st, DT)
    s = out["scalars"][:st.nCells, :L]
    err = np.max(np.abs(s - 0.0123)) / 0.0123
    print(f"L={L}: constant kept to {err:.3e} relative")
    assert err < 1e-12
    only_scalars_written(out, st)


@pytest.mark.parametrize("L", [5, 56])
def test_unlimited_stage_conserves_and_overshoots(x1_2562, L):
    check_unlimited_stage_conserves_and_overshoots(x1_2562, L)


def check_unlimited_stage_conserves_and_overshoots(mesh, L):
    st, vol = transport_state(mesh, L, DT)
    st["scalars"][...] = st["scalars_old"]
    nC = st.nCells
    out, r_i = R.advance_scalars(st, DT)
    s_new = out["scalars"][:nC, :L]
    m_old = mass(st["rho_zz_old_split"][:nC, :L], vol, st["scalars_old"][:nC, :L])
    m_new = mass(r_i, vol, s_new)
    print(f"L={L}: mass error {np.max(np.abs(m_new / m_old - 1)):.3e}")
    assert np.allclose(m_new, m_old, rtol=1e-12, atol=0)
    lo, hi = neighbourhood_bounds(st)
    eps = 1e-13 * 0.02
    assert np.any(s_new < lo - eps) or np.any(s_new > hi + eps)  # the limiter of the last stage is not idle
    only_scalars_written(out, st)


@pytest.mark.parametrize("L", [5, 56])
def test_rk3_transport_is_monotone_and_conservative(x1_2562, L):
    check_rk3_transport_is_monotone_and_conservative(x1_2562, L)


def check_rk3_transport_is_monotone_and_conservative(mesh, L):
    st, vol = transport_state(mesh, L, DT)
    st["scalars"][...] = st["scalars_old"]
    nC = st.nCells
    out = R.rk3_transport(st, DT)
    s_new = out["scalars"][:nC, :L]
    lo, hi = neighbourhood_bounds(st)
    eps = 1e-13 * 0.02
    print(f"L={L}: worst excess over the bounds {max(np.max(lo - s_new), np.max(s_new - hi)):.3e}")
    assert np.all(s_new >= lo - eps) and np.all(s_new <= hi + eps)
    m_old = mass(st["rho_zz_old_split"][:nC, :L], vol, st["scalars_old"][:nC, :L])
    m_new = mass(out["rho_zz"][:nC, :L], vol, s_new)
    assert np.allclose(m_new, m_old, rtol=1e-12, atol=0)
    single = R.advance_scalars_mono_rk(st, DT, flux_from_old=True)
    assert np.max(np.abs(s_new - single["scalars"][:nC, :L])) > 1e-7
    for name, a in out.arrays.items():
        if name != "scalars":
            assert np.array_equal(a, st.arrays[name], equal_nan=True), name


def test_three_unlimited_stages_are_third_order(x1_2562):
    check_three_unlimited_stages_are_third_order(x1_2562)


def check_three_unlimited_stages_are_third_order(mesh):
    st0 = R.stream_flow_state(mesh, make_state)
    nC, L = st0.nCells, st0.L

    def run_steps(N, dt):
        st = st0.copy()
        for _ in range(N):
            st["scalars_old"][...] = st["scalars"]
            for f in (dt / 3, dt / 2, dt):
                st, _ = R.advance_scalars(st, f)
        return st["scalars"][:nC, :L].copy()

    ratios, d = R.convergence_ratios(run_steps)
    print(f"max|s_N - s_2N| = {d}, ratios {ratios}")
    assert all(r >= 6.0 for r in ratios), (ratios, d)


def test_abi_has_the_two_tasks():
    from mpasdyn import lib
    txt = open(os.path.join(REPO, "include", "mpas_dyn.h")).read()
    declared = set(re.findall(r"\bint\s+(mpas_\w+)\s*\(", txt))
    for name in ("mpas_atm_advance_scalars", "mpas_atm_advance_scalars_mono_rk"):
        assert name in declared, name
        assert name in lib.EXPORTS, name
