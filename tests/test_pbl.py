"""CPU properties of the surface-flux and boundary-layer restatement (tests/pbl_ref.py), the authority the GPU task
(libmpasdyn k_pbl.hip) is tested against in tests/test_gpu_pbl.py: conservation of each mixing step, the water
budget against the evaporation, the range of the mixed values, calm columns, the fixed point, the direction of the
surface step, the coverage of both arms of the two switches by the generated columns (so that no case of the GPU
test is vacuous), the edge projection and the surface-temperature helpers.  x1.2562, no GPU.

Bounds: the properties hold exactly in real arithmetic, so each bound is a rounding allowance -- the issue's 1e-14
(conservation, range) and 1e-12 (water against E), both at least ten times what a prototype of these formulas gave
on 2800 such columns (4.6e-16, 1.8e-16, 1.7e-14); the fixed point's 1e-13 allows a few roundings per level of the
two sweeps over at most 63 levels (about 500 eps)."""
import math

import numpy as np
import pytest

import pbl_ref as P
from helpers import compare_states, make_state
from mpasdyn import mesh as M
from mpasdyn import surface

LEVELS = [1, 2, 3, 5, 26, 56, 63]
DTS = [90.0, 720.0, 1800.0]
_C = {}


def gen(mesh, L, variant="mpas0"):
    """(the generated state, its surface temperatures), built once and never modified"""
    key = (L, variant)
    if key not in _C:
        _C[key] = P.physical_columns(make_state(M.zero_based(mesh) if variant == "mpas0" else mesh, L, "random"))
    return _C[key]


def cols(mesh, L, dt):
    key = (L, dt, "columns")
    if key not in _C:
        st, ts = gen(mesh, L)
        _C[key] = (P.column_inputs(st, ts), P.columns(dt, **P.column_inputs(st, ts)))
    return _C[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_generated_columns_are_physical_and_cover_both_arms(x1_2562):
    wind, pint, dz0, tsa = [], [], [], []
    for L in LEVELS:
        st, ts = gen(x1_2562, L)
        i, d = cols(x1_2562, L, 720.0)
        nC = st.nCells
        assert np.all(i["rz"] > 0.0) and np.all(i["zz"] > 0.0) and np.all(i["qv"] >= 0.0)
        T = i["pi"] * i["theta"]
        assert T.min() >= 200.0 - 1e-9 and T.max() <= 310.0 + 1e-9
        assert 9.0e4 < i["ps"].min() and i["ps"].max() < 1.3e5
        assert np.all(d["wind"][P.CALM(nC)] == 0.0) and P.CALM(nC).sum() > 300
        assert np.all(d["wind"][~P.CALM(nC)] > 0.0)
        wind.append(d["wind"])
        pint.append(d["pint"][:, 1:L].ravel())
        dz0.append(d["dz"][:, 0])
        tsa.append(ts)
    wind, pint, dz0, tsa = (np.concatenate(x) for x in (wind, pint, dz0, tsa))
    assert dz0.min() < 70.0 and dz0.max() > 1900.0
    assert wind.max() > 38.0 and (wind < 20.0).sum() > 1000 and (wind >= 20.0).sum() > 1000
    assert np.any((wind > 19.0) & (wind < 20.0)) and np.any((wind >= 20.0) & (wind < 21.0))
    assert (pint >= 85000.0).sum() > 1000 and (pint < 85000.0).sum() > 1000
    assert tsa.min() < 272.0 and tsa.max() > 301.0 and tsa.min() >= 271.0 and tsa.max() <= 302.0


def test_switches_are_continuous():
    eps = 1e-9
    assert abs(float(P.drag(np.float64(20.0 - eps))) - float(P.drag(np.float64(20.0)))) < 1e-12
    assert float(P.drag(np.float64(20.0))) == 2e-3 and float(P.drag(np.float64(45.0))) == 2e-3
    assert abs(float(P.decay(np.float64(85000.0 - 1e-3))) - 1.0) < 1e-12 and float(P.decay(np.float64(85000.0))) == 1.0
    assert 0.36 < float(P.decay(np.float64(75000.0))) < 0.37  # exp(-1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L", LEVELS)
def test_each_mixing_step_conserves(x1_2562, L, dt):
    i, d = cols(x1_2562, L, dt)
    m = d["m"]
    worst = 0.0
    for x1, x2 in ((d["u1"], d["u2"]), (d["v1"], d["v2"]), (d["th1"], d["th2"]), (d["q1"], d["q2"])):
        assert np.isfinite(x2).all()
        diff = np.abs(np.sum(m * x2, axis=1) - np.sum(m * x1, axis=1))
        scale = np.sum(m * np.abs(x1), axis=1)
        assert np.all(diff[scale == 0.0] == 0.0)
        worst = max(worst, float(np.max(diff[scale > 0.0] / scale[scale > 0.0])))
    print(f"L={L} dt={dt:g}: worst |sum m X2 - sum m X1| / sum m |X1| = {worst:.3e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L", LEVELS)
def test_column_water_change_is_the_evaporation(x1_2562, L, dt):
    i, d = cols(x1_2562, L, dt)
    m = d["m"]
    w0 = np.sum(m * i["qv"], axis=1)
    res = np.abs(np.sum(m * d["q2"], axis=1) - w0 - d["E"]) / w0
    print(f"L={L} dt={dt:g}: worst |dW - E| / W = {res.max():.3e}; E in [{d['E'].min():.3e}, {d['E'].max():.3e}] mm")
    assert res.max() <= 1e-12
    assert np.any(d["E"] > 0.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L", LEVELS)
def test_mixed_values_stay_inside_their_inputs(x1_2562, L, dt):
    i, d = cols(x1_2562, L, dt)
    worst = 0.0
    for x1, x2 in ((d["u1"], d["u2"]), (d["v1"], d["v2"]), (d["th1"], d["th2"]), (d["q1"], d["q2"])):
        lo, hi = x1.min(axis=1, keepdims=True), x1.max(axis=1, keepdims=True)
        scale = np.max(np.abs(x1), axis=1, keepdims=True)
        over = np.maximum(np.maximum(lo - x2, x2 - hi), 0.0)
        assert np.all(over[(scale == 0.0)[:, 0]] == 0.0)
        ok = (scale > 0.0)[:, 0]
        worst = max(worst, float(np.max(over[ok] / scale[ok])))
    print(f"L={L} dt={dt:g}: worst excursion outside the inputs' range = {worst:.3e} of the column's largest value")
    assert worst <= 1e-14


@pytest.mark.parametrize("L", [1, 5, 26, 63])
def test_one_level_and_mixing_do_something(x1_2562, L):
    i, d = cols(x1_2562, L, 720.0)
    if L == 1:  # the surface step alone
        for a, b in (("u1", "u2"), ("v1", "v2"), ("th1", "th2"), ("q1", "q2")):
            assert np.array_equal(bits(d[a]), bits(d[b])), a
        return
    live = ~P.CALM(len(d["wind"]))
    assert np.all(np.any(d["u2"][live] != d["u1"][live], axis=1))
    assert np.all(d["Dm"][:, 0] == 0.0) and np.all(d["Dm"][:, L] == 0.0) and np.all(d["Dm"][live, 1:L] > 0.0)
    assert np.all(d["Dh"][:, 0] == 0.0) and np.all(d["Dh"][:, L] == 0.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("L", [1, 5, 56])
def test_surface_step_moves_towards_the_surface_values(x1_2562, L, dt):
    i, d = cols(x1_2562, L, dt)
    live = ~P.CALM(len(d["wind"]))
    slack = 4.0 * np.finfo(float).eps
    for a, b in ((i["ua"], d["u1"]), (i["va"], d["v1"])):
        assert np.all(np.abs(b[:, 0]) <= np.abs(a[:, 0])) and np.all(b[:, 0] * a[:, 0] >= 0.0)
        assert np.all(np.abs(b[live, 0]) < np.abs(a[live, 0]))
        assert np.array_equal(bits(b[:, 1:]), bits(a[:, 1:]))
    for x0, x1, tgt in ((i["theta"], d["th1"], i["ts"] / i["pi"][:, 0]), (i["qv"], d["q1"], d["qss"])):
        lo, hi = np.minimum(x0[:, 0], tgt), np.maximum(x0[:, 0], tgt)
        assert np.all(x1[:, 0] >= lo * (1.0 - slack)) and np.all(x1[:, 0] <= hi * (1.0 + slack))
        moved = live & (x0[:, 0] != tgt)
        assert moved.sum() > 2000 and np.all(np.abs(x1[moved, 0] - tgt[moved]) < np.abs(x0[moved, 0] - tgt[moved]))
        assert np.array_equal(bits(x1[:, 1:]), bits(x0[:, 1:]))


@pytest.mark.parametrize("L", [1, 5, 26, 63])
def test_uniform_column_at_the_surface_values_is_a_fixed_point(x1_2562, L):
    """theta = Ts / pi(0) and qv = qss at every level: neither the surface step nor the mixing moves them"""
    i, _ = cols(x1_2562, L, 720.0)
    i = dict(i)
    i["theta"] = np.repeat((i["ts"] / i["pi"][:, 0])[:, None], L, axis=1)
    i["qv"] = np.repeat(P.qsat_surface(i["ps"], i["ts"])[:, None], L, axis=1)
    d = P.columns(1800.0, **i)
    for x0, x2 in ((i["theta"], d["th2"]), (i["qv"], d["q2"])):
        assert float(np.max(np.abs(x2 - x0) / x0)) <= 1e-13
    assert float(np.max(np.abs(d["E"]) / (d["m"][:, 0] * i["qv"][:, 0]))) <= 1e-13


@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("L", [1, 5, 26])
def test_task_on_a_state(x1_2562, L, variant):
    """calm columns keep their bits; nothing but the task's fields is written, and only below level L"""
    st, ts = gen(x1_2562, L, variant)
    out, acc = st.copy(), P.new_acc(st.nCells)
    d = P.surface_pbl(out, 720.0, ts, acc)
    nC, nE = st.nCells, st.nEdges
    calm = P.CALM(nC)
    for name in ("theta_m", "rtheta_p"):
        assert np.array_equal(bits(out[name][:nC, :L][calm]), bits(st[name][:nC, :L][calm])), name
        assert not np.array_equal(out[name][:nC, :L][~calm], st[name][:nC, :L][~calm]), name
    assert np.array_equal(bits(out["scalars"][:nC, :L, 0][calm]), bits(st["scalars"][:nC, :L, 0][calm]))
    assert np.all(bits(d["Fu"][calm]) == 0) and np.all(bits(d["Fv"][calm]) == 0) and np.all(bits(d["E"][calm]) == 0)
    assert np.all(acc["calls"] == 1.0) and np.array_equal(acc["evap"], d["E"]) and np.any(d["E"] != 0.0)
    assert np.isfinite(out["tend_ru_physics"][:nE, :L]).all() and np.any(out["tend_ru_physics"][:nE, :L] != 0.0)
    bad = compare_states(out, st, rtol=0.0, skip=set(P.WRITTEN))
    assert not bad, bad[:6]
    for name in P.WRITTEN:
        n = nE if name == "tend_ru_physics" else nC
        assert np.array_equal(out[name][n], st[name][n]) and np.array_equal(out[name][:, L], st[name][:, L]), name
    assert np.array_equal(out["scalars"][..., 1:], st["scalars"][..., 1:])


def test_uniform_vector_projects_onto_every_edge(x1_2562):
    st, _ = gen(x1_2562, 5)
    nC, nE, L = st.nCells, st.nEdges, st.L
    fu, fv = 3.25e-3, -1.5e-3
    t = P.project_edges(st, np.full((nC, L), fu), np.full((nC, L), fv))
    ang = st["angleEdge"][:nE, 0]
    want = np.array([fu * math.cos(x) + fv * math.sin(x) for x in ang])
    assert np.array_equal(bits(t), bits(np.repeat(want[:, None], L, axis=1)))
    # a zonal tendency on an edge whose normal points east is taken whole, on one pointing north not at all
    assert abs(float(t[np.argmax(np.cos(ang)), 0]) - fu) < 1e-3 * abs(fu)


def test_surface_temperatures():
    assert np.array_equal(surface.sst_constant(290.0, 4), np.full(4, 290.0))
    lat = np.array([0.0, np.radians(26.0), np.radians(90.0), -np.radians(26.0)])
    t = surface.sst_tj16(lat)
    assert t[0] == 300.0 and abs(t[1] - (271.0 + 29.0 * math.exp(-0.5))) < 1e-12 and t[1] == t[3]
    assert 271.0 < t[2] < 271.1
