"""CPU properties of the Kessler warm-rain restatement (tests/kessler_ref.py), the authority the GPU task
(libmpasdyn k_kessler.hip) is tested against in tests/test_gpu_kessler.py: the water budget, signs and idle
cells, the coverage of every branch by the generated state (asserted from the diagnostics, so that no case of the
GPU test is vacuous), the terminal velocity's closed form, the shallow columns, and mpasdyn.jw.add_moisture.
x1.2562, no GPU."""
import numpy as np
import pytest

import kessler_ref as K
from helpers import compare_states, make_state
from mpasdyn import jw
from mpasdyn import mesh as M

DT = 720.0
_C = {}


def case(mesh, L, variant="mpas0"):
    """(the generated state, the state after the task, the diagnostics), built once and never modified"""
    key = (L, variant)
    if key not in _C:
        st = K.physical_columns(make_state(M.zero_based(mesh) if variant == "mpas0" else mesh, L, "random"))
        out = st.copy()
        _C[key] = (st, out, K.kessler(out, DT))
    return _C[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("L", [5, 26])
def test_generated_state_is_physical(x1_2562, L):
    st, _, _ = case(x1_2562, L)
    nC = st.nCells
    T = st["exner"][:nC, :L] * st["theta_m"][:nC, :L] / (1.0 + K.RVORD * st["scalars"][:nC, :L, 0])
    assert T.min() >= 200.0 - 1e-9 and T.max() <= 310.0 + 1e-9
    rho_d = st["zz"][:nC, :L] * st["rho_zz"][:nC, :L]
    assert np.all(np.diff(rho_d, axis=1) < 0.0) and 1.1 < rho_d[:, 0].mean() < 1.3
    dz = 1.0 / (st["rdzw"][:L][None, :] * st["zz"][:nC, :L])
    assert dz.min() > 50.0 and dz.min() < 70.0 and dz.max() > 2500.0
    q = st["scalars"][:nC, :L, :3]
    assert q.min() == 0.0 and q[..., 1].max() <= 3e-3 and q[..., 2].max() <= 5e-3
    assert np.all(q[K.DRY(nC)] == 0.0) and np.any(q[~K.DRY(nC)] > 0.0)


@pytest.mark.parametrize("L", [5, 26, 56])
def test_water_budget(x1_2562, L):
    st, out, d = case(x1_2562, L)
    nC = st.nCells
    before, after = K.water(st), K.water(out)
    wet = ~K.DRY(nC)
    ok = wet & ~d["clip"]
    assert ok.sum() >= 0.9 * wet.sum(), (ok.sum(), wet.sum())
    rel = np.abs(before[ok] - (after[ok] + d["P"][ok])) / before[ok]
    print(f"L={L}: {ok.sum()} of {wet.sum()} wet columns unclipped; worst budget residual {rel.max():.3e}")
    assert rel.max() <= 1e-13


@pytest.mark.parametrize("L", [5, 26])
def test_signs_and_idle_cells(x1_2562, L):
    st, out, d = case(x1_2562, L)
    nC = st.nCells
    assert out["scalars"][:nC, :L, :3].min() >= 0.0
    for idle in (K.DRY(nC), K.SUBSATURATED(nC)):
        assert idle.sum() > 100
        for name in ("theta_m", "rtheta_p"):
            assert np.array_equal(bits(out[name][:nC, :L][idle]), bits(st[name][:nC, :L][idle])), name
        assert np.array_equal(bits(out["scalars"][:nC, :L, :3][idle]), bits(st["scalars"][:nC, :L, :3][idle]))
        assert np.all(bits(out["rt_diabatic_tend"][:nC, :L][idle]) == 0)  # +0.0
        assert np.all(d["P"][idle] == 0.0)
    # a cell no subcycle heated or cooled keeps theta_m, rtheta_p, qv and qc bit for bit, wherever it is
    still = ~d["cond_pos"] & ~d["cond_neg"] & (d["dsum"] == 0.0)
    assert still.sum() > K.DRY(nC).sum() * L
    for name in ("theta_m", "rtheta_p"):
        assert np.array_equal(bits(out[name][:nC, :L][still]), bits(st[name][:nC, :L][still])), name
    assert np.all(bits(out["rt_diabatic_tend"][:nC, :L][still]) == 0)
    assert np.array_equal(np.sign(d["dtheta"]), np.sign(d["dsum"]))
    assert np.any(d["dtheta"] > 0.0) and np.any(d["dtheta"] < 0.0)


def test_branch_coverage(x1_2562):
    for L in (5, 26):
        st, _, d = case(x1_2562, L)
        n = d["n"]
        assert np.any(n == 1) and np.any(n >= 3), L
        assert np.any(n[1:] != n[:-1]), L  # two columns adjacent in cell order, one wavefront below LP = 64
        # ... inside one wavefront: 64 / LP columns each
        per = 64 // (8 if L == 5 else 32)
        g = n[:len(n) // per * per].reshape(-1, per)
        assert np.any(g.max(axis=1) != g.min(axis=1)), L
        assert d["cond_pos"].any() and d["cond_neg"].any(), L
        for arm in (K.ARM_RATE, K.ARM_DEFICIT, K.ARM_RAIN):
            assert np.any(d["arm"] & arm), (L, arm)
        assert np.any(d["qc_max"] > 0.001) and np.any((d["qc_max"] < 0.001) & (d["qc_max"] > 0.0)), L
        assert not K.near_integer(d["x"]).any(), L


@pytest.mark.parametrize("L", [1, 2, 3, 5, 26, 56, 63])
@pytest.mark.parametrize("variant", ["random", "mpas0"])
def test_no_column_near_an_integer_x(x1_2562, L, variant):
    """the GPU test leaves out columns whose x lies within 1e-9 of an integer: with this seed, none"""
    _, _, d = case(x1_2562, L, variant)
    assert not K.near_integer(d["x"]).any()
    assert d["n"].max() < K.MAX_SUB


def test_rain_a_rounding_below_zero(x1_2562):
    """a rain the transport's limiter left a rounding below zero (outside the contract's qr >= 0, met in the
    driver's moist wave): the shared logarithm is -inf there, every power 0 -- no NaN anywhere, the rain
    accumulator included, and the subcycle's max(., 0) lifts the cell to 0 or above"""
    st, _, _ = case(x1_2562, 5)
    neg = st.copy()
    nC = neg.nCells
    neg["scalars"][:nC:2, 0, 2] = -1e-20
    neg["scalars"][1:nC:4, 3, 2] = -3e-19
    acc = K.new_acc(nC)
    d = K.kessler(neg, DT, acc)
    for name in K.WRITTEN:
        assert np.isfinite(neg[name]).all(), name
    assert np.isfinite(acc["rain"]).all() and np.isfinite(d["x"]).all()
    assert neg["scalars"][:nC, :5, :3].min() >= 0.0


def test_terminal_velocity():
    v = float(K.terminal_velocity(np.float64(1.2e-6), np.float64(1.1), np.float64(1.1)))
    assert abs(v - 36.34 * 1.2e-6 ** 0.1364) <= 4 * np.finfo(float).eps * v
    assert 5.6 < v < 5.8
    assert float(K.terminal_velocity(np.float64(0.0), np.float64(1.0), np.float64(1.2))) == 0.0


@pytest.mark.parametrize("L", [1, 2, 3])
def test_shallow_columns(x1_2562, L):
    st, out, d = case(x1_2562, L)
    nC = st.nCells
    assert np.isfinite(out["theta_m"][:nC, :L]).all() and np.isfinite(out["scalars"][:nC, :L, :3]).all()
    assert np.any(d["P"] > 0.0)
    if L == 1:  # the only flux is the surface's: P = sum over the subcycles of dt0 F(0), and the budget closes
        ok = ~d["clip"] & ~K.DRY(nC)
        before, after = K.water(st), K.water(out)
        assert np.max(np.abs(before[ok] - (after[ok] + d["P"][ok])) / before[ok]) <= 1e-13
    # nothing but the task's fields, and only below level L of the cells
    bad = compare_states(out, st, rtol=0.0, skip=set(K.WRITTEN))
    assert not bad, bad[:6]
    for name in K.WRITTEN:
        assert np.array_equal(out[name][nC], st[name][nC]) and np.array_equal(out[name][:, L], st[name][:, L]), name
    assert np.array_equal(out["scalars"][..., 3:], st["scalars"][..., 3:])


def test_add_moisture(x1_2562):
    m = M.zero_based(x1_2562)
    L = 26
    st = jw.add_moisture(jw.jw_state(m, L), m)
    nC = m.nCells
    qv = st["scalars"][:nC, :L, 0]
    assert np.all(st["scalars"][:nC, :L, 1:3] == 0.0)
    c, k = np.unravel_index(np.argmax(qv), qv.shape)
    assert k == 0 and abs(np.asarray(m.latCell)[c]) < np.radians(6.0)
    assert 0.0180 < qv.max() < 0.0184  # q0 / (1 - q0) = 0.01833 at the equatorial surface
    eta = (st["pressure_base"][:nC, :L] + st["pressure_p"][:nC, :L]) / st["surface_pressure"][:nC, 0][:, None]
    assert np.any(eta <= 0.1) and np.allclose(qv[eta <= 0.1], 1e-12, rtol=1e-9, atol=0.0)
    assert qv[eta > 0.1].min() > 0.0
    # supersaturation of the initial state against the restatement's qvs (a finding, recorded in DESIGN.md §7)
    pi = st["exner"][:nC, :L]
    T = pi * st["theta_m"][:nC, :L] / (1.0 + K.RVORD * qv)
    qvs = K.saturation(T, K.pc_of(pi))
    over = qv > qvs
    print(f"add_moisture at x1.2562 x {L}: {int(over.sum())} of {over.size} cells supersaturated; "
          f"largest qv / qvs {float((qv / qvs).max()):.4f}")
    assert np.isfinite(qvs).all() and np.all(qvs > 0.0)
