"""The NumPy restatement of the sigma-level statistics task (tests/stats_ref.py) and the host layer
mpasdyn/stats.py, pinned on the CPU by the properties that define them.  tests/test_gpu_sigma_stats.py
holds the device task to the restatement."""
import math

import numpy as np
import pytest

import oracle as O
import stats_ref as R
from helpers import make_state
from mpasdyn import jw, stats
from mpasdyn import mesh as M

EPS = np.finfo(float).eps
SIGMA7 = [1.0, 0.9, 0.7, 0.5, 0.3, 0.1, 0.001]


@pytest.fixture(scope="module")
def mono(x1_2562):
    """26 levels, pressures decreasing with the level (never modified)"""
    return R.decreasing_pressures(make_state(x1_2562, 26, "random").copy())


@pytest.fixture(scope="module")
def raw(x1_2562):
    """26 levels, the raw random pressures: positive everywhere, columns not monotone (never modified)"""
    return make_state(x1_2562, 26, "random")


def test_fields_affine_in_log_s_are_reproduced(mono):
    """u, v, T = A + B log s at every level give A + B log sigma_j at every sampled target.  The bound, with
    M = |A| + |B| max|log s| the size of the values: each column value A + B l is off by at most 2 eps M (a
    product and a sum); the weight a = (lsig - l0) / (l1 - l0) is three roundings of exact operands, and
    |a| <= 1 + d where d = eps max|log s| / min(l0 - l1) allows for a log rounded across the bracket's end; the
    difference, the product and the sum of x0 + a (x1 - x0) then add up to under 17 eps M (1 + d), and the
    expected value, formed the same way, to 2 eps M more: 20 eps M (1 + d)."""
    st = mono.copy()
    nC, L = st.nCells, st.L
    d = R.columns(st)
    coef = {"u": (3.0, 25.0), "v": (-7.0, 4.0), "T": (280.0, 30.0)}
    st["uReconstructZonal"][:nC, :L] = coef["u"][0] + coef["u"][1] * d["ls"]
    st["uReconstructMeridional"][:nC, :L] = coef["v"][0] + coef["v"][1] * d["ls"]
    st["theta_m"][:nC, :L] = coef["T"][0] + coef["T"][1] * d["ls"]
    st["exner"][:nC, :L] = 1.0
    smp = R.sample(st, R.DEFAULT_SIGMA)
    hit = smp["hit"]
    assert hit.mean() > 0.9
    k0 = np.where(hit, smp["kb"], 0)
    l0 = np.take_along_axis(d["ls"], k0, axis=1)
    l1 = np.take_along_axis(d["ls"], k0 + 1, axis=1)
    dl = float(np.min((l0 - l1)[hit]))
    lmax = float(np.max(np.abs(d["ls"])))
    assert dl > 0.0
    lsig = np.array([math.log(x) for x in R.DEFAULT_SIGMA])
    for name, (A, B) in coef.items():
        bound = 20.0 * EPS * (abs(A) + abs(B) * lmax) * (1.0 + EPS * lmax / dl)
        err = float(np.max(np.abs(smp[name] - (A + B * lsig[None, :]))[hit]))
        print(f"{name}: max error {err:.3e}, bound {bound:.3e} (smallest log s spacing {dl:.3e})")
        assert err <= bound


def test_targets_outside_the_column_take_no_sample(mono):
    nC = mono.nCells
    d = R.columns(mono)
    acc = R.new_acc(nC, len(SIGMA7))
    R.accumulate(acc, mono, SIGMA7)
    sg = np.array(SIGMA7)[None, :]
    above = sg > d["s"][:, :1]          # the target lies above the lowest level's s
    below = sg <= d["s"][:, -1:]        # ... at or below the highest level's
    assert above[:, 0].mean() > 0.9 and below[:, -1].all() and not below[:, :-1].any()
    out = above | below
    for name in R.STATS:
        assert np.all(acc[name][out] == 0.0), name
        assert not np.signbit(acc[name][out]).any(), name
    inside = ~out  # (the columns decrease monotonically: every target inside the column is sampled)
    assert np.all(acc["n"][inside] == 1.0) and inside.mean() > 0.5
    assert np.all(acc["ps"][:, 2] == 1.0) and np.array_equal(acc["ps"][:, 0], d["ps"])


def test_non_monotone_columns_take_the_lowest_bracket(raw):
    d = R.columns(raw)
    s = d["s"]
    assert np.all(s > 0.0)
    assert np.mean(np.any(np.diff(s, axis=1) > 0.0, axis=1)) > 0.9  # hardly a column is monotone
    sg = list(R.DEFAULT_SIGMA)
    kb = R.brackets(s, sg)
    several = 0
    for c in range(0, raw.nCells, 7):
        for j, x in enumerate(sg):
            ks = [k for k in range(raw.L - 1) if s[c, k] >= x > s[c, k + 1]]
            assert kb[c, j] == (ks[0] if ks else -1), (c, j)
            several += len(ks) > 1
    assert several > 100  # the rule was exercised: pairs with more than one qualifying bracket


def test_two_calls_add_the_sample_twice(raw):
    nC = raw.nCells
    once, twice = R.new_acc(nC, 20), R.new_acc(nC, 20)
    R.accumulate(once, raw, R.DEFAULT_SIGMA)
    R.accumulate(twice, raw, R.DEFAULT_SIGMA)
    R.accumulate(twice, raw, R.DEFAULT_SIGMA)
    assert np.any(once["n"] == 1.0)
    for name in R.STATS + ("ps",):
        assert np.array_equal(twice[name], once[name] + once[name]), name


# ---- mpasdyn.stats.zonal_means --------------------------------------------------------------------------
def _geometry(mesh):
    st = make_state(M.zero_based(mesh), 2, "physical")
    nC = st.nCells
    return st["lat"][:nC, 0].copy(), 1.0 / st["invAreaCell"][:nC, 0]


def _acc_of(u, v, T, calls=3):
    """accumulators of `calls` identical samples of per-cell values u, v, T [nC, ns]"""
    acc = R.new_acc(*u.shape)
    for _ in range(calls):
        for name, x in (("n", np.ones_like(u)), ("u", u), ("v", v), ("T", T), ("uu", u * u), ("vv", v * v),
                        ("TT", T * T), ("uv", u * v), ("vT", v * T)):
            acc[name] += x
        acc["ps"] += np.array([1.0e5, 1.0e10, 1.0])[None, :]
    return acc


def test_zonally_symmetric_field_has_no_eddies(x1_2562):
    """values constant within each band: every mean is the value to within the rounding of a weighted mean over
    the band's N cells -- (N + 2) eps relative is a bound for any summation order --, so a second moment minus
    the product of the means stays under 3 (N + 2) eps times the product of the values' magnitudes"""
    lat, area = _geometry(x1_2562)
    nb, ns = 18, 4
    band = stats.band_of(lat, nb)
    lev = 1.0 + 0.1 * np.arange(ns)[None, :]
    u = (10.0 + 3.0 * band)[:, None] * lev
    v = (-2.0 + 0.5 * band)[:, None] * lev
    T = (250.0 + 2.0 * band)[:, None] * lev
    z = stats.zonal_means(_acc_of(u, v, T), lat, area, nb)
    N = np.bincount(band, minlength=nb)[:, None]
    assert N.min() > 0
    first = lambda x: np.stack([x[band == b][0] for b in range(nb)])  # noqa: E731
    ub, vb, Tb = first(np.abs(u)), first(np.abs(v)), first(np.abs(T))
    tol = 3.0 * (N + 2) * EPS
    for name, size in (("uu", ub * ub), ("vv", vb * vb), ("TT", Tb * Tb), ("uv", ub * vb), ("vT", vb * Tb)):
        assert np.all(np.abs(z[name]) <= tol * size), name
    assert np.all(np.abs(z["T"] - first(T)) <= tol * Tb)
    assert np.all(np.abs(z["ps"] - 1.0e5) <= tol[:, 0] * 1.0e5)


def test_u_cos_lat_is_recovered_within_the_band(x1_2562):
    lat, area = _geometry(x1_2562)
    nb, ns, U = 36, 3, 30.0
    u = (U * np.cos(lat))[:, None] * np.ones((1, ns))
    z = stats.zonal_means(_acc_of(u, 0.0 * u, 0.0 * u + 1.0), lat, area, nb)
    band = stats.band_of(lat, nb)
    for b in range(nb):
        cb = np.cos(lat[band == b])
        assert cb.size  # (36 bands of the 2562-cell mesh all hold cells)
        assert np.all(z["u"][b] >= U * cb.min() * (1 - 4 * EPS)) and np.all(z["u"][b] <= U * cb.max() * (1 + 4 * EPS)), b


def test_band_without_cells_or_samples_is_nan(x1_2562):
    lat, area = _geometry(x1_2562)
    nb = 4000  # more bands than cells: most hold none
    u = np.ones((len(lat), 2))
    acc = _acc_of(u, u, u)
    acc_none = {k: v.copy() for k, v in acc.items()}
    for name in R.STATS:  # level 1 never sampled
        acc_none[name][:, 1] = 0.0
    z = stats.zonal_means(acc_none, lat, area, nb)
    empty = np.bincount(stats.band_of(lat, nb), minlength=nb) == 0
    assert empty.any() and not empty.all()
    for name in ("u", "v", "T", "uu", "vv", "TT", "uv", "vT"):
        assert np.isnan(z[name][empty]).all() and np.isnan(z[name][:, 1]).all(), name
        assert np.isfinite(z[name][~empty, 0]).all(), name
    assert np.isnan(z["ps"][empty]).all() and np.isfinite(z["ps"][~empty]).all()


def test_a_partition_changes_nothing_after_the_reorder(x1_2562, raw):
    lat, area = _geometry(x1_2562)
    nC = raw.nCells
    acc = R.new_acc(nC, 20)
    R.accumulate(acc, raw, R.DEFAULT_SIGMA)
    R.accumulate(acc, raw, R.DEFAULT_SIGMA)
    ref = stats.zonal_means(acc, lat, area, 36)
    perm = np.random.default_rng(7).permutation(nC)
    cuts = [0, nC // 3, nC // 3 + 500, nC]
    gids = [perm[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    parts = [{k: v[g] for k, v in acc.items()} for g in gids]
    got = stats.zonal_means(stats.assemble(parts, gids, nC), lat, area, 36)
    for k in ref:
        assert np.array_equal(got[k], ref[k], equal_nan=True), k


def test_jw_jet(x1_2562):
    """the balanced Jablonowski-Williamson state at 26 levels: the jet maximum of [u] lies within 1 m/s of the
    state's largest uReconstructZonal, in the latitude band that holds it.  18 bands of 10 degrees: the jets sit
    at 45 degrees, the centre of a band."""
    st = jw.jw_state(M.zero_based(x1_2562), 26, perturb=False)
    o = O.Oracle(st)
    o.mpas_solve_diagnostics(0, -1)
    o.mpas_reconstruct_2d(False, True)
    nC, L = st.nCells, st.L
    acc = R.new_acc(nC, 20)
    smp = R.accumulate(acc, st, R.DEFAULT_SIGMA)
    assert smp["hit"].mean() > 0.8
    lat, area = st["lat"][:nC, 0], 1.0 / st["invAreaCell"][:nC, 0]
    nb = 18
    z = stats.zonal_means(acc, lat, area, nb)
    uz = st["uReconstructZonal"][:nC, :L]
    cmax = int(np.argmax(uz.max(axis=1)))
    b, j = np.unravel_index(np.nanargmax(z["u"]), z["u"].shape)
    print(f"max [u] {z['u'][b, j]:.3f} m/s at band {b} ({np.degrees(z['lat'][b]):.0f} deg), sigma {R.DEFAULT_SIGMA[j]}; "
          f"max uReconstructZonal {uz.max():.3f} m/s at {np.degrees(lat[cmax]):.2f} deg")
    assert abs(z["u"][b, j] - uz.max()) <= 1.0
    assert b == stats.band_of(lat[cmax:cmax + 1], nb)[0]
