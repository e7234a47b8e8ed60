"""GPU (libmpasdyn k_forcing.hip) Held-Suarez forcing: the task mpas_atm_held_suarez_forcing against
its NumPy restatement (tests/forcing_ref.py, pinned on the CPU by tests/test_forcing.py), and option
forcing = 1 of mpas_atm_srk3.

Task parity: tend_ru_physics bit for bit (no libm call on its path); tend_rtheta_physics within the
project's per-task bound RTOL_FAST = 1e-11 of the field's maximum magnitude -- the device's log
against the host's is the only difference (a few ulp of a term of the size of theta_eq, then
multiplied by kT rho_zz like the field itself: about 1e-15 expected; the observed maximum is
printed and recorded in DESIGN.md §7).  Every other field stays bit-unchanged.

Forced steps against the oracle forced by the restatement: every field within RTOL_STEP = 1e-9
normwise, in the exact and in the benchmark path -- the bound tests/test_gpu_mpas_dynamics.py holds
whole steps of the benchmark path to, with its rule for the zero slot of rho_zz; no field is held
tighter in the exact path, as the log's ulps reach every field through tend_theta.  States: the
Jablonowski-Williamson state where it exists (it needs three levels), at one level the synthetic
0-based state.  Everything else here is bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import forcing_ref as F
import oracle as O
from helpers import ZERO_SLOT_WRITTEN, compare_states, make_state
from mpasdyn import jw, lib
from mpasdyn import mesh as M
from mpasdyn import tasks as T

pytestmark = pytest.mark.gpu

RTOL_FAST = 1e-11
RTOL_STEP = 1e-9
DT = 720.0
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "mpas-regent_amd", "mpasdyn", "libmpasdyn_bounds.so")
# ps reads level L; the smallest real column; LP 8; LP 32; the level-pair layout; level L in the last lane
LEVELS = [1, 2, 5, 26, 56, 63]
OUT = ("tend_rtheta_physics", "tend_ru_physics")

_ST = {}


def state(mesh, L, variant):
    """synthetic states, built once and never modified: "random" the raw 1-based ids (zero slot),
    "mpas0" 0-based ids, "jw" the Jablonowski-Williamson state with MPAS-A's initial diagnostics"""
    key = (L, variant)
    if key not in _ST:
        if variant == "jw":
            st = jw.jw_state(M.zero_based(mesh), L, perturb=True)
            o = O.Oracle(st)
            o.mpas_solve_diagnostics(0, -1)
            o.mpas_reconstruct_2d(False, True)
        else:
            st = make_state(M.zero_based(mesh) if variant == "mpas0" else mesh, L, "random")
        _ST[key] = st
    return _ST[key]


def gpu(st, fn, opts=None):
    got = st.copy()
    with lib.Context(*st.dims()) as ctx:
        if os.environ.get("MPAS_LIB") == BOUNDS_LIB:  # (the child run of the last test)
            assert ctx.get_option("bounds") == 1, "not the bounds-checked build"
        ctx.set_option("physics", 2)
        for k, v in (opts or {}).items():
            ctx.set_option(k, v)
        ctx.upload(st)
        fn(ctx)
        ctx.sync()
        ctx.download(got)
    return got


@pytest.mark.parametrize("variant", ["random", "mpas0"])
@pytest.mark.parametrize("L", LEVELS)
def test_task(x1_2562, L, variant):
    st = state(x1_2562, L, variant)
    ref = st.copy()
    F.held_suarez_forcing(ref)
    got = gpu(st, T.atm_held_suarez_forcing)
    nC, nE = st.nCells, st.nEdges
    assert np.any(ref["tend_ru_physics"][:nE, :L] != st["tend_ru_physics"][:nE, :L])
    assert np.array_equal(got["tend_ru_physics"], ref["tend_ru_physics"])
    err = float(np.max(np.abs(got["tend_rtheta_physics"] - ref["tend_rtheta_physics"])))
    scale = float(np.max(np.abs(ref["tend_rtheta_physics"])))
    print(f"L={L} {variant}: max|gpu - restatement| of tend_rtheta_physics = {err:.3e} = {err / scale:.3e} of its max")
    assert np.isfinite(ref["tend_rtheta_physics"]).all() and scale > 0.0
    assert err <= RTOL_FAST * scale
    # nothing else is written: every other field, and level L and the zero slot of the two outputs
    bad = compare_states(got, st, rtol=0.0, skip=set(OUT))
    assert not bad, bad[:6]
    for name, n in (("tend_rtheta_physics", nC), ("tend_ru_physics", nE)):
        assert np.array_equal(got[name][:, L], st[name][:, L]), name
        assert np.array_equal(got[name][n], st[name][n]), name


@pytest.mark.parametrize("L", [26, 56])
def test_task_on_the_jw_state(x1_2562, L):
    """the task on the state the forced steps start from: tend_ru_physics bit for bit, and
    tend_rtheta_physics off by the log alone.  The bound: the device's and the host's log are each
    within 1 ulp, |log(p / p0)| < 8 there (ulp 8.9e-16), so dthz log c2 differs by at most 1.8e-14, under
    one ulp of a theta_eq of 128 K or more (2.8e-14); the two subtractions and the product that follow
    round once each: under 8 ulp of the largest theta_eq in all, times the largest kT rho_zz, and a
    factor two of margin -- 16 eps max(kT rho_zz) max(theta_eq)."""
    st = state(x1_2562, L, "jw")
    ref = st.copy()
    d = F.held_suarez_forcing(ref)
    got = gpu(st, T.atm_held_suarez_forcing)
    nC, nE = st.nCells, st.nEdges
    assert np.any(ref["tend_ru_physics"][:nE, :L] != 0.0)
    assert np.array_equal(got["tend_ru_physics"], ref["tend_ru_physics"])
    err = float(np.max(np.abs(got["tend_rtheta_physics"] - ref["tend_rtheta_physics"])))
    scale = float(np.max(np.abs(ref["tend_rtheta_physics"])))
    bound = 16 * np.finfo(float).eps * float(np.max(d["kT"] * st["rho_zz"][:nC, :L])) * float(np.max(d["theq"]))
    print(f"L={L} jw: max|gpu - restatement| of tend_rtheta_physics = {err:.3e} = {err / scale:.3e} of its max "
          f"(bound {bound:.3e})")
    assert float(np.max(np.abs(np.log(d["sigma"] * d["ps"][:, None] / F.P0)))) < 8.0 and float(np.min(d["theq"])) >= 128.0
    assert err <= bound and err <= RTOL_FAST * scale
    bad = compare_states(got, st, rtol=0.0, skip=set(OUT))
    assert not bad, bad[:6]


def _forced(c, n=1):
    for _ in range(n):
        T.atm_srk3(c, DT, 1)


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("L", [5, 56])
def test_step_is_the_composition(x1_2562, L, exact):
    """atm_srk3 with forcing = 1 == the task, then atm_srk3 with forcing = 0: bit for bit in every field"""
    st = state(x1_2562, L, "mpas0")
    got = gpu(st, _forced, {"exact": exact, "forcing": 1})
    assert not np.array_equal(got["tend_ru_physics"], st["tend_ru_physics"])

    def composed(c):
        T.atm_held_suarez_forcing(c)
        T.atm_srk3(c, DT, 1)
    ref = gpu(st, composed, {"exact": exact, "forcing": 0})
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


def _oracle_forced(st, n):
    ref = st.copy()
    o = O.Oracle(ref)
    for _ in range(n):
        F.held_suarez_forcing(ref)
        o.mpas_srk3(DT, 1, physics=2)
    return ref


@pytest.mark.parametrize("L,variant,steps", [(5, "jw", 3), (56, "jw", 3), (1, "mpas0", 1), (63, "jw", 1)])
def test_forced_steps_against_the_oracle(x1_2562, L, variant, steps):
    st = state(x1_2562, L, variant)
    ref = _oracle_forced(st, steps)
    for exact in (1, 0):
        got = gpu(st, lambda c: _forced(c, steps), {"exact": exact, "forcing": 1})
        worst = compare_states(got, ref, rtol=1e-300, zero_slot_excluded=ZERO_SLOT_WRITTEN)
        worst = max(((e / s, n) for n, e, s in worst if s), default=(0.0, "-"))
        print(f"L={L} {variant} {steps} step(s) exact={exact}: worst field {worst[1]} at {worst[0]:.3e} of its max")
        bad = compare_states(got, ref, rtol=RTOL_STEP, zero_slot_excluded=ZERO_SLOT_WRITTEN)
        assert not bad, f"exact={exact}: {bad[:6]}"


def test_graph_replay_and_recapture(x1_2562):
    st = state(x1_2562, 26, "mpas0")
    out = {}
    for graph in (0, 1):
        got = st.copy()
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("graph", graph)
            ctx.set_option("physics", 2)
            ctx.set_option("forcing", 1)
            ctx.upload(st)
            _forced(ctx, 2)
            ctx.sync()
            assert ctx.get_option("graph_captures") == graph
            assert ctx.get_option("graph_launches") == 2 * graph
            ctx.download(got)
            if graph:
                ctx.set_option("forcing", 0)  # toggling the option: a new capture
                _forced(ctx, 1)
                ctx.sync()
                assert ctx.get_option("graph_captures") == 2
                ctx.set_option("forcing", 1)
                ctx.timing(True)  # the task appears in the per-task timing, once per step
                _forced(ctx, 1)
                ctx.sync()
                rep = ctx.timing_report()
                assert rep["atm_held_suarez_forcing"][0] == 1, rep
        out[graph] = got
    bad = compare_states(out[1], out[0], rtol=0.0)
    assert not bad, bad[:6]


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("overlap", [1, 0])
def test_decomposed_equals_single(x1_2562, nparts, overlap):
    """N loopback subdomains, two forced steps: the kv scratch is exchanged on the ghost cells"""
    from test_gpu_decomp import run_decomposed, run_single
    st = state(x1_2562, 26, "mpas0")

    def fn(c):
        c.set_option("physics", 2)
        c.set_option("forcing", 1)
        _forced(c, 2)
    ref = run_single(st, fn, 0)
    assert not np.array_equal(ref["tend_ru_physics"], st["tend_ru_physics"])
    got, stats = run_decomposed(st, nparts, fn, 0, overlap=overlap)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
    assert all(s[0] > 0 for s in stats)


def test_keep_check_forced_step(x1_2562):
    """option keep_check: every keep tail still equals its field after each task of a forced step
    (graph 0: the tasks of a captured step are not checked), and after the task called directly"""
    st = state(x1_2562, 26, "mpas0")
    gpu(st, _forced, {"graph": 0, "forcing": 1, "keep_check": 1})
    gpu(st, T.atm_held_suarez_forcing, {"keep_check": 1})


def test_option_rules(x1_2562):
    st = state(x1_2562, 5, "mpas0")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("forcing") == 0
        for physics in (0, 1):
            ctx.set_option("physics", physics)
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("forcing", 1)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
        ctx.set_option("physics", 2)
        for bad in (2, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("forcing", bad)
            assert "(-1)" in str(e.value)
        ctx.set_option("forcing", 1)
        assert ctx.get_option("forcing") == 1
        ctx.set_option("physics", 1)  # leaving the MPAS dynamics switches it off
        assert ctx.get_option("forcing") == 0
        ctx.set_option("physics", 2)
        # forcing = 0: a step leaves the two fields as uploaded
        ctx.upload(st)
        _forced(ctx, 1)
        ctx.sync()
        got = st.copy()
        ctx.download(got, names=list(OUT))
    for name in OUT:
        assert np.array_equal(got[name], st[name]), name


def test_task_parity_under_bounds_checks():
    """the task-parity cases in a child pytest on the bounds-checked build (the pattern of
    tests/test_gpu_bounds.py): neither kernel touches memory outside its fields"""
    assert os.path.exists(BOUNDS_LIB), "libmpasdyn_bounds.so missing: run __graft_entry__.build()"
    cmd = [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-k",
           "test_task and not bounds", "tests/test_gpu_forcing.py"]
    env = dict(os.environ, MPAS_LIB=BOUNDS_LIB, PYTHONUNBUFFERED="1")
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "MPAS_EBOUNDS" not in r.stdout, tail
