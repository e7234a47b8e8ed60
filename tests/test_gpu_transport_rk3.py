"""GPU (libmpasdyn k_transport.hip) RK3 scalar transport: the two tasks mpas_atm_advance_scalars
and mpas_atm_advance_scalars_mono_rk against their NumPy restatement (tests/transport_ref.py,
pinned on the CPU by tests/test_transport_rk3.py), and option transport = 2 of mpas_atm_srk3.

Tolerance of the task parity: 1e-12 normwise on scalars -- about 50 roundings of 1.1e-16 on terms
of a few max|s| (the kernels evaluate the restatement's expressions in its operand order, built
with -ffp-contract=off; the observed maximum is printed and recorded in DESIGN.md §7).  Every
other field must stay bit-unchanged.  Everything else here is bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import transport_ref as R
from helpers import compare_states, make_state, transport_state
from mpasdyn import lib, tasks as T
from mpasdyn import mesh as M
from test_transport import neighbourhood_bounds

pytestmark = pytest.mark.gpu

DT = 600.0
RTOL = 1e-12
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "mpas-regent_amd", "mpasdyn", "libmpasdyn_bounds.so")
LEVELS = [1, 2, 4, 5, 26, 56, 63]  # no interface; 2nd order only; one flux3 interface; LP 8; pitch-L scratch; full column

_IN = {}


def stage_input(mesh, L, const=None):
    """transport_state with scalars the output of a first unlimited stage over dt/3 (built once per
    L, never modified); returns (state, cell volumes)"""
    key = (L, const)
    if key not in _IN:
        st, vol = transport_state(mesh, L, DT, const=const)
        st["scalars"][...] = st["scalars_old"]
        st, _ = R.advance_scalars(st, DT / 3)
        _IN[key] = (st, vol)
    return _IN[key]


def gpu(st, fn, opts=None):
    got = st.copy()
    with lib.Context(*st.dims()) as ctx:
        if os.environ.get("MPAS_LIB") == BOUNDS_LIB:  # (the child run of the last test)
            assert ctx.get_option("bounds") == 1, "not the bounds-checked build"
        ctx.set_option("physics", 1)
        for k, v in (opts or {}).items():
            ctx.set_option(k, v)
        ctx.upload(st)
        fn(ctx)
        ctx.sync()
        ctx.download(got)
    return got


def check_task(got, ref, st, what):
    err = float(np.max(np.abs(got["scalars"] - ref["scalars"])))
    scale = float(np.max(np.abs(ref["scalars"])))
    print(f"{what}: max|gpu - restatement| = {err:.3e} = {err / scale:.3e} max|s|")
    bad = compare_states(got, ref, rtol=RTOL, tol_fields={"scalars"})
    assert not bad, bad[:6]
    # only scalars is written (levels 0..L-1 of the cells)
    bad = compare_states(got, st, rtol=0.0, skip={"scalars"})
    assert not bad, bad[:6]
    assert np.array_equal(got["scalars"][:, st.L], st["scalars"][:, st.L])
    assert np.array_equal(got["scalars"][st.nCells], st["scalars"][st.nCells])


@pytest.mark.parametrize("L", LEVELS)
def test_task_stage(x1_2562, L):
    st, _ = stage_input(x1_2562, L)
    ref, _ = R.advance_scalars(st, DT / 2)
    got = gpu(st, lambda c: T.atm_advance_scalars(c, DT / 2))
    check_task(got, ref, st, f"atm_advance_scalars L={L}")


@pytest.mark.parametrize("L", LEVELS)
def test_task_mono_rk(x1_2562, L):
    st, _ = stage_input(x1_2562, L)
    ref = R.advance_scalars_mono_rk(st, DT)
    got = gpu(st, lambda c: T.atm_advance_scalars_mono_rk(c, DT))
    check_task(got, ref, st, f"atm_advance_scalars_mono_rk L={L}")


@pytest.mark.parametrize("task", ["stage", "mono_rk"])
def test_task_random_ids(x1_2562, task):
    """the literal 1-based ids of the reference's mesh (zero slot, the non-SELF gathers), every
    input synthetic"""
    st = make_state(x1_2562, 5, "random")
    if task == "stage":
        ref, _ = R.advance_scalars(st, DT)
        got = gpu(st, lambda c: T.atm_advance_scalars(c, DT))
    else:
        ref = R.advance_scalars_mono_rk(st, DT)
        got = gpu(st, lambda c: T.atm_advance_scalars_mono_rk(c, DT))
    check_task(got, ref, st, f"{task} random ids")


@pytest.mark.parametrize("trorder", [0, 1, 7, -256])
def test_task_slot_orders(x1_2562, trorder):
    """options trorder / trorder_e (negative here) apply: speed only, the same bits as the default"""
    st, _ = stage_input(x1_2562, 56)
    def both(c):
        T.atm_advance_scalars(c, DT / 2)
        T.atm_advance_scalars_mono_rk(c, DT)
    ref = gpu(st, both)
    got = gpu(st, both, {"trorder_e": -trorder} if trorder < 0 else {"trorder": trorder})
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


@pytest.mark.parametrize("L", [5, 56])
def test_mono_rk_equals_mono_on_equal_levels(x1_2562, L):
    """scalars = scalars_old bit for bit on entry: mpas_atm_advance_scalars_mono's result"""
    st, _ = transport_state(x1_2562, L, DT)
    st["scalars"][...] = st["scalars_old"]
    ref = gpu(st, lambda c: T.atm_advance_scalars_mono(c, DT))
    got = gpu(st, lambda c: T.atm_advance_scalars_mono_rk(c, DT))
    assert not np.array_equal(got["scalars"], st["scalars"])
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


def mass(rho, vol, s):
    return np.einsum("ck,cki->i", rho * vol, s)


@pytest.mark.parametrize("L", [5, 56])
def test_properties(x1_2562, L):
    """on the GPU result: the unlimited stage keeps a constant and conserves mass with rho_int as
    the new density; two stages then mono_rk stay inside the bounds of scalars_old and conserve"""
    nC = x1_2562.nCells
    stc, _ = transport_state(x1_2562, L, DT, const=0.0123)
    stc["scalars"][...] = stc["scalars_old"]
    got = gpu(stc, lambda c: T.atm_advance_scalars(c, DT))
    err = np.max(np.abs(got["scalars"][:nC, :L] - 0.0123)) / 0.0123
    print(f"L={L}: constant kept to {err:.3e} relative")
    assert err < 1e-12

    st, vol = transport_state(x1_2562, L, DT)
    st["scalars"][...] = st["scalars_old"]
    m_old = mass(st["rho_zz_old_split"][:nC, :L], vol, st["scalars_old"][:nC, :L])
    got = gpu(st, lambda c: T.atm_advance_scalars(c, DT))
    _, r_i = R.advance_scalars(st, DT)  # (rho_int is the stage's own: never stored)
    assert np.allclose(mass(r_i, vol, got["scalars"][:nC, :L]), m_old, rtol=1e-12, atol=0)

    def rk3(c):
        T.atm_advance_scalars(c, DT / 3)
        T.atm_advance_scalars(c, DT / 2)
        T.atm_advance_scalars_mono_rk(c, DT)
    got = gpu(st, rk3)
    s_new = got["scalars"][:nC, :L]
    lo, hi = neighbourhood_bounds(st)
    eps = 1e-13 * 0.02
    print(f"L={L}: worst excess over the bounds {max(np.max(lo - s_new), np.max(s_new - hi)):.3e}")
    assert np.all(s_new >= lo - eps) and np.all(s_new <= hi + eps)
    assert np.allclose(mass(got["rho_zz"][:nC, :L], vol, s_new), m_old, rtol=1e-12, atol=0)
    single = gpu(st, lambda c: T.atm_advance_scalars_mono(c, DT))
    assert np.max(np.abs(s_new - single["scalars"][:nC, :L])) > 1e-7


def test_three_stages_are_third_order(x1_2562):
    """the convergence test of tests/test_transport_rk3.py through the task API"""
    st0 = R.stream_flow_state(x1_2562, make_state)
    nC, L = st0.nCells, st0.L
    with lib.Context(*st0.dims()) as ctx:
        ctx.set_option("physics", 1)

        def run_steps(N, dt):
            st = st0.copy()
            ctx.upload(st)
            for _ in range(N):
                ctx.download(st, names=["scalars"])
                st["scalars_old"][...] = st["scalars"]
                ctx.upload(st, names=["scalars_old"])
                for f in (dt / 3, dt / 2, dt):
                    T.atm_advance_scalars(ctx, f)
            ctx.sync()
            ctx.download(st, names=["scalars"])
            return st["scalars"][:nC, :L].copy()

        ratios, d = R.convergence_ratios(run_steps)
    print(f"max|s_N - s_2N| = {d}, ratios {ratios}")
    assert all(r >= 6.0 for r in ratios), (ratios, d)


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("L", [5, 56])
def test_srk3_is_the_composition(x1_2562, L, exact):
    """atm_srk3 with transport = 2 == atm_srk3 with transport = 0, then scalars_old := the step's
    first scalars and the three task calls: bit for bit in every field (the MPAS dynamics' substep
    finish keeps rho_zz, ruAvg and wwAvg)"""
    st = make_state(M.zero_based(x1_2562), L, "random")
    dt = 720.0
    opts = {"exact": exact, "physics": 2}
    got = gpu(st, lambda c: T.atm_srk3(c, dt, 1), dict(opts, transport=2))
    assert not np.array_equal(got["scalars"], st["scalars"])

    def composed(c):
        T.atm_srk3(c, dt, 1)
        old = st.copy()
        old["scalars_old"][...] = st["scalars"]
        c.upload(old, names=["scalars_old"])
        T.atm_advance_scalars(c, dt / 3)
        T.atm_advance_scalars(c, dt / 2)
        T.atm_advance_scalars_mono_rk(c, dt)
    ref = gpu(st, composed, dict(opts, transport=0))
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
    assert np.array_equal(got["scalars_old"], st["scalars"])


def test_graph_and_timing(x1_2562):
    st = make_state(M.zero_based(x1_2562), 26, "random")
    out = {}
    for graph in (0, 1):
        got = st.copy()
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("graph", graph)
            ctx.set_option("physics", 2)
            ctx.set_option("transport", 2)
            ctx.upload(st)
            for _ in range(2):
                T.atm_srk3(ctx, 720.0, 1)
            ctx.sync()
            assert ctx.get_option("graph_captures") == graph
            assert ctx.get_option("graph_launches") == 2 * graph
            ctx.download(got)
            if graph:
                ctx.timing(True)
                T.atm_srk3(ctx, 720.0, 1)
                ctx.sync()
                rep = ctx.timing_report()
                assert rep["atm_advance_scalars"][0] == 2 and rep["atm_advance_scalars_mono_rk"][0] == 1, rep
                assert rep["scalars_save"][0] == 1 and "atm_advance_scalars_mono" not in rep
                assert ctx.get_option("graph_captures") == 1
        out[graph] = got
    bad = compare_states(out[1], out[0], rtol=0.0)
    assert not bad, bad[:6]


def test_option_rules(x1_2562):
    st, _ = stage_input(x1_2562, 5)
    with lib.Context(*st.dims()) as ctx:
        with pytest.raises(lib.MpasError):
            ctx.set_option("transport", 2)  # needs physics >= 1
        ctx.set_option("physics", 1)
        for bad in (-1, 3):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("transport", bad)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
        ctx.set_option("transport", 2)
        assert ctx.get_option("transport") == 2
        ctx.set_option("transport", 1)
        assert ctx.get_option("transport") == 1
        ctx.set_option("transport", 2)
        ctx.set_option("physics", 0)
        assert ctx.get_option("transport") == 0
        ctx.set_option("physics", 1)
        ctx.upload(st)
        for name, on, off in (("trtile", 1, 0), ("tredge", 1, 0), ("trsu", 1, 0), ("trepw", 2, 1)):
            ctx.set_option(name, on)
            for task in (T.atm_advance_scalars, T.atm_advance_scalars_mono_rk):
                with pytest.raises(lib.MpasError) as e:
                    task(ctx, DT)
                assert "(-5)" in str(e.value), str(e.value)  # MPAS_ENOTSUP
            ctx.set_option(name, off)
        T.atm_advance_scalars(ctx, DT)  # and the context still works
        ctx.sync()


def _with(opts, fn):
    def g(c):
        for k, v in opts.items():
            c.set_option(k, v)
        fn(c)
    return g


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("overlap", [1, 0])
def test_tasks_decomposed_equal_single(x1_2562, nparts, overlap):
    """N loopback subdomains: scalars is exchanged over the adv-list rings like scalars_old"""
    from test_gpu_decomp import run_decomposed, run_single
    st, _ = stage_input(x1_2562, 56)
    for fn in (lambda c: T.atm_advance_scalars(c, DT / 2), lambda c: T.atm_advance_scalars_mono_rk(c, DT)):
        f = _with({"physics": 1}, fn)
        ref = run_single(st, f, 1)
        got, stats = run_decomposed(st, nparts, f, 1, overlap=overlap)
        bad = compare_states(got, ref, rtol=0.0)
        assert not bad, bad[:6]
        assert all(s[0] > 0 for s in stats)


@pytest.mark.parametrize("nparts", [2, 3])
@pytest.mark.parametrize("overlap", [1, 0])
def test_srk3_decomposed_equals_single(x1_2562, nparts, overlap):
    from test_gpu_decomp import run_decomposed, run_single
    st = make_state(M.zero_based(x1_2562), 26, "random")
    def two_steps(c):
        for _ in range(2):
            T.atm_srk3(c, 720.0, 1)
    fn = _with({"physics": 2, "transport": 2}, two_steps)
    ref = run_single(st, fn, 0)
    got, _ = run_decomposed(st, nparts, fn, 0, overlap=overlap)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]


def test_keep_check_step(x1_2562):
    """option keep_check: every keep tail still equals its field after each task of the step"""
    st = make_state(M.zero_based(x1_2562), 26, "random")
    gpu(st, lambda c: T.atm_srk3(c, 720.0, 1), {"physics": 2, "transport": 2, "keep_check": 1})


def test_task_parity_under_bounds_checks():
    """the task-parity tests above in a child pytest on the bounds-checked build (the pattern of
    tests/test_gpu_bounds.py): no kernel of the two tasks touches memory outside its fields"""
    assert os.path.exists(BOUNDS_LIB), "libmpasdyn_bounds.so missing: run __graft_entry__.build()"
    cmd = [sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-k",
           "test_task_stage or test_task_mono_rk or test_task_random_ids", "tests/test_gpu_transport_rk3.py"]
    env = dict(os.environ, MPAS_LIB=BOUNDS_LIB, PYTHONUNBUFFERED="1")
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "MPAS_EBOUNDS" not in r.stdout, tail
