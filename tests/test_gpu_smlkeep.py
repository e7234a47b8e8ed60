"""Options `dd0` and `smlkeep` (tests/test_dd0_identity.py is the CPU premise).

dd0: atm_srk3's acoustic launches (reference semantics) take rw_save - rw as the constant 0.0 and load
neither column, nor X_Dd.  The setup stores rw_save = rw where the difference is read and no task of
the step writes rw, so for finite rw every field keeps its bits -- in every launch order, with every
pairing of the remaining column loads (accoef x smlsum x exact, at LP 8 and 64).

smlkeep: set_smlstep's slope-flux sum X_smlS is formed ahead of a step whose inputs may have changed
since it was last formed, not in every step.  Every public entry point but the step and the pure
queries makes the next step form it again, so a caller's new u_tend / zb_cell / zb3_cell count at
the very next step; the captured graph holds no flux launch and is captured as often as before;
decomposed contexts form the sum in every step, with the exchanges they had.
"""
import itertools

import numpy as np
import pytest

import oracle as O
from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import tasks as T
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import state as mpas_state
from test_gpu_serp import _state

pytestmark = pytest.mark.gpu

FLUX = "atm_set_smlstep_pert_variables_work[flux]"
DT = 720.0


def _run(st, nsteps, opts, schedule=1, exact=0, snaps=None, between=None):
    """the states after the steps listed in snaps (default: the last); between(ctx, n) runs after step n"""
    snaps = snaps or (nsteps,)
    out = []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("exact", exact)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.upload(st)
        for n in range(1, nsteps + 1):
            T.atm_srk3(ctx, DT, schedule)
            if n in snaps:
                ctx.sync()
                got = st.copy()
                ctx.download(got)
                out.append(got)
            if between is not None:
                between(ctx, n)
    return out


# accoef, smlsum, hfuse fully crossed; graph = accoef ^ hfuse and schedule = smlsum ^ hfuse: an
# orthogonal array of strength 2 (every pair of the five takes all four value pairs).  The load pairings
# depend on accoef, smlsum (ddx 1 / 0 with dd0 off), exact and LP, which are fully crossed
MATRIX = [(a, s, h, a ^ h, s ^ h) for a, s, h in itertools.product((0, 1), repeat=3)]


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("L", [5, 56])
def test_dd0_bit_identical(x1_2562, L, exact, variant):
    """dd0 1 against 0: every field after one and after three steps"""
    st = _state(x1_2562, L, variant)
    for accoef, smlsum, hfuse, graph, schedule in MATRIX:
        opts = dict(accoef=accoef, smlsum=smlsum, hfuse=hfuse, graph=graph)
        on = _run(st, 3, dict(opts, dd0=1), schedule, exact, snaps=(1, 3))
        off = _run(st, 3, dict(opts, dd0=0), schedule, exact, snaps=(1, 3))
        for i, n in enumerate((1, 3)):
            bad = compare_states(on[i], off[i], rtol=0.0)
            assert not bad, f"{opts} schedule={schedule} after {n} step(s): {bad[:6]}"


@pytest.mark.parametrize("fusesetup,fusedamp", [(0, 1), (1, 0), (0, 0)])
def test_dd0_other_launch_orders(x1_2562, fusesetup, fusedamp):
    """the separate setup launches and the unfused damping (plain acoustic launches, MODE 0)"""
    st = _state(x1_2562, 26, "random")
    for exact, accoef in itertools.product((0, 1), repeat=2):
        opts = dict(fusesetup=fusesetup, fusedamp=fusedamp, accoef=accoef)
        on = _run(st, 2, dict(opts, dd0=1), exact=exact, snaps=(1, 2))
        off = _run(st, 2, dict(opts, dd0=0), exact=exact, snaps=(1, 2))
        for n in range(2):
            bad = compare_states(on[n], off[n], rtol=0.0)
            assert not bad, f"{opts} exact={exact} after {n + 1} step(s): {bad[:6]}"


@pytest.mark.parametrize("dd0", [1, 0])
@pytest.mark.parametrize("hfuse", [0, 1])
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("L", [5, 56])
def test_smlkeep_bit_identical(x1_2562, L, graph, hfuse, dd0):
    """smlkeep 1 against 0 after each of three steps (a stale or missing sum shows from the second);
    without dd0 the kept X_Dd is formed from rw alone, ahead of the setup"""
    st = _state(x1_2562, L, "random")
    keep_check = 1 if (graph == 0 and hfuse == 0 and L == 56 and dd0 == 1) else 0  # (eager launches, once)
    opts = dict(graph=graph, hfuse=hfuse, dd0=dd0, keep_check=keep_check)
    on = _run(st, 3, dict(opts, smlkeep=1), snaps=(1, 2, 3))
    off = _run(st, 3, dict(opts, smlkeep=0), snaps=(1, 2, 3))
    for n in range(3):
        bad = compare_states(on[n], off[n], rtol=0.0)
        assert not bad, f"after {n + 1} step(s): {bad[:6]}"


def _toggle(name, orig, other):
    """after the first step: the option to `other`, a step, the option back"""
    def fn(ctx, n):
        if n == 1:
            ctx.set_option(name, other)
            T.atm_srk3(ctx, DT, 1)
            ctx.set_option(name, orig)
    return fn


def _upload(other, name):
    return lambda ctx, n: ctx.upload(other, names=[name]) if n == 1 else None


CHANGES = ["u_tend", "zb_cell", "zb3_cell", "fill", "signs", "core_init", "smlsum", "physics"]


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("change", CHANGES)
def test_smlkeep_invalidation(x1_2562, change, graph):
    """step; change an input of the sum (or the form of the step); two steps: all fields equal the same
    sequence with smlkeep 0"""
    L = 26
    if change == "physics":  # (the MPAS forms want mpas-mode ids)
        st = mpas_state(x1_2562, L, "mpas0")
    else:
        st = _state(x1_2562, L, "random")
    if change in ("u_tend", "zb_cell", "zb3_cell"):
        other = make_state(x1_2562, L, "random", seed=77)
        assert not np.array_equal(other[change], st[change])
        between = _upload(other, change)
    elif change == "fill":
        between = lambda ctx, n: ctx.fill_synthetic(4242) if n == 1 else None  # noqa: E731
    elif change == "signs":
        between = lambda ctx, n: T.atm_compute_signs(ctx) if n == 1 else None  # noqa: E731
    elif change == "core_init":
        between = lambda ctx, n: T.atm_core_init(ctx) if n == 1 else None  # noqa: E731
    elif change == "smlsum":
        between = _toggle("smlsum", 1, 0)
    else:
        between = _toggle("physics", 0, 1)
    on = _run(st, 3, dict(graph=graph, smlkeep=1), snaps=(1, 3), between=between)
    off = _run(st, 3, dict(graph=graph, smlkeep=0), snaps=(1, 3), between=between)
    for i in range(2):
        bad = compare_states(on[i], off[i], rtol=0.0)
        assert not bad, f"snapshot {i}: {bad[:6]}"
    if change in ("u_tend", "zb_cell", "zb3_cell", "fill"):
        # ... and the new values reached the step: without them w ends elsewhere
        plain = _run(st, 3, dict(graph=graph, smlkeep=0))
        assert not np.array_equal(plain[0]["w"], off[1]["w"], equal_nan=True)


def test_smlkeep_launch_counts(x1_2562):
    """under per-task timing: one flux launch after an upload however many steps follow; one per step
    with smlkeep 0; one more after a further upload of u_tend"""
    st = _state(x1_2562, 5, "random")
    for hfuse, smlkeep in itertools.product((0, 1), repeat=2):
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("hfuse", hfuse)
            ctx.set_option("smlkeep", smlkeep)
            ctx.upload(st)
            ctx.timing(True)
            for _ in range(3):
                T.atm_srk3(ctx, DT, 1)
            ctx.sync()
            rep = ctx.timing_report()
            if smlkeep:  # (the small grids' combined launch is then the one without the flux body)
                assert rep[FLUX][0] == 1, rep
                assert "hfuse[setup+dyn_A+sml_flux]" not in rep
                assert not hfuse or rep["hfuse[setup+dyn_A]"][0] == 3
            elif hfuse:
                assert FLUX not in rep and rep["hfuse[setup+dyn_A+sml_flux]"][0] == 3, rep
            else:
                assert rep[FLUX][0] == 3, rep
            if smlkeep:
                ctx.upload(st, names=["u_tend"])
                T.atm_srk3(ctx, DT, 1)
                ctx.sync()
                assert ctx.timing_report()[FLUX][0] == 2


def test_smlkeep_graph_counts(x1_2562):
    """the flux launch stays outside the capture: one capture per dt, one replay per step"""
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("smlkeep") == 1 and ctx.get_option("dd0") == 1  # the defaults
        ctx.upload(st)
        for dt in (720.0, 720.0, 720.0, 360.0, 360.0):
            T.atm_srk3(ctx, dt, 1)
        ctx.sync()
        assert ctx.get_option("graph_captures") == 2
        assert ctx.get_option("graph_launches") == 5


def test_smlkeep_three_subdomains(x1_2562):
    """three loopback subdomains form the sum in every step, as before: the fields of one context, the
    same exchange counts with smlkeep 0 and 1"""
    st = _state(x1_2562, 56, "random")

    def step(smlkeep):
        def fn(c):
            c.set_option("smlkeep", smlkeep)
            for _ in range(3):
                T.atm_srk3(c, DT, 1)
        return fn
    got1, stats1 = run_decomposed(st, 3, step(1), 0)
    got0, stats0 = run_decomposed(st, 3, step(0), 0)
    assert all(s[0] > 0 for s in stats1)  # the halo was exercised
    assert stats1 == stats0
    one = run_single(st, step(1), 0)
    for got in (got1, got0):
        bad = compare_states(got, one, rtol=0.0)
        assert not bad, bad[:6]


def test_option_values(x1_2562):
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        for name in ("dd0", "smlkeep"):
            assert ctx.get_option(name) == 1  # the default
            for bad in (2, -1, 3):
                with pytest.raises(lib.MpasError) as e:
                    ctx.set_option(name, bad)
                assert "(-1)" in str(e.value)  # MPAS_EINVAL
                assert ctx.get_option(name) == 1
            ctx.set_option(name, 0)
            assert ctx.get_option(name) == 0
            ctx.set_option(name, 1)
            assert ctx.get_option(name) == 1


@pytest.mark.parametrize("small_step", [0, 1])
def test_standalone_task_reads_the_stored_columns(x1_2562, small_step):
    """the standalone acoustic task with a non-zero rw_save - rw uploaded and dd0 on: the oracle's bits"""
    st = _state(x1_2562, 26, "random")
    n, L = st.nCells, st.L
    assert np.count_nonzero(st["rw_save"][:n, 1:L] - st["rw"][:n, 1:L]) > n
    ref = st.copy()
    O.Oracle(ref).atm_advance_acoustic_step_work(240.0, small_step)
    got = st.copy()
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("exact", 1)
        ctx.set_option("dd0", 1)
        ctx.upload(st)
        T.atm_advance_acoustic_step_work(ctx, 240.0, small_step)
        ctx.sync()
        ctx.download(got)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
