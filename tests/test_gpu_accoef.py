"""Option `accoef`: atm_srk3's acoustic launches form cofwr, coftz and a_tri from the
columns they hold (zz, theta_m, cofwz, cofwt) instead of loading the three stored columns; stage 0's
setup launch then leaves the three unstored (stage 1's vert_imp stores them), and vert_imp takes
coftz's level L from the field's keep tail instead of loading the column.

The expressions are vert_imp's own, in its order (tests/test_accoef_identity.py is the CPU premise),
so every field must have the same bits with the option on and off -- after one step and after two:
with stage 0's stores skipped, a stage-0 launch that still read a stored column would see the previous
step's dt/2 values in the second step.  The MPAS forms (physics 1 / 2) are left as they were: the
option changes nothing there.  The standalone acoustic task always reads the stored columns.
"""
import numpy as np
import pytest

from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import tasks as T
from test_gpu_decomp import run_decomposed, run_single
from test_gpu_mpas_dynamics import state as mpas_state
from test_gpu_serp import _state, _steps

pytestmark = pytest.mark.gpu

COLS = ("cofwr", "coftz", "a_tri")


@pytest.mark.parametrize("schedule", [0, 1])
@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("L", [5, 26, 56])
def test_accoef_bit_identical(x1_2562, L, exact, variant, schedule):
    """accoef 1 against 0 after one and after two steps, every field, in each launch order (hfuse 0 / 1)
    and both as a replayed graph and eagerly"""
    st = _state(x1_2562, L, variant)

    def steps(**opts):
        out = []
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("exact", exact)
            for k, v in opts.items():
                ctx.set_option(k, v)
            ctx.upload(st)
            for _ in range(2):
                T.atm_srk3(ctx, 720.0, schedule)
                ctx.sync()
                got = st.copy()
                ctx.download(got)
                out.append(got)
        return out

    for hfuse in (0, 1):
        for graph in (0, 1):
            on = steps(hfuse=hfuse, graph=graph, accoef=1)
            off = steps(hfuse=hfuse, graph=graph, accoef=0)
            for n in range(2):
                bad = compare_states(on[n], off[n], rtol=0.0)
                assert not bad, f"hfuse={hfuse} graph={graph} after {n + 1} step(s): {bad[:6]}"


@pytest.mark.parametrize("fusesetup,fusedamp", [(0, 1), (1, 0), (0, 0)])
def test_accoef_other_launch_orders(x1_2562, fusesetup, fusedamp):
    """the separate setup / moist / vert_imp launches and the unfused damping (plain acoustic launches)"""
    st = _state(x1_2562, 26, "random")
    for exact in (0, 1):
        on, _ = _steps(st, exact, 2, fusesetup=fusesetup, fusedamp=fusedamp, accoef=1)
        off, _ = _steps(st, exact, 2, fusesetup=fusesetup, fusedamp=fusedamp, accoef=0)
        for n in range(2):
            bad = compare_states(on[n], off[n], rtol=0.0)
            assert not bad, f"exact={exact} after {n + 1} step(s): {bad[:6]}"


def test_accoef_with_tmedge(x1_2562):
    """option tmedge (off by default) keeps the stored set: the step runs, and has the same bits"""
    st = _state(x1_2562, 26, "random")
    for exact in (0, 1):
        on, _ = _steps(st, exact, 2, tmedge=1, accoef=1)
        off, _ = _steps(st, exact, 2, tmedge=1, accoef=0)
        ref, _ = _steps(st, exact, 2, accoef=1)
        for n in range(2):
            assert not compare_states(on[n], off[n], rtol=0.0)
            assert not compare_states(on[n], ref[n], rtol=0.0)


@pytest.mark.parametrize("physics,transport", [(1, 1), (2, 0)])
@pytest.mark.parametrize("L", [5, 56])
def test_accoef_mpas_forms(x1_2562, physics, transport, L):
    """the MPAS forms keep loading the stored set (stage 1's recover changes theta_m before stage 2
    reuses it): two steps with the option on and off, bit-identical"""
    st = mpas_state(x1_2562, L, "mpas0")
    for exact in (1, 0):
        out = {}
        for accoef in (0, 1):
            got = st.copy()
            with lib.Context(*st.dims()) as ctx:
                ctx.set_option("exact", exact)
                ctx.set_option("physics", physics)
                ctx.set_option("transport", transport)
                ctx.set_option("accoef", accoef)
                ctx.upload(st)
                for _ in range(2):
                    T.atm_srk3(ctx, 720.0, 1)
                ctx.sync()
                ctx.download(got)
            out[accoef] = got
        bad = compare_states(out[1], out[0], rtol=0.0)
        assert not bad, f"exact={exact}: {bad[:6]}"


@pytest.mark.parametrize("L", [5, 56])
def test_accoef_three_subdomains(x1_2562, L):
    """three loopback subdomains with the option on against one context (on, and off): the three values
    are column-local, so the halos do not matter"""
    st = _state(x1_2562, L, "random")

    def step(accoef):
        def fn(c):
            c.set_option("accoef", accoef)
            T.atm_srk3(c, 720.0, 1)
            T.atm_srk3(c, 720.0, 1)
        return fn
    got, stats = run_decomposed(st, 3, step(1), 0)
    assert all(s[0] > 0 for s in stats)  # the halo was exercised
    for accoef in (1, 0):
        bad = compare_states(got, run_single(st, step(accoef), 0), rtol=0.0)
        assert not bad, f"single accoef={accoef}: {bad[:6]}"


@pytest.mark.parametrize("small_step", [0, 1])
def test_standalone_task_reads_the_stored_columns(x1_2562, small_step):
    """standalone vert_imp, then other cofwr / coftz / a_tri uploaded, then the standalone acoustic step:
    the task reads the columns a caller stored, whatever the option says"""
    st = _state(x1_2562, 26, "random")
    other = st.copy()
    rng = np.random.default_rng(7)
    for name in COLS:
        other.arrays[name][...] = rng.uniform(0.5, 1.5, other.arrays[name].shape)

    def run(accoef, swap):
        got = st.copy()
        with lib.Context(*st.dims()) as ctx:
            ctx.set_option("exact", 1)
            ctx.set_option("accoef", accoef)
            ctx.upload(st)
            T.atm_compute_vert_imp_coefs(ctx, 240.0)
            if swap:
                ctx.upload(other, names=COLS)
            T.atm_advance_acoustic_step_work(ctx, 240.0, small_step)
            ctx.sync()
            ctx.download(got)
        return got
    on, off = run(1, True), run(0, True)
    bad = compare_states(on, off, rtol=0.0)
    assert not bad, bad[:6]
    n = st.nCells
    for name in COLS:  # (the uploaded columns, untouched by the task; row nCells is not transferred)
        assert np.array_equal(on.arrays[name][:n], other.arrays[name][:n]), name
    # ... and they were read: vert_imp's own columns give another rw_p
    assert not np.array_equal(on.arrays["rw_p"], run(1, False).arrays["rw_p"], equal_nan=True)


def test_accoef_option_values(x1_2562):
    st = _state(x1_2562, 5, "random")
    with lib.Context(*st.dims()) as ctx:
        assert ctx.get_option("accoef") == 1  # the default
        for bad in (2, -1):
            with pytest.raises(lib.MpasError) as e:
                ctx.set_option("accoef", bad)
            assert "(-1)" in str(e.value)  # MPAS_EINVAL
            assert ctx.get_option("accoef") == 1
        ctx.set_option("accoef", 0)
        assert ctx.get_option("accoef") == 0
        ctx.set_option("accoef", 1)
        assert ctx.get_option("accoef") == 1
