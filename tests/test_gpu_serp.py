"""Stage 0's edge copies made by dyn_tend's cell kernel A.

atm_srk3 under the reference semantics with `ntu` and `fusecopy` on, on the large grids' launch
order (hfuse 0): stage 0's edge kernel B forms neither tend_u nor the theta flux, so the u and ru
columns it loaded served setup's copies ru_save = ru, u_2 = u alone.  A gathers both columns at the
cell's edges anyway and now stores the copies of the edges the cell owns (X_eown); the edges no cell
lists (X_orph: edge 0 under the raw 1-based ids of the x1.2562 fixture) are copied by a launch of
their own, and B loads neither column.  The copies must be the bytes B stored: the raw value below
level L, level L untouched (dynamics_tasks.rg:758-761).

The B-copies path of this file is the setup kernel's own copy (fusecopy 0): the same task, no fusion.
Decomposed runs and the hfuse launch order keep the copy in B; both must stay bit-identical with the
one-context run.
"""
import numpy as np
import pytest

from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import tasks as T
from test_gpu_decomp import run_decomposed, run_single

pytestmark = pytest.mark.gpu

_ST = {}


def _state(mesh, L, variant):
    key = (L, variant)
    if key not in _ST:
        _ST[key] = make_state(mesh, L, variant)
    return _ST[key]


def _steps(st, exact, nsteps, **opts):
    """the state after each of nsteps atm_srk3 steps, and the context's orphan-edge count"""
    out = []
    with lib.Context(*st.dims()) as ctx:
        ctx.set_option("exact", exact)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.upload(st)
        for _ in range(nsteps):
            T.atm_srk3(ctx, 720.0, 1)
            ctx.sync()
            got = st.copy()
            ctx.download(got)
            out.append(got)
        orph = ctx.get_option("orphan_edges")
    return out, orph


def _orphans(st):
    """the edges no cell lists within its first nEdgesOnCell slots (k_own_min's rule)"""
    eoc, ne = st.arrays["edgesOnCell"], st.arrays["nEdgesOnCell"].reshape(-1)
    listed = np.zeros(st.nEdges + 1, dtype=bool)
    for i in range(eoc.shape[1]):
        e = eoc[:st.nCells, i][(i < ne[:st.nCells]) & (eoc[:st.nCells, i] >= 0) & (eoc[:st.nCells, i] < st.nEdges)]
        listed[e] = True
    return np.flatnonzero(~listed[:st.nEdges])


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("L", [5, 56])
def test_copies_by_A_bit_identical(x1_2562, L, exact, variant):
    """after one and after two steps every field, ru_save and u_2 among them, has the same bits with
    the copies made by A (hfuse 0, fusecopy 1) and by the setup kernel (fusecopy 0); the orphan edge's
    columns are the step's starting ru / u below level L and the uploaded value at level L"""
    st = _state(x1_2562, L, variant)
    a, orph = _steps(st, exact, 2, hfuse=0, fusecopy=1)
    b, _ = _steps(st, exact, 2, hfuse=0, fusecopy=0)
    for n in range(2):
        bad = compare_states(a[n], b[n], rtol=0.0)
        assert not bad, f"after {n + 1} step(s): {bad[:6]}"
    oe = _orphans(st)
    assert orph == len(oe) and len(oe) >= 1  # (edge 0 of the raw 1-based ids)
    start = [st, a[0]]  # (the state each step starts from)
    for n in range(2):
        for dst, src in (("ru_save", "ru"), ("u_2", "u")):
            got = a[n].arrays[dst][oe]
            assert np.array_equal(got[:, :L], start[n].arrays[src][oe][:, :L], equal_nan=True), (n, dst)
            assert np.array_equal(got[:, L], st.arrays[dst][oe][:, L], equal_nan=True), (n, dst, "level L")
            # (every edge, owned ones too: the same rule)
            assert np.array_equal(a[n].arrays[dst][:st.nEdges, :L], start[n].arrays[src][:st.nEdges, :L], equal_nan=True)
            assert np.array_equal(a[n].arrays[dst][:st.nEdges, L], st.arrays[dst][:st.nEdges, L], equal_nan=True)


@pytest.mark.parametrize("L", [5, 56])
def test_copies_hfuse_order_and_graph(x1_2562, L):
    """the hfuse launch order (A beside the setup launch: the copy stays in B) and the eager step give the
    same bits as the graph-replayed large-grid order whose A makes the copies"""
    st = _state(x1_2562, L, "random")
    a, _ = _steps(st, 0, 2, hfuse=0, graph=1)
    for opts in ({"hfuse": 2, "graph": 1}, {"hfuse": 0, "graph": 0}):
        b, _ = _steps(st, 0, 2, **opts)
        bad = compare_states(b[1], a[1], rtol=0.0)
        assert not bad, f"{opts}: {bad[:6]}"


def test_copies_keep_check(x1_2562):
    """keep tails (eager steps, every task checked) with A's copies: no keep failure, the default run's bits"""
    st = _state(x1_2562, 56, "random")
    a, _ = _steps(st, 0, 1, hfuse=0)
    b, _ = _steps(st, 0, 1, hfuse=0, graph=0, keep_check=1)
    bad = compare_states(b[0], a[0], rtol=0.0)
    assert not bad, bad[:6]


@pytest.mark.parametrize("L", [5, 56])
def test_three_subdomains_equal_one_context(x1_2562, L):
    """three loopback subdomains (the copy stays in B there) against one context, one step, default options"""
    st = _state(x1_2562, L, "random")
    step = lambda c: T.atm_srk3(c, 720.0, 1)  # noqa: E731
    ref = run_single(st, step, 0)
    got, stats = run_decomposed(st, 3, step, 0)
    bad = compare_states(got, ref, rtol=0.0)
    assert not bad, bad[:6]
    assert all(s[0] > 0 for s in stats)  # the halo was exercised
