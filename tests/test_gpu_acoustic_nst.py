"""The acoustic launch that stores no acoustic state (tag `-st`, option `ntu`) in its own instance (k_acoustic NST,
DESIGN §4q): the default step's MODE 2 launch with the dead state columns loads rw_p alone -- wwAvg, which only
its own store reads, is not loaded, and nothing of the four columns is stored.

The twin is independent of the build: with `ntu` 0 no launch is tagged `-st`, every substep stores its state and
the later stages overwrite what was dead.  Every field is the same bits.

Reaching the instance.  A MODE 2 launch takes it only on the separate-launch path of `acoustic_lp`: with `hfuse` 0
(the small grids' default pairs the stage's last acoustic launch with solve_diagnostics in a combined kernel) and
not on the tail grid, which a mesh below 16384 owned cells (kTailCells) takes as soon as it has an orphan edge --
and the `random` variant of both small meshes has one.  Both of those paths keep the runtime test.  So the small
cases use the zero-based ids (no orphan edge; the SELF instances), and the instances without SELF, which only the
1-based ids give, run on x1.40962, the smallest mesh of the family above kTailCells; each case asserts its path.
"""
import pytest

from helpers import compare_states, make_state
from mpasdyn import lib
from mpasdyn import mesh as M
from mpasdyn import tasks as T
from test_gpu_stepkeep import DT, _run, _same

pytestmark = pytest.mark.gpu

K_TAIL_CELLS = 16384  # (k_acoustic.hip kTailCells)
ST_KEY = "atm_advance_acoustic_step_work[ss>0+damp-old-st]"
# small meshes, zero-based ids: x1.2562 and the Voronoi mesh with 4- to 8-sided cells, at LP 8 and LP 64
SMALL = [("x1.2562", 5), ("x1.2562", 56), ("irregular", 5), ("irregular", 56)]

_MESH = {}


def _mesh(name, x1_2562):
    if name == "x1.2562":
        return x1_2562
    if name not in _MESH:
        _MESH[name] = M.irregular() if name == "irregular" else M.x1(40962)
    return _MESH[name]


def _path(log):
    """what decides the launch path, read once the mesh is uploaded"""
    def fn(ctx):
        log.append((ctx.get_option("orphan_edges"), ctx.get_option("selfc")))
    return fn


def _timed_keys(log):
    def fn(ctx):
        ctx.timing(True)
        ctx.timing_reset()
        T.atm_srk3(ctx, DT, 1)
        ctx.sync()
        log.append(sorted(ctx.timing_report()))
        ctx.timing(False)
    return fn


def _on_instance_path(nCells, orph):
    """the MODE 2 launches are k_acoustic's, not the tail grid's k_acoustic_o (acoustic_lp)"""
    return orph == 0 or nCells >= K_TAIL_CELLS


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("case", SMALL, ids=[f"{m}-L{L}" for m, L in SMALL])
def test_nst_instance_bit_identical(x1_2562, case, graph):
    """SELF instances: the default step against ntu 0, every field after each of three steps; a fourth, timed step
    shows that the step made a `-st` launch past a stage's first substep, and the twin none"""
    name, L = case
    st = make_state(M.zero_based(_mesh(name, x1_2562)), L, "random")
    keys, keys0, path = [], [], []
    on, _ = _run(st, dict(hfuse=0, graph=graph), [_path(path)] + ["step"] * 3 + [_timed_keys(keys)])
    off, _ = _run(st, dict(hfuse=0, graph=graph, ntu=0), ["step"] * 3 + [_timed_keys(keys0)])
    orph, selfc = path[0]
    assert orph == 0 and _on_instance_path(st.dims()[0], orph) and selfc == 1
    _same(on, off, "ntu 1 (NST instance) / ntu 0")
    assert ST_KEY in keys[0], keys[0]
    assert not [k for k in keys0[0] if "-st" in k], keys0[0]


def _three_steps(st, opts):
    got = st.copy()
    with lib.Context(*st.dims()) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.upload(st)
        path = (ctx.get_option("orphan_edges"), ctx.get_option("selfc"))
        for _ in range(3):
            T.atm_srk3(ctx, DT, 1)
        ctx.sync()
        ctx.download(got)
    return got, path


@pytest.mark.parametrize("L", [5, 32])
def test_nst_instance_without_self(x1_2562, L):
    """the instances without SELF (1-based ids), LP 8 and LP 64: x1.40962, above kTailCells, so the orphan edge's
    blocks are a launch of their own and the cell launch is k_acoustic's; every field after three captured steps
    (one download per run: the mesh is the size the path needs)"""
    st = make_state(_mesh("x1.40962", x1_2562), L, "random")
    on, (orph, selfc) = _three_steps(st, dict(hfuse=0))
    assert selfc == 0 and _on_instance_path(st.dims()[0], orph)
    off, _ = _three_steps(st, dict(hfuse=0, ntu=0))
    bad = compare_states(on, off, rtol=0.0)
    assert not bad, bad[:6]
