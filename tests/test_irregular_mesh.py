"""mesh.irregular(): a Voronoi mesh with 4- to 8-sided cells, on the CPU.

Every other mesh of the suite (x1.2562, icosahedral) has 5- and 6-sided cells only, so no list
longer than the kernels' unconditional NF = 6 edgesOnCell / QF = 10 edgesOnEdge slots, and
entity counts that are multiples of every block's column count.  Here: (1) the mesh is a valid
MPAS mesh; (2) it has what tests/test_gpu_irregular_mesh.py relies on, asserted so that a later
change of seed or jitter cannot hollow those tests out; (3) the oracle -- the reference of the
GPU tests, whose long-list loops are as unexercised as the kernels' -- against the NumPy
restatements and the transport properties of the x1.2562 tests, on this mesh."""
import functools

import numpy as np
import pytest

import test_init_mesh_tasks as TI
import test_oracle as TO
import test_transport as TT
import test_transport_rk3 as TR
from mpasdyn import mesh as M


@functools.lru_cache(maxsize=None)
def irregular_mesh():
    return M.irregular()


def _xyz(m, kind):
    return np.stack([getattr(m, a + kind) for a in "xyz"], 1)


# ------------------------------------------------------------------------- a valid MPAS mesh
def test_counts_and_euler():
    m = irregular_mesh()
    assert (m.nCells, m.nEdges, m.nVertices) == (10 * 4 ** 3 + 2 + 5, 1935, 1290)
    assert m.nCells - m.nEdges + m.nVertices == 2
    assert m.nEdgesOnCell.sum() == 2 * m.nEdges and 3 * m.nVertices == 2 * m.nEdges


def test_edges_listed_by_their_two_cells():
    m = irregular_mesh()
    c = np.arange(m.nCells)
    cnt = np.zeros(m.nEdges, int)
    for j in range(10):
        on = j < m.nEdgesOnCell
        e = m.edgesOnCell[:, j] - 1
        mine = (m.cellsOnEdge[e, 0] - 1 == c) | (m.cellsOnEdge[e, 1] - 1 == c)
        assert mine[on].all()
        np.add.at(cnt, e[on], 1)
        other = np.where(m.cellsOnEdge[e, 0] - 1 == c, m.cellsOnEdge[e, 1], m.cellsOnEdge[e, 0])
        assert (m.cellsOnCell[:, j] == other)[on].all()
    assert (cnt == 2).all()
    assert (m.cellsOnEdge[:, 0] != m.cellsOnEdge[:, 1]).all()


def test_edges_on_cell_counter_clockwise():
    """consecutive edge midpoints turn left around the cell centre (seen from outside), and
    the turns of a cell add up to one revolution"""
    m = irregular_mesh()
    xc, xe = _xyz(m, "Cell"), _xyz(m, "Edge")
    ne = m.nEdgesOnCell
    total = np.zeros(m.nCells)
    for j in range(10):
        on = j < ne
        a = xe[m.edgesOnCell[:, j] - 1] - xc
        b = xe[m.edgesOnCell[np.arange(m.nCells), (j + 1) % ne] - 1] - xc
        a -= np.sum(a * xc, 1)[:, None] * xc  # into the tangent plane
        b -= np.sum(b * xc, 1)[:, None] * xc
        turn = np.arctan2(np.sum(np.cross(a, b) * xc, 1), np.sum(a * b, 1))
        assert (turn[on] > 0).all()
        total += np.where(on, turn, 0.0)
    assert np.allclose(total, 2 * np.pi, rtol=0, atol=1e-12)


def test_vertices_on_cell_between_edges():
    m = irregular_mesh()
    ne = m.nEdgesOnCell
    for j in range(10):
        on = j < ne
        v = m.verticesOnCell[:, j]
        e0 = m.edgesOnCell[:, j] - 1
        e1 = m.edgesOnCell[np.arange(m.nCells), (j + 1) % ne] - 1
        for e in (e0, e1):
            assert ((m.verticesOnEdge[e] == v[:, None]).any(1))[on].all()
        assert ((m.cellsOnVertex[v - 1] - 1 == np.arange(m.nCells)[:, None]).any(1))[on].all()
    # vertices: both cells of each vertex edge belong to the vertex
    for j in range(3):
        e = m.edgesOnVertex[:, j] - 1
        for s in range(2):
            assert ((m.cellsOnVertex - 1) == (m.cellsOnEdge[e, s] - 1)[:, None]).any(1).all()


def test_edges_on_edge_trisk_order():
    """nEdgesOnEdge = n1 + n2 - 2: the other edges of cell 1 counter-clockwise from the edge,
    then those of cell 2"""
    m = irregular_mesh()
    c1, c2 = m.cellsOnEdge[:, 0] - 1, m.cellsOnEdge[:, 1] - 1
    assert (m.nEdgesOnEdge == m.nEdgesOnCell[c1] + m.nEdgesOnCell[c2] - 2).all()
    for e in range(m.nEdges):
        want = []
        for c in (c1[e], c2[e]):
            row = m.edgesOnCell[c, :m.nEdgesOnCell[c]].tolist()
            i = row.index(e + 1)
            want += row[i + 1:] + row[:i]
        assert m.edgesOnEdge[e, :len(want)].tolist() == want, e


def test_geometry():
    """a Delaunay triangulation's circumcentre dual: cell and triangle areas tile the sphere;
    the kites (two unsigned triangle areas each) are finite and positive only"""
    m = irregular_mesh()
    assert abs(m.areaCell.sum() - 4 * np.pi) < 1e-12
    assert abs(m.areaTriangle.sum() - 4 * np.pi) < 1e-12
    assert (m.areaCell > 0).all() and (m.areaTriangle > 0).all()
    assert (m.dcEdge > 0).all() and (m.dvEdge > 0).all()
    assert np.isfinite(m.kiteAreasOnVertex).all() and (m.kiteAreasOnVertex > 0).all()
    for k in ("xCell", "xEdge", "xVertex"):
        r = _xyz(m, k[1:])
        assert np.allclose(np.sum(r * r, 1), 1.0, rtol=0, atol=1e-14)


def test_padding_follows_the_file_convention():
    """edgesOnCell / cellsOnCell repeat the last valid entry, verticesOnCell, edgesOnEdge and
    weightsOnEdge pad with 0; ids are 1-based"""
    m = irregular_mesh()
    ne = m.nEdgesOnCell
    last = m.edgesOnCell[np.arange(m.nCells), ne - 1]
    lastc = m.cellsOnCell[np.arange(m.nCells), ne - 1]
    for j in range(10):
        pad = j >= ne
        assert (m.edgesOnCell[pad, j] == last[pad]).all() and (m.cellsOnCell[pad, j] == lastc[pad]).all()
        assert (m.verticesOnCell[pad, j] == 0).all() and (m.verticesOnCell[~pad, j] >= 1).all()
    pad = np.arange(20)[None, :] >= m.nEdgesOnEdge[:, None]
    assert (m.edgesOnEdge[pad] == 0).all() and (m.weightsOnEdge[pad] == 0).all()
    assert (m.edgesOnEdge[~pad] >= 1).all() and m.edgesOnEdge.max() <= m.nEdges
    assert m.edgesOnCell.min() >= 1 and m.edgesOnCell.max() == m.nEdges
    assert m.cellsOnEdge.min() == 1 and m.cellsOnEdge.max() == m.nCells
    for a in (m.edgesOnCell, m.cellsOnCell, m.verticesOnCell, m.edgesOnEdge, m.nEdgesOnCell, m.nEdgesOnEdge):
        assert a.dtype == np.int32


def test_generator_limits():
    with pytest.raises(ValueError, match="9 edges"):
        M.irregular(jitter=0.25)  # (a 9-sided cell: build_state's advCellsForEdge list overflows)
    with pytest.raises(ValueError):
        M.irregular(level=1, extra=1, order="peano")


# ------------------------------------------------------- what the GPU tests need from the mesh
def test_coverage_conditions():
    m = irregular_mesh()
    ne = m.nEdgesOnCell
    hist = np.bincount(ne, minlength=11)
    assert hist[8] >= 3 and hist[7] >= 50 and hist[:5].sum() >= 3 and hist[9:].sum() == 0
    assert (m.nEdgesOnEdge > 10).sum() >= 100 and m.nEdgesOnEdge.max() <= 20
    for n in (m.nCells, m.nEdges, m.nVertices):
        assert n % 4 != 0
    # Hilbert order (the default): columns that share a wavefront at LP = 8
    kinds = [len(set(ne[i:i + 8].tolist())) for i in range(0, m.nCells - 7, 8)]
    assert max(kinds) >= 3
    # the histograms profiles/irregular_mesh/README.md quotes
    assert hist[4:9].tolist() == [6, 123, 400, 113, 5]
    assert np.bincount(m.nEdgesOnEdge)[8:].tolist() == [29, 338, 1069, 404, 85, 10]


# ----------------------------------------------------------------- the oracle on this mesh
def test_oracle_restatements():
    m = irregular_mesh()
    TO.check_divergence_q9(m)
    TO.check_vert_imp(m)
    TO.check_div_damping(m)
    TO.check_output_diagnostics(m)
    TO.check_reconstruct_2d(m)


def test_oracle_recover_restatement():
    """the plain-Python w recovery on cells of every nEdgesOnCell (4 to 8)"""
    m = irregular_mesh()
    cells = [int(np.nonzero(m.nEdgesOnCell == n)[0][i]) for n in (4, 5, 6, 7, 8) for i in (0, 1, 2)]
    TO.check_recover_large_step(m, cells=cells)


@pytest.mark.parametrize("L", [5, 26])
def test_transport_properties(L):
    m = irregular_mesh()
    TT.check_constant_preserved(m, L)
    TT.check_monotone_and_conservative(m, L)


def test_transport_unlimited_where_smooth():
    TT.check_unlimited_where_smooth(irregular_mesh())


@pytest.mark.parametrize("L", [5, 26])
def test_transport_rk3_properties(L):
    m = irregular_mesh()
    TR.check_mono_rk_on_old_fluxes_matches_oracle(m, L)
    TR.check_unlimited_stage_keeps_a_constant(m, L)
    TR.check_unlimited_stage_conserves_and_overshoots(m, L)
    TR.check_rk3_transport_is_monotone_and_conservative(m, L)


def test_transport_rk3_third_order():
    TR.check_three_unlimited_stages_are_third_order(irregular_mesh())


@pytest.mark.parametrize("ids", ["raw", "zero_based"])
def test_mesh_tasks_match_build_state(ids):
    """the oracle's mesh tasks against build_state's host restatements; the advection lists
    hold up to 9 cells here (the reference's cap) and as few as the 4-sided cells leave"""
    n = TI.check_mesh_tasks_match_build_state(irregular_mesh(), ids)
    assert n.max() == 9 and n.min() >= 4


@pytest.mark.parametrize("variant", ["random", "ref", "mpas0"])
@pytest.mark.parametrize("L", [5, 26])
def test_oracle_steps_stay_finite(variant, L):
    """an oracle atm_srk3 and mpas_srk3 leave the prognostic fields finite at every entity"""
    import oracle as O
    from helpers import make_state
    m = irregular_mesh()
    st0 = make_state(M.zero_based(m) if variant == "mpas0" else m, L, "ref" if variant == "ref" else "random")
    for step in ("atm_srk3", "mpas_srk3"):
        st = st0.copy()
        getattr(O.Oracle(st), step)(720.0, 1)
        nC, nE = st.nCells, st.nEdges
        for f, n in (("w", nC), ("theta_m", nC), ("rho_zz", nC), ("u", nE), ("ru_p", nE)):
            assert np.isfinite(st[f][:n, :L]).all(), (step, f)
