"""The premises of options `dd0` and `smlkeep`, on the CPU oracle alone.

`dd0`: the acoustic step reads rw_save and rw only as rw_save - rw at the interfaces 0 < k < L.  The
step's setup stores rw_save = rw at every level but L and, recover not being called in the reference
semantics (Q7), no task of atm_srk3 writes rw: after any number of steps the two columns are the same
bits below level L, so the difference is +0.0 wherever rw is finite.

`smlkeep`: set_smlstep's slope-flux sum is a function of u_tend, zb_cell, zb3_cell, edgesOnCell_sign
(and fzm / fzp, the mesh lists): no task of the step writes any of them (u_tend: Q2), so the sum of
one step is the sum of the next.
"""
import numpy as np
import pytest

import oracle as O
from helpers import make_state

INPUTS = ("u_tend", "zb_cell", "zb3_cell", "edgesOnCell_sign", "rw", "fzm", "fzp", "edgesOnCell", "nEdgesOnCell")


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26])
def test_rw_save_is_rw_and_the_flux_inputs_stay(x1_2562, L, variant):
    st = make_state(x1_2562, L, variant)
    before = st.copy()
    o = O.Oracle(st)
    n = st.nCells
    for step in (1, 2):
        o.atm_srk3(720.0, 1)
        a, b = st["rw_save"][:n, :L], st["rw"][:n, :L]
        assert a.tobytes() == b.tobytes(), f"rw_save != rw below level L after {step} step(s)"
        for name in INPUTS:
            assert st[name].tobytes() == before[name].tobytes(), f"{name} changed in step {step}"
    # (the premise is not vacuous: the step ran and moved the state)
    assert not np.array_equal(st["w"], before["w"], equal_nan=True)
