"""The premise of option `accoef`: three of vert_imp's coefficient columns are
functions of columns the acoustic step has loaded anyway.

atm_compute_vert_imp_coefs (dynamics_tasks.rg:550-578) forms

    cofwr(k) = .5 * dtseps * gravity * (fzm*zz + fzp*zz_m)
    coftz(k) = dtseps * (fzm*tm + fzp*tm_m)                        (0.0 at level 0)
    a_tri(k) = -1.0*cofwz*coftz_m*rdzw_m*zz_m + cofwr*cofrz_m - cofwt_m*coftz_m*rdzw_m

at the interfaces 0 < k < L, with cofrz_m = dtseps*rdzw_m.  The acoustic kernels hold zz, theta_m,
cofwz and cofwt in registers; evaluated from those in this order (no contraction, IEEE doubles),
the three expressions must give the stored columns bit for bit -- then recomputing them is not a
reassociation and every bit-identity test keeps its meaning.  CPU only: the oracle and NumPy.
"""
import numpy as np
import pytest

import oracle as O
from helpers import make_state

DTS = 240.0
EPSSM = 0.1
GRAVITY = 9.80616


@pytest.mark.parametrize("variant", ["random", "physical"])
@pytest.mark.parametrize("L", [5, 26, 56])
def test_three_coefficients_from_acoustic_registers(x1_2562, L, variant):
    st = make_state(x1_2562, L, variant)
    ref = st.copy()
    O.Oracle(st).atm_compute_vert_imp_coefs(DTS)
    n = st.nCells
    dtseps = .5 * DTS * (1.0 + EPSSM)
    fzm, fzp, rdzw = ref["fzm"], ref["fzp"], ref["rdzw"]
    # what the acoustic step reads: mesh / state columns vert_imp does not write, and the two
    # coefficient columns it still loads (the oracle's, as stored)
    zz, tm = ref["zz"][:n], ref["theta_m"][:n]
    assert np.array_equal(st["zz"][:n], zz) and np.array_equal(st["theta_m"][:n], tm, equal_nan=True)
    cofwz, cofwt = st["cofwz"][:n], st["cofwt"][:n]
    cofwr = np.zeros((n, L))
    coftz = np.zeros((n, L))  # (level 0: 0.0)
    for k in range(1, L):
        cofwr[:, k] = .5 * dtseps * GRAVITY * (fzm[k] * zz[:, k] + fzp[k] * zz[:, k - 1])
        coftz[:, k] = dtseps * (fzm[k] * tm[:, k] + fzp[k] * tm[:, k - 1])
    assert (st["coftz"][:n, 0] == 0.0).all()
    assert np.array_equal(st["cofwr"][:n, 1:L], cofwr[:, 1:L], equal_nan=True)
    assert np.array_equal(st["coftz"][:n, :L], coftz, equal_nan=True)
    # level L of coftz is left as it was (the value the field's keep tail holds)
    assert np.array_equal(st["coftz"][:n, L], ref["coftz"][:n, L], equal_nan=True)
    for k in range(1, L):
        cofrz_m = dtseps * rdzw[k - 1]
        a = -1.0 * cofwz[:, k] * coftz[:, k - 1] * rdzw[k - 1] * zz[:, k - 1] + cofwr[:, k] * cofrz_m - \
            cofwt[:, k - 1] * coftz[:, k - 1] * rdzw[k - 1]
        assert np.array_equal(st["a_tri"][:n, k], a, equal_nan=True), k
