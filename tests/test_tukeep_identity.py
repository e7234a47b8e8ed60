"""The premise of option `tukeep`, on the CPU oracle alone.

Stage 2's dyn_tend edge section stores tend_u, tend_u_euler (the deferred del4 applied) and, with option vdyn, v.
tend_u(k) reads the evolving set of §4k through w at level k + 1 alone (the curvature term), and of w only level L
moves from one step to the next (§4k).  From the second consecutive step on, the ends of two steps therefore differ
in tend_u at level L - 1 and at no other level, and tend_u_euler and v are one set of bytes: a kept step that finds
the step-before's columns in place has one level of one column to form.  Between steps 1 and 2 tend_u differs at
other levels too (stage 0 of step 1 read the uploaded diagnostics), so the columns have to come from a kept step.

Variant `random` only: with `physical` w at level L does not move and nothing differs at all, which would make
every assertion here vacuous.
"""
import numpy as np
import pytest

import oracle as O
from helpers import make_state
from mpasdyn import mesh as M

DT = 720.0
STEPS = 4
# measured share of the edges whose tend_u(L - 1) differs between consecutive kept steps' ends (printed by the test):
# x1.2562 0.83 and 0.85 (L 5 / 26); the bar asks more than half
MIN_SHARE = 0.5

_IRR = {}


def _mesh(name, x1_2562):
    if name == "x1.2562":
        return x1_2562
    if "m" not in _IRR:
        _IRR["m"] = M.irregular()
    return _IRR["m"]


@pytest.mark.parametrize("case", [("x1.2562", 5), ("x1.2562", 26), ("irregular", 5)], ids=lambda c: f"{c[0]}-L{c[1]}")
def test_tend_u_moves_at_its_top_level_alone(x1_2562, case):
    name, L = case
    st = make_state(_mesh(name, x1_2562), L, "random")
    nE = st.dims()[1]
    o = O.Oracle(st)
    ends = []
    for _ in range(STEPS):
        o.atm_srk3(DT, 1)
        ends.append({n: st[n].copy() for n in ("tend_u", "tend_u_euler", "v")})
    for n in (1, 2):  # the ends of steps 2 / 3 and 3 / 4
        a, b = ends[n], ends[n + 1]
        assert a["tend_u_euler"].tobytes() == b["tend_u_euler"].tobytes(), n + 1
        assert a["v"].tobytes() == b["v"].tobytes(), n + 1
        ta, tb = a["tend_u"], b["tend_u"]
        keep = np.ones(ta.shape[1], dtype=bool)
        keep[L - 1] = False
        assert ta[:, keep].tobytes() == tb[:, keep].tobytes(), n + 1
        with np.errstate(invalid="ignore"):
            share = float(np.mean(ta[:nE, L - 1].view(np.uint64) != tb[:nE, L - 1].view(np.uint64)))
        print(f"{name} L {L}, steps {n + 1} / {n + 2}: tend_u(L - 1) differs at {share:.4f} of {nE} edges")
        assert share > MIN_SHARE, share
    # steps 1 / 2: the full step's columns are not the kept steps'
    ta, tb = ends[0]["tend_u"], ends[1]["tend_u"]
    other = [k for k in range(L) if k != L - 1 and ta[:nE, k].tobytes() != tb[:nE, k].tobytes()]
    assert other, "tend_u differs at level L - 1 alone between steps 1 and 2 as well"
