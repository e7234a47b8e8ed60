#!/usr/bin/env python3
"""The launches of atm_srk3 and the option surface, as data (tests/golden/srk3_rows_x1.2562.json).

step_rows(cfg): a context at x1.2562, cfg's options on top of the defaults, a random state, per-task
timing on; four consecutive atm_srk3 calls (a full step, generation 1, generation 2, a second kept
step) with timing_reset() between them.  Per step the rows of timing_report() with calls > 0, in
report order, as [key, calls]; a configuration the library refuses gives {"error": code}.

option_rows(name): a fresh context per option name; for each of VALUES the return code of
mpas_set_option (and its error text), then the return code and value of mpas_get_option.  Nothing is
launched after a set.

Run once on the build whose behaviour is the reference (the parent of a driver refactor):
    python tools/record_step_rows.py            # writes the fixture
tests/test_gpu_step_rows.py calls the same two functions and asserts equality.
"""
import ctypes
import json
import os
import sys
import threading

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "mpas-regent_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(REPO, "tests", "golden", "srk3_rows_x1.2562.json")
LEVELS = (5, 56)  # LP 8 and LP 64 (norz, the finish beside solve_e and etile exist at LP 64 only)
STEPS = 4
VALUES = (-1, 0, 1, 2, 3, 4, 5, 8, 67, 256, 512, 1 << 21)


def _matrix():
    """(name, options in order, dt, schedule, decomposed)"""
    out = []

    def add(opts, dt=720.0, schedule=1, decomposed=False, tag=""):
        name = ",".join(f"{k}={v}" for k, v in opts) or "defaults"
        out.append((name + tag, tuple(opts), dt, schedule, decomposed))

    # reference semantics
    add([])
    for kv in (("fusedamp", 0), ("tmedge", 1), ("epw", 1), ("ntu", 0)):
        add([("hfuse", 1), kv])
    add([("hfuse", 0)])
    for kv in (("fusedamp", 0), ("fusesml", 0), ("smlsum", 0), ("smlkeep", 0), ("fusesetup", 0), ("fusecopy", 0),
               ("defer4", 0), ("ntu", 0), ("ntu", 2), ("ntu", 3), ("accoef", 0), ("dd0", 0), ("vdyn", 0), ("tmedge", 1),
               ("exact", 1), ("stepkeep", 0), ("stepkeep", 2), ("vikeep", 0), ("a0keep", 0), ("dynkeep", 0), ("etile", 1)):
        add([("hfuse", 0), kv])
    for dt in (1.0, 2.0, 3.0, 720.0):  # rk_step triples (0,0,0), (0,1,1), (1,1,1), (240,360,360)
        add([("hfuse", 0)], dt=dt, schedule=0, tag=f";schedule=0;dt={dt:g}")
    # the MPAS vertical solver
    add([("physics", 1)])
    for extra in ([("transport", 1)], [("transport", 1), ("trsave", 0)], [("transport", 2)], [("mdamp", 0)], [("ntu", 0)]):
        add([("physics", 1)] + extra)
    # the MPAS dynamics
    add([("physics", 2)])
    for kv in (("mru", 0), ("msml", 0), ("mdamp", 0), ("forcing", 1), ("transport", 2), ("exact", 1), ("ntu", 0)):
        add([("physics", 2), kv])
    # a 2-part loopback split, rank 0's rows
    for v in (1, 0):
        add([("fusedamp_halo", v)], decomposed=True, tag=";2 parts")
    return out


MATRIX = _matrix()
CONFIGS = {f"L{L};{name}": (L, opts, dt, schedule, dec) for L in LEVELS for name, opts, dt, schedule, dec in MATRIX}

# every option name of mpas_set_option / mpas_get_option, listed by hand once
SETTABLE = [
    "exact", "graph", "fusedamp", "fusesetup", "fusecopy", "defer4", "ntu", "mdamp", "accoef", "dd0", "smlkeep",
    "stepkeep", "vikeep", "a0keep", "dynkeep", "mru", "msml", "vdyn", "tmedge", "fusesml", "smlsum", "fusedamp_halo",
    "hfuse", "graph_halo", "stub_refuse_capture", "stub_latency_us", "xcd", "keep_check", "epw", "vcmix", "physics",
    "trorder_e", "cve", "bsplit", "trepw", "trsu", "trorder", "ring1", "trtile", "trsave", "tredge", "trtile_ghosts",
    "trtcells", "trtclo", "etile", "etmode", "etthreads", "etcells", "etclo", "transport", "forcing", "overlap", "self",
    "bounds_probe",
]
GET_ONLY = [
    "tredge_active", "tredge_irregular", "trtile_active", "trtile_count", "etile_active", "etile_count", "etile_columns",
    "etile_maxclo", "stepkeep_gen", "dynkeep_fresh", "eoe_same", "hfuse_active", "graph_fallbacks", "graph_refused",
    "halo_state", "fusedamp_active", "orphan_edges", "graph_captures", "graph_launches", "bounds", "bounds_units", "selfc",
]
UNKNOWN = ["no_such_option"]
OPTION_NAMES = SETTABLE + GET_ONLY + UNKNOWN

_STATES = {}


def _state(L, zero_based):
    """the random state of the suite (tests/helpers.py), built once per shape and left unchanged"""
    key = (L, bool(zero_based))
    if key not in _STATES:
        from helpers import make_state
        from mpasdyn import mesh
        m = mesh.load_x1_2562()
        _STATES[key] = make_state(mesh.zero_based(m) if zero_based else m, L, "random")
    return _STATES[key]


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def _rc(rc):
    if rc != 0:
        raise Refused(rc)


def _four_steps(ctx, dt, schedule):
    steps = []
    for _ in range(STEPS):
        ctx.timing_reset()
        _rc(ctx.lib.mpas_atm_srk3(ctx.h, dt, schedule))
        ctx.sync()
        steps.append([[k, calls] for k, (calls, _ms) in ctx.timing_report().items() if calls > 0])
    return steps


def _set_all(ctx, opts):
    for k, v in opts:
        _rc(ctx.lib.mpas_set_option(ctx.h, k.encode(), int(v)))


def step_rows(cfg):
    from mpasdyn import decomp, lib
    L, opts, dt, schedule, decomposed = cfg
    physics = max([v for k, v in opts if k == "physics"] or [0])
    st = _state(L, physics > 0)
    try:
        if not decomposed:
            with lib.Context(*st.dims()) as ctx:
                _set_all(ctx, opts)
                ctx.upload(st)
                ctx.timing(True)
                return _four_steps(ctx, dt, schedule)
        # the setup of tests/test_gpu_decomp.py's run_decomposed: one context and one host thread per part
        nparts = 2
        d = decomp.Decomposition(st, nparts)
        ctxs = [lib.Context(*d.n_local(r), st.L) for r in range(nparts)]
        try:
            for r, c in enumerate(ctxs):
                lib.setup_subdomain(c, d, r)
                _set_all(c, opts)
                c.upload(d.local_state(r))
                c.timing(True)
            lib.halo_loopback(ctxs)
            res = [None] * nparts

            def drive(r):
                try:
                    res[r] = _four_steps(ctxs[r], dt, schedule)
                except Exception as e:  # noqa: BLE001 -- reported below
                    res[r] = e
            th = [threading.Thread(target=drive, args=(r,)) for r in range(nparts)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=120)
            for x in res:
                if isinstance(x, Exception):
                    raise x
            return res[0]
        finally:
            for c in ctxs:
                c.close()
    except Refused as e:
        return {"error": e.code}


def option_rows(name):
    """[[value, set rc, set error text, get rc, got value], ...] on one fresh context"""
    from mpasdyn import lib
    st = _state(56, False)
    rows = []
    with lib.Context(*st.dims()) as ctx:
        ctx.upload(st)
        for v in VALUES:
            rc = ctx.lib.mpas_set_option(ctx.h, name.encode(), v)
            text = ctx.lib.mpas_last_error(ctx.h).decode() if rc else ""
            got = ctypes.c_int64(0)
            grc = ctx.lib.mpas_get_option(ctx.h, name.encode(), ctypes.byref(got))
            rows.append([v, rc, text, grc, int(got.value) if grc == 0 else None])
    return rows


def pack(steps_by_config, options):
    """equal row lists stored once: the configurations hold indices into "rowsets" """
    rowsets, index, configs = [], {}, {}
    for name, steps in steps_by_config.items():
        if isinstance(steps, dict):
            configs[name] = steps
            continue
        ids = []
        for rows in steps:
            key = json.dumps(rows)
            if key not in index:
                index[key] = len(rowsets)
                rowsets.append(rows)
            ids.append(index[key])
        configs[name] = ids
    return {"mesh": "x1.2562", "steps": STEPS, "values": list(VALUES), "option_names": OPTION_NAMES,
            "rowsets": rowsets, "configs": configs, "options": options}


def unpack_steps(fx, name):
    c = fx["configs"][name]
    return c if isinstance(c, dict) else [fx["rowsets"][i] for i in c]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    steps = {}
    for name, cfg in CONFIGS.items():
        steps[name] = step_rows(cfg)
        print(name, "refused" if isinstance(steps[name], dict) else [len(s) for s in steps[name]], flush=True)
    options = {name: option_rows(name) for name in OPTION_NAMES}
    fx = pack(steps, options)
    one = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    with open(out, "w") as f:  # one row set, configuration or option name per line
        f.write("{\n")
        for k in ("mesh", "steps", "values", "option_names"):
            f.write(f"{json.dumps(k)}:{one(fx[k])},\n")
        f.write('"rowsets":[\n' + ",\n".join(one(r) for r in fx["rowsets"]) + "\n],\n")
        for k in ("configs", "options"):
            f.write(f"{json.dumps(k)}:{{\n" + ",\n".join(f"{json.dumps(n)}:{one(v)}" for n, v in fx[k].items()) +
                    ("\n},\n" if k == "configs" else "\n}\n"))
        f.write("}\n")
    print(f"{len(steps)} configurations, {len(options)} option names -> {out}")


if __name__ == "__main__":
    main()
