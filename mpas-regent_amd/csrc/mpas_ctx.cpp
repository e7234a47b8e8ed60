// mpas_ctx.cpp -- libmpasdyn host runtime: context, device residency, the C-ABI task
// entry points of include/mpas_dyn.h, and the atm_srk3 driver (rk_timestep.rg:361-500).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <memory>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "mpas_dev.h"
#include "mpas_halo.h"
#include "mpas_dyn.h"

namespace mpas {
const FieldInfo kFields[X_COUNT] = {
#define MPAS_FIELD(name, KIND, W, DIST, LO, HI) {#name, K_##KIND, W, D_##DIST, LO, HI},
#include "mpas_fields.def"
#undef MPAS_FIELD
    {"cosAngleEdge", K_E2F, 1, D_M, 0, 0},
    {"cosLatEdge", K_E2F, 1, D_M, 0, 0},
    {"cosLatCell", K_C2F, 1, D_M, 0, 0},
    {"sinLatCell", K_C2F, 1, D_M, 0, 0},
    {"cosLonCell", K_C2F, 1, D_M, 0, 0},
    {"sinLonCell", K_C2F, 1, D_M, 0, 0},
    {"ce_c1", K_C2I, 10, D_M, 0, 0},
    {"ce_c2", K_C2I, 10, D_M, 0, 0},
    {"ce_dv", K_C2F, 10, D_M, 0, 0},
    {"ce_dc", K_C2F, 10, D_M, 0, 0},
    {"ve_dc", K_V2F, 3, D_M, 0, 0},
    {"ce_idc", K_C2F, 10, D_M, 0, 0},
    {"ce_msd2", K_C2F, 10, D_M, 0, 0},
    {"ce_msd4", K_C2F, 10, D_M, 0, 0},
    {"ce_oth", K_C2I, 10, D_M, 0, 0},
    {"ce_s1", K_C2I, 10, D_M, 0, 0},
    {"eB", K_E2I, 24, D_M, 0, 0},
    {"cR", K_C2I, CREC, D_M, 0, 0},
    {"cRs", K_C2I, CREC, D_M, 0, 0},
    {"wfl", K_C2F, 2, D_M, 0, 0},
    {"wc", K_C3, 1, D_M, 0, 0},
    {"F", K_E3, 1, D_M, 0, 0},
    {"Fw", K_E3, 1, D_M, 0, 0},
    {"dvA", K_C3, 1, D_M, 0, 0},
    {"dvB", K_C3, 1, D_M, 0, 0},
    {"rupB", K_E3, 1, D_M, 0, 0},
    {"eown", K_C2I, 1, D_M, 0, 0},
    {"eowner", K_E2I, 1, D_M, 0, 0},
    {"orph", K_E2I, 1, D_M, 0, 0},
    {"tme", K_E3, 1, D_M, 0, 0},
    {"smlS", K_C3, 1, D_M, 0, 0},
    {"Dd", K_C3, 1, D_M, 0, 0},
    {"Ah", K_E3, 8, D_M, 0, 0},
    {"Rp", K_C3V, 8, D_M, 0, 0},
    {"Rm", K_C3V, 8, D_M, 0, 0},
    {"su", K_C3V, 8, D_M, 0, 0},
    {"hskv", K_C3, 1, D_M, 0, 0},
    {"w0", K_C3, 1, D_M, 0, 0},
    {"cofwt0", K_C3, 1, D_M, 0, 0},
    {"cofwz0", K_C3, 1, D_M, 0, 0},
    {"a0", K_C3, 1, D_M, 0, 0},
    {"b0", K_C3, 1, D_M, 0, 0},
    {"c0", K_C3, 1, D_M, 0, 0},
    {"kd0", K_C3, 1, D_M, 0, 0},
    {"tue0", K_E3, 1, D_M, 0, 0},
    {"w1", K_C3, 1, D_M, 0, 0},
    {"w2", K_C3, 1, D_M, 0, 0},
    {"dkf", K_ZV, 1, D_M, 0, 0},
    {"pblFu", K_C3, 1, D_M, 0, 0},
    {"pblFv", K_C3, 1, D_M, 0, 0},
    {"sinAngleEdge", K_E2F, 1, D_M, 0, 0},
};
// translation units with kernels, registered at load time (mpas_dev.h, bounds-checked build)
static std::vector<void* (*)()>& bounds_tus() {
    static std::vector<void* (*)()> v;
    return v;
}
int bounds_register_tu(void* (*symbol)()) {
    bounds_tus().push_back(symbol);
    return 0;
}
}  // namespace mpas

using namespace mpas;

struct TimedCall {
    int task;
    hipEvent_t e0, e1;
};

struct mpas_ctx {
    int device = 0;
    mpas_dims dims{};
    DevState S{};
    hipStream_t stream = nullptr;
    std::string err;
    int exact = 0;
    // option "transport": atm_srk3 runs the scalar transport (physics >= 1) -- 1 the monotonic task once
    // over dt, 2 MPAS's RK3 form: two unlimited stages over dt/3 and dt/2, then the monotonic task over dt
    int transport = 0;
    // option "forcing" (the MPAS dynamics, physics = 2): 1 -- atm_srk3 runs the Held-Suarez forcing task once per
    // step, ahead of stage 0's setup; its two tendencies are held over the three stages (as MPAS-A holds its
    // physics tendencies).  0: the step never writes them
    int forcing = 0;
    // the sigma-level statistics (k_stats.hip; mpas_sigma_stats_configure): the accumulators -- one record of
    // stats_rec(stats_ns) doubles per local cell, not registry fields -- and the targets with their logs.
    // Option "stats_every" = N > 0: mpas_atm_srk3 launches the task on the stream after every N-th step since
    // the option was set (stats_step counts them), behind the step's launches or its replayed graph: never part
    // of a capture, so the captured step is the one without the option.  stats_samples: the task's runs since
    // the accumulators were last zeroed
    double* stats_acc = nullptr;
    double* stats_sig = nullptr;
    int stats_ns = 0;
    int stats_every = 0;
    int64_t stats_step = 0, stats_samples = 0;
    // option "microphysics" (the MPAS dynamics, physics = 2): 1 -- atm_srk3 ends with the Kessler warm-rain task
    // (k_kessler.hip) over the step's dt, inside the captured graph; 0: the step is launch for launch the step
    // without it.  precip: the task's accumulators -- three runs of nCells doubles (accumulated rain, the last
    // call's, the calls), not registry fields -- allocated and zeroed on first use (precip_ensure: when the option
    // is set, or at the first direct call; never inside a capture)
    int microphysics = 0;
    double* precip = nullptr;
    // option "pbl" (the MPAS dynamics, physics = 2): 1 -- atm_srk3 ends with the surface-flux and boundary-layer
    // task (k_pbl.hip) over the step's dt, behind the Kessler task, inside the captured graph; 0: the step is launch
    // for launch the step without it.  sst: the configured surface temperature per local cell
    // (mpas_surface_set_temperature; nullptr until then); sflux: the task's accumulators -- three runs of nCells
    // doubles (accumulated evaporation, the last call's, the calls), not registry fields -- allocated and zeroed on
    // first use (sflux_ensure: never inside a capture)
    int pbl = 0;
    double* sst = nullptr;
    double* sflux = nullptr;
    int self_on = 1;  // option "self": allow the SELF gathers when the mesh permits
    int self_ok = 0;   // k_prepare's verdict on the uploaded mesh
    int overlap = 1;   // option "overlap": halo exchanges beside interior compute
    // option "hfuse": independent neighbouring kernels share a launch (same values); 2 = on
    // where the grids do not fill the chip (hfuse_auto_cells), the case it pays in
    // (x1.2562: -3 %; x1.163842: +0.8 %, the pair runs at the lower occupancy of the two)
    int hfuse = 2;
    int fusesml = 1;    // option "fusesml": each stage's set_smlstep inside its first acoustic launch (with fusedamp)
    int smlsum = 1;     // option "smlsum": its slope-flux sum once per step (fast path, with fusesml)
    int fusedamp_halo = 1;  // option "fusedamp_halo": fusedamp / fusesml on decomposed meshes too
    int tmedge = 0;     // option "tmedge": theta_m edge sums from dyn_tend for the acoustic substeps (same values;
                        // measured slower at both sizes)
    int fusecopy = 1;   // option "fusecopy" (with fusesetup): setup's edge copies made by stage 0's dyn_tend
                        // edge kernel from the columns it loads anyway (same values)
    int fusesetup = 1;  // option "fusesetup": stage 0's setup, moist and vert_imp in one launch (same values)
    int vdyn = 1;      // option "vdyn": atm_srk3's stage 2 dyn_tend edge kernel stores solve_diagnostics' v
                       // (reference semantics, edgesOnEdge_ECP = edgesOnEdge; same values)
    int defer4 = 1;    // option "defer4": atm_srk3 applies rk_step 0's del4 of tend_u_euler (dyn_tend D) in the
                       // next stage's rk_step > 0 edge kernel (reference semantics; same values)
    int msml = 1;      // option "msml" (the MPAS dynamics): each stage's set_smlstep applied by dyn_tend's E to
                       // the tend_w it forms (no task reads tend_w in between)
    int mru = 1;       // option "mru" (the MPAS dynamics, fast path): the kernel forming a stage's final tend_u
                       // stores its first acoustic substep's ru_p / ruAvg (k_acoustic_ru FIRST skipped)
    int mdamp = 1;     // option "mdamp" (the MPAS forms): each divergence damping applied by the kernel that next
                       // reads ru_p -- the next substep's k_acoustic_ru, or the stage's recover edge kernel
    int ntu = 1;       // option "ntu" (with defer4): that rk_step 0 call's whole tend_u is dead (the next stage's
                       // edge kernel rewrites it, no task in between reads it): its edge kernel forms none of
                       // it and skips its gathers (k_dyn_B NTU; the same values of everything read later)
    int accoef = 1;    // option "accoef" (atm_srk3, reference semantics): the acoustic launches form cofwr, coftz
                       // and a_tri from the columns they hold instead of loading them; stage 0's setup launch
                       // does not store the three, vert_imp takes coftz's level L from the keep tail (same bits)
    int dd0 = 1;       // option "dd0" (atm_srk3, reference semantics): the acoustic launches take rw_save - rw as
                       // the constant 0.0 -- the setup stores rw_save = rw where the difference is read and no
                       // task of the step writes rw -- and load neither column, nor X_Dd (same bits for finite rw)
    int smlkeep = 1;   // option "smlkeep" (with smlsum, undecomposed): X_smlS is formed when its inputs may have
                       // changed (sml_valid below), ahead of the step, not in every step
    // X_smlS (and X_Dd without dd0) hold what the flux kernel would form now.  Set by srk3_step when it has run
    // the kernel; cleared by every public entry point but the step itself and the pure queries (guarded()):
    // the sum's inputs -- u_tend, zb_cell, zb3_cell, edgesOnCell_sign, fzm, fzp, the mesh lists, rw -- have no
    // writer among the step's tasks, so only a call from outside can change them
    bool sml_valid = false;
    // option "stepkeep" (reference semantics, where StepForm::stepkeep holds): no task of the step
    // writes u, ru, rw, rho_zz, theta_m, rho_p, rtheta_p, h, zz, exner or the base fields, so most of what a step
    // stores is what the step before stored.  keep_gen counts the steps completed since the last call from
    // outside that could have changed a field or the form of the step (0, 1, 2: sml_valid generalised; cleared
    // where it is cleared, and by a step with another dt or schedule than keep_dt / keep_schedule):
    //   >= 1 (a full step has run): neither solve_diagnostics launch runs -- their outputs are functions of u
    //        and h alone --, and the setup launch stores only w_2 and vert_imp's columns (k_setup_vi KEPT);
    //   2, with stepkeep = 2 only (a generation-1 step has run, whose stage 0 read the step's own diagnostics):
    //        stage 0's dyn_tend does not run -- everything it stores is final but w, restored from the copy the
    //        generation-1 step took (X_w0) -- and stage 2 forms tend_u, v and w alone.
    //   >= 1 also: stage 2's dyn_tend runs without its kernel A -- at rk_step > 0 A stores h_divergence alone, a
    //        function of ru and the mesh, final from the full step on (its row keeps its tags, with -A)
    // 1 is the default; 2 changes which dyn_tend rows a timed step has
    int stepkeep = 1;
    // option "vikeep" (where stepkeep is active): vert_imp's two coefficient sets -- stage 0's, dts
    // = dt / 3, and stage 1's -- are functions of fields no task of the step writes, but for alpha_tri / gamma_tri
    // (Q17's stale gamma).  Stage 0's set lives in scratch (X_cofwt0, X_cofwz0, X_a0, X_b0, X_c0) in every
    // generation, so the fields keep stage 1's; at keep_gen >= 1 both launches form alpha_tri / gamma_tri alone
    // from the stored a, b, c.  Invalidation is keep_gen's: a full step rewrites every one of them first
    int vikeep = 1;
    // option "a0keep" (where stepkeep is active): everything stage 0's dyn_tend kernel A stores --
    // tend_rho, dpdz, the w scratch X_wc, setup's copies ru_save / u_2 -- is a function of fields no task of the
    // step writes, but kdiff, which reads v: stage 2 of a full step leaves another v than the one its own stage 0
    // read.  A full step therefore ends with one launch that forms the next step's kdiff into X_kd0; a step at
    // keep_gen >= 1 copies it into kdiff in its setup launch, runs stage 0's dyn_tend without A (B stays the
    // instance that loads neither u nor ru) and the finish without its edge part (ruAvg has no writer, so
    // ruAvg_split = ruAvg is the identity).  Invalidation is keep_gen's
    int a0keep = 1;
    // option "dynkeep" (where a0keep is active and stepkeep is 1): what a kept step's dyn_tend
    // still forms from fields no task of the step writes -- stage 0's B, C and E, stage 1's and 2's E -- is
    // formed by the first kept step after a full one alone, which also leaves the columns the step rewrites
    // (tend_u_euler before its del4, each stage's w) in X_tue0 / X_w0..2.  The later kept steps launch the same
    // kernels, which copy those columns back and return: the decision is a device flag (X_dkf) the guarded
    // instances load, cleared by every full step and set by every kept one, so one captured graph serves both.
    // Invalidation is keep_gen's: an outside call leads to a full step, which clears the flag first
    int dynkeep = 1;
    // option "tukeep" (exactly where dynkeep is active): between two kept steps stage 2's edge
    // kernel stores other bits at one level of one column only -- tend_u at level L - 1, which reads w at level L;
    // tend_u_euler (final, del4 included), v and the rest of tend_u hold the step-before's, and its flux X_F has no
    // reader in a fresh kept step.  With X_dkf 1 the guarded instance of that kernel returns and k_dyn_B_top,
    // launched behind it in the same task, forms that one level from tend_u_euler as stored; stage 0's guarded edge
    // kernel then returns without copying X_tue0 back.  X_dkf 0: every launch as with dynkeep alone.  The same
    // launches either way: one captured graph, dynkeep's timing keys.  Invalidation is keep_gen's
    int tukeep = 1;
    int keep_gen = 0;
    double keep_dt = 0.0;
    int keep_schedule = -1;
    int fusedamp = 1;  // option "fusedamp": atm_srk3 applies each divergence damping inside the next
                       // acoustic launch (reference semantics, undecomposed; same bits)
    void* raw[X_COUNT] = {};  // the allocations behind S.f (S.f[f] = raw[f] + stagger)
    bool timing = false;
    bool dirty = true;  // derived mesh arrays need k_prepare
    std::vector<std::string> task_names;
    std::vector<int64_t> task_calls;
    std::vector<double> task_ms;
    std::vector<TimedCall> pending;
    std::vector<hipEvent_t> event_pool;
    std::unique_ptr<Halo> halo;           // decomposed mesh only
    std::shared_ptr<LoopGroup> loopgrp;   // in-process loopback transport
    int* gid_dev[3] = {nullptr, nullptr, nullptr};
    void* sum_scratch = nullptr;  // summarize_timestep partials (allocated on first use)
    double* sum_out = nullptr;
    // option "graph": mpas_atm_srk3 captured once per (dt, schedule) as a HIP graph and
    // replayed (one hipGraphLaunch per step instead of ~60 kernel launches); invalidated
    // by any option change or mesh upload; not used while per-task timing is on or on a
    // decomposed context (the halo bookkeeping is host-side per launch)
    int graph_on = 1;
    // decomposed contexts (option "graph_halo"; RCCL and stub transports -- the loopback's
    // host barriers cannot be captured): the halo bookkeeping is host-side and evolves
    // identically every step from a given state at the step's start, so that state is part
    // of a captured step's key (stale0), and a replay sets the host state to the one the
    // captured step ended in (stale1).  A few steps are kept, one per start state seen twice
    // (a standalone task or an upload between steps gives a second one)
    struct GraphEntry {
        double dt = 0.0;
        int schedule = -1;
        int gen = 0;  // (option stepkeep: the generation the captured step ran at)
        std::vector<uint8_t> stale0, stale1;
        int64_t exch = 0, fields = 0;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        uint64_t used = 0;
    };
    static constexpr size_t kGraphCache = 6;  // (two (dt, schedule) pairs at the three generations of stepkeep)
    std::vector<GraphEntry> graphs;
    uint64_t graph_clock = 0;
    int64_t graph_captures = 0, graph_launches = 0;
    // 2 (default): the stub transport only; 1: RCCL too (its grouped send / recv captured --
    // exercised on a 1-rank communicator only, which moves nothing); 0: off.  A capture that
    // fails on a transport falls back to eager steps (graph_fallbacks)
    int graph_halo = 2;
    int64_t graph_fallbacks = 0;
    // option "keep_check" (tests): after every task, every keep tail is compared with its
    // field on the owned entities (mpas_dev.h keep tails); a mismatch fails the task
    int keep_check = 0;
    int* keep_flag = nullptr;
    // set when a transport refused a capture: eager steps from then on (the user's graph_halo
    // stays as set; a new halo plan or a graph_halo option change clears it)
    bool graph_refused = false;
    std::vector<std::vector<uint8_t>> seen_stale0;  // start states stepped eagerly once
    // option "trtile": the tiled transport (k_transport.hip) when the mesh allows it; the
    // tiles are rebuilt after a mesh upload or a change of the owned / interior cells.
    // Off by default: measured 2x slower than the three kernels
    int trtile = 0;
    int trt_cells = TRT_CELLS, trt_clo = 96;  // options "trtcells", "trtclo": tile size limits (speed only)
    int trt_ghosts = 0;  // option "trtile_ghosts": a decomposed mesh's ghosts close over
                         // advCellsForEdge(edgesOnCell) (decomp.Decomposition(tiled_transport))
    bool trt_dirty = true;
    TrTiles trt;
    // option "tredge" (default 0: measured slower): the transport's edge kernel
    // with scalars_old staged in LDS per group of consecutive edges (undecomposed contexts;
    // rebuilt with the tiles)
    int tredge = 0;
    // option "trsave" (default 1; atm_srk3 with the transport, undecomposed, the default transport
    // kernels): scalars_save's copy folded into the transport -- its edge and bounds kernels read the old
    // scalars from scalars itself (nothing writes scalars before the transport's update) and the bounds
    // kernel stores them to scalars_old
    int trsave = 1;
    TrEdgeGroups tre;
    // option "etile" (default 1): dyn_tend's cell kernel E over compact tiles of cells, the tile's
    // theta_m closure staged in LDS, each edge's advCells flux formed there (k_dyn_Et) -- the edge
    // kernel then forms no flux and the per-edge scratch X_F goes (reference semantics, LP = 64,
    // undecomposed; the same bits either way).  Options "etcells" / "etclo": tile size limits
    int etile = 0;
    int ett_cells = 8, ett_clo = 56;
    bool ett_dirty = true;
    TrTiles ett;
};

namespace {

void ett_ensure(mpas_ctx* c);

struct Fail {
    int code;
    std::string msg;
};

void hipcheck(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Fail{MPAS_EHIP, std::string(what) + ": " + hipGetErrorString(e)};
}

int entity_count(const mpas_ctx* c, int kind) {
    switch (kind) {
        case K_C3: case K_C3V: case K_C2F: case K_C2I: case K_C3B: return c->dims.nCells;
        case K_E3: case K_E2F: case K_E2I: return c->dims.nEdges;
        case K_V3: case K_V2F: case K_V2I: return c->dims.nVertices;
        default: return 1;
    }
}
size_t elem_size(int kind) {
    if (kind == K_C2I || kind == K_E2I || kind == K_V2I) return 4;
    if (kind == K_C3B) return 1;
    return 8;
}
// bytes of one device array (entity rows include the zero slot)
size_t dev_bytes(const mpas_ctx* c, int f) {
    const FieldInfo& fi = kFields[f];
    const size_t LP = c->S.LP;
    size_t rows = (size_t)entity_count(c, fi.kind) + 1;
    switch (fi.kind) {
        // (width-1 fields: + the two keep tails of rows doubles each, mpas_dev.h keep_tail)
        case K_C3: case K_E3: case K_V3: return rows * fi.width * LP * 8 + (fi.width == 1 ? 2 * rows * 8 : 0);
        case K_C3V: return rows * fi.width * LP * 8;
        case K_C3B: return rows * LP;
        case K_ZV: return LP * 8;
        default: return rows * fi.width * elem_size(fi.kind);
    }
}
// Keep tails (mpas_dev.h): the fields a step kernel writes with the kept value of level L
// (kKeepL) or of level 0 (kKeep0) -- the slots the reference never writes there.  Their
// tails are set from the field after every write from outside the step kernels
// (keep_refresh); option "keep_check" compares them with the field after every task.
const int kKeepL[] = {
    // dyn_tend (A, D, E; B and C keep the reference's unwritten slots)
    F_kdiff, F_h_divergence, F_tend_rho, F_dpdz, F_v, F_ru_save, F_u_2, F_tend_u_euler, F_tend_u,
    F_tend_w_euler, F_tend_theta_euler, F_tend_rtheta_adv, F_w, F_rthdynten, F_tend_theta,
    // vert_imp
    F_coftz, F_cofwt, F_cofwr, F_cofwz, F_a_tri, F_b_tri, F_c_tri, F_alpha_tri, F_gamma_tri,
    // solve_diagnostics (its edge kernel)
    F_h_edge, F_ke_edge, F_rho_edge, F_pv_edge,
    // setup + moist
    F_cqu, F_rw_save, F_rtheta_p_save, F_rho_p_save, F_w_2, F_theta_m_2, F_rho_zz_2, F_rho_zz_old_split,
    F_theta_m_save, F_qtot, F_cqw,
    // acoustic
    F_rtheta_pp_old, F_rho_pp, F_rtheta_pp,
    // recover (the MPAS forms)
    F_rho_p, F_rho_zz, F_rtheta_p, F_theta_m, F_exner, F_pressure_p, F_rw, F_ru, F_u,
    // substep_finish
    F_wwAvg_split, F_ruAvg_split,
    // mpas_reconstruct_2d
    F_uReconstructX, F_uReconstructY, F_uReconstructZ, F_uReconstructZonal, F_uReconstructMeridional,
    // the Held-Suarez forcing
    F_tend_rtheta_physics, F_tend_ru_physics,
    // the Kessler microphysics (its other fields: recover's)
    F_rt_diabatic_tend};
const int kKeep0[] = {F_cofwr, F_cofwz, F_a_tri, F_b_tri, F_c_tri, F_alpha_tri, F_cqw, F_rw};
int keep_kind(int f) { return kFields[f].kind == K_C3 ? 0 : kFields[f].kind == K_E3 ? 1 : 2; }  // KC / KE / KV

void keep_refresh_all(mpas_ctx* c) {
    for (int f : kKeepL) hipcheck(launch_keep_refresh(c->S, c->stream, f, keep_kind(f)), "keep_refresh");
    for (int f : kKeep0) hipcheck(launch_keep_refresh(c->S, c->stream, f, keep_kind(f)), "keep_refresh");
}
void keep_verify(mpas_ctx* c, const char* task) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hipcheck(hipStreamIsCapturing(c->stream, &cs), "hipStreamIsCapturing");
    if (cs != hipStreamCaptureStatusNone) return;  // (a captured step is checked when it runs eagerly)
    if (!c->keep_flag) hipcheck(hipMalloc(&c->keep_flag, 8 * sizeof(int)), "hipMalloc");
    hipcheck(hipMemsetAsync(c->keep_flag, 0, 7 * sizeof(int), c->stream), "hipMemsetAsync");
    hipcheck(hipMemsetAsync(c->keep_flag + 7, 0x7f, sizeof(int), c->stream), "hipMemsetAsync");
    for (int f : kKeepL) hipcheck(launch_keep_check(c->S, c->stream, f, keep_kind(f), 0, c->keep_flag), "keep_check");
    for (int f : kKeep0) hipcheck(launch_keep_check(c->S, c->stream, f, keep_kind(f), 1, c->keep_flag), "keep_check");
    int fl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipcheck(hipMemcpyAsync(fl, c->keep_flag, sizeof(fl), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
    hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    if (fl[0]) {
        double v[2];
        std::memcpy(v, fl + 2, sizeof v);
        throw Fail{MPAS_EINVAL, std::string(task) + ": keep tail of " + kFields[(fl[0] - 1) / 2].name + " (level " +
                                    ((fl[0] - 1) % 2 ? "0" : "L") + ") differs from the field at entity " +
                                    std::to_string(fl[1]) + ": field " + std::to_string(v[0]) + ", tail " +
                                    std::to_string(v[1]) + "; " + std::to_string(fl[6]) +
                                    " mismatches, the first at entity " + std::to_string(fl[7]) + " (keep_check)"};
    }
}

// entity kind an integer field refers to (for the Q1 clamp), -1 if it is not an id
int id_target(int f) {
    switch (f) {
        case F_edgesOnCell: case F_edgesOnEdge: case F_edgesOnEdge_ECP: case F_edgesOnVertex: return K_E3;
        case F_cellsOnEdge: case F_advCellsForEdge: case F_cellsOnCell: case F_cellsOnVertex: return K_C3;
        case F_verticesOnEdge: case F_verticesOnCell: return K_V3;
        default: return -1;
    }
}

// true when p is device memory (a device-resident view: Legion framebuffer instance,
// torch tensor); host, pinned-host and unregistered pointers are host views
bool is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // unregistered host memory reports an error: clear it
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}
// bytes a strided view of n entities x W components x levels 0..Lv spans (non-negative strides)
size_t view_span(int n, int W, int Lv, int64_t se, int64_t sl, int64_t sc, size_t elem) {
    if (n <= 0) return 0;
    if (se < 0 || sl < 0 || sc < 0) throw Fail{MPAS_EINVAL, "device views need non-negative strides"};
    return (size_t)((int64_t)(n - 1) * se + (int64_t)Lv * sl + (int64_t)(W - 1) * sc) + elem;
}
bool is_3d(int kind) { return kind == K_C3 || kind == K_E3 || kind == K_V3 || kind == K_C3V || kind == K_C3B; }

// width of the id rows a count field gives the length of (0: not a count)
int count_width(int f) {
    switch (f) {
        case F_nEdgesOnCell: return 10;      // edgesOnCell, verticesOnCell, cellsOnCell, edgesOnCell_sign, ...
        case F_nEdgesOnEdge: return 20;      // edgesOnEdge, weightsOnEdge
        case F_nAdvCellsForEdge: return 15;  // advCellsForEdge, adv_coefs(_3rd)
        default: return 0;
    }
}

int task_index(mpas_ctx* c, const char* name) {
    for (size_t i = 0; i < c->task_names.size(); i++)
        if (c->task_names[i] == name) return (int)i;
    c->task_names.push_back(name);
    c->task_calls.push_back(0);
    c->task_ms.push_back(0.0);
    return (int)c->task_names.size() - 1;
}

hipEvent_t get_event(mpas_ctx* c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipcheck(hipEventCreate(&e), "hipEventCreate");
    return e;
}

void harvest(mpas_ctx* c) {
    for (auto& t : c->pending) {
        hipcheck(hipEventSynchronize(t.e1), "hipEventSynchronize");
        float ms = 0.f;
        hipcheck(hipEventElapsedTime(&ms, t.e0, t.e1), "hipEventElapsedTime");
        c->task_calls[t.task] += 1;
        c->task_ms[t.task] += ms;
        c->event_pool.push_back(t.e0);
        c->event_pool.push_back(t.e1);
    }
    c->pending.clear();
}

// run a task launcher, bracketed by events when timing is on
// roctx ranges per task (SURVEY §5 tracing): env MPAS_ROCTX=1 loads libroctx64 at the
// first task and brackets every task launch, so rocprofv3 --marker-trace shows the
// Regent task names over their kernels.  Off: no library, no cost.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char* v = std::getenv("MPAS_ROCTX");
        if (!v || !*v || *v == '0') return;
        void* h = dlopen("libroctx64.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("/opt/rocm/lib/libroctx64.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
const Roctx& roctx() {
    static Roctx r;
    return r;
}

// the derived mesh arrays (k_prepare), where an upload or an init task has left them stale
void prepare_mesh(mpas_ctx* c) {
    if (!c->dirty) return;
    hipcheck(launch_prepare(c->S, c->stream), "prepare");
    c->self_ok = c->S.selfc;
    c->S.selfc = c->self_ok && c->self_on;
    c->dirty = false;
}

template <class Fn>
void run_task(mpas_ctx* c, const char* name, Fn&& fn) {
    const Roctx& rx = roctx();
    if (rx.push) rx.push(name);
    struct Pop {
        const Roctx& r;
        ~Pop() {
            if (r.pop) r.pop();
        }
    } pop_at_exit{rx};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int ti = -1;
    if (c->timing) {
        ti = task_index(c, name);
        e0 = get_event(c);
        e1 = get_event(c);
        hipcheck(hipEventRecord(e0, c->stream), "hipEventRecord");
    }
    prepare_mesh(c);
    ett_ensure(c);  // (built before a capture by prepare_now)
    hipError_t e = fn();
    if (e != hipSuccess) {
        if (c->halo && !c->halo->err.empty())
            throw Fail{MPAS_ERCCL, std::string(name) + ": halo exchange: " + c->halo->err};
        throw Fail{MPAS_EHIP, std::string(name) + ": " + hipGetErrorString(e)};
    }
    if (c->halo && !c->halo->race.empty()) throw Fail{MPAS_EINVAL, std::string(name) + ": " + c->halo->race};
    if (c->keep_check) keep_verify(c, name);
    if (c->timing) {
        hipcheck(hipEventRecord(e1, c->stream), "hipEventRecord");
        c->pending.push_back({ti, e0, e1});
        if (c->pending.size() > 4096) harvest(c);
    }
}

// ---- bounds-checked build (mpas_dev.h MPAS_BOUNDS): the field table the kernels check
// against, and the check after every C-ABI call (which then synchronises the context)
#if MPAS_BOUNDS
struct BoundsReg {
    std::mutex mu;
    std::map<unsigned long long, std::pair<unsigned long long, std::string>> fields;  // lo -> (hi, name)
    BoundsTab* dev = nullptr;
};
BoundsReg& bounds_reg() {
    static BoundsReg r;
    return r;
}
// upload the sorted field ranges (every live context) and point each unit's table at them
void bounds_publish() {
    BoundsReg& r = bounds_reg();
    std::lock_guard<std::mutex> lk(r.mu);
    if (r.fields.size() > (size_t)kBoundsMax) throw Fail{MPAS_ENOMEM, "bounds table full"};
    hipcheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (!r.dev) {
        hipcheck(hipMalloc(&r.dev, sizeof(BoundsTab)), "hipMalloc");
        hipcheck(hipMemset(r.dev, 0, sizeof(BoundsTab)), "hipMemset");
        for (auto sym : bounds_tus()) {
            void* p = sym();
            if (!p) throw Fail{MPAS_EHIP, "bounds table symbol not found"};
            hipcheck(hipMemcpy(p, &r.dev, sizeof(r.dev), hipMemcpyHostToDevice), "hipMemcpy bounds");
        }
    }
    std::vector<unsigned long long> lo, hi;
    for (auto& kv : r.fields) lo.push_back(kv.first), hi.push_back(kv.second.first);
    const int n = (int)lo.size();
    if (n) {
        hipcheck(hipMemcpy(r.dev->lo, lo.data(), n * sizeof(lo[0]), hipMemcpyHostToDevice), "hipMemcpy bounds");
        hipcheck(hipMemcpy(r.dev->hi, hi.data(), n * sizeof(hi[0]), hipMemcpyHostToDevice), "hipMemcpy bounds");
    }
    hipcheck(hipMemcpy(&r.dev->n, &n, sizeof(n), hipMemcpyHostToDevice), "hipMemcpy bounds");
}
void bounds_add(mpas_ctx* c) {
    {
        BoundsReg& r = bounds_reg();
        std::lock_guard<std::mutex> lk(r.mu);
        for (int f = 0; f < X_COUNT; f++) {
            const unsigned long long lo = (unsigned long long)c->S.f[f];
            // (the columns only: the keep tails behind them are reached by keepv / keep_put alone)
            const FieldInfo& fi = kFields[f];
            const bool tails = (fi.kind == K_C3 || fi.kind == K_E3 || fi.kind == K_V3) && fi.width == 1;
            const size_t cols = dev_bytes(c, f) - (tails ? 2 * ((size_t)entity_count(c, fi.kind) + 1) * 8 : 0);
            r.fields[lo] = {lo + cols, kFields[f].name};
        }
    }
    bounds_publish();
}
void bounds_remove(mpas_ctx* c) {
    {
        BoundsReg& r = bounds_reg();
        std::lock_guard<std::mutex> lk(r.mu);
        for (int f = 0; f < X_COUNT; f++)
            if (c->S.f[f]) r.fields.erase((unsigned long long)c->S.f[f]);
    }
    try {
        bounds_publish();
    } catch (const Fail&) {
    }
}
// translation units whose table pointer is set (read back from each unit's symbol)
int bounds_units() {
    BoundsReg& r = bounds_reg();
    int n = 0;
    for (auto sym : bounds_tus()) {
        void* p = sym();
        BoundsTab* t = nullptr;
        if (p && hipMemcpy(&t, p, sizeof(t), hipMemcpyDeviceToHost) == hipSuccess && t && t == r.dev) n++;
    }
    return n;
}
void bounds_check(mpas_ctx* c) {
    BoundsReg& r = bounds_reg();
    if (!r.dev || !c->stream) return;
    hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    unsigned int count = 0;
    hipcheck(hipMemcpy(&count, &r.dev->count, sizeof(count), hipMemcpyDeviceToHost), "hipMemcpy bounds");
    if (!count) return;
    unsigned long long addr = 0, flo = 0, where = 0;
    hipcheck(hipMemcpy(&addr, &r.dev->addr, sizeof(addr), hipMemcpyDeviceToHost), "hipMemcpy bounds");
    hipcheck(hipMemcpy(&flo, &r.dev->field_lo, sizeof(flo), hipMemcpyDeviceToHost), "hipMemcpy bounds");
    hipcheck(hipMemcpy(&where, &r.dev->where, sizeof(where), hipMemcpyDeviceToHost), "hipMemcpy bounds");
    const unsigned int zero = 0;
    hipcheck(hipMemcpy(&r.dev->count, &zero, sizeof(zero), hipMemcpyHostToDevice), "hipMemcpy bounds");
    std::string name = "?";
    unsigned long long fhi = 0;
    {
        std::lock_guard<std::mutex> lk(r.mu);
        auto it = r.fields.find(flo);
        if (it != r.fields.end()) name = it->second.second, fhi = it->second.first;
    }
    char msg[256];
    snprintf(msg, sizeof msg, "%u access(es) outside their field; first: field %s, byte %lld of %llu (block %llu thread %llu)",
             count, name.c_str(), (long long)(addr - flo), fhi - flo, where >> 32, where & 0xffffffffull);
    throw Fail{MPAS_EBOUNDS, msg};
}
#else
void bounds_add(mpas_ctx*) {}
void bounds_remove(mpas_ctx*) {}
void bounds_check(mpas_ctx*) {}
#endif

// keeps_sml: the call leaves the kept flux sum (mpas_ctx::sml_valid) as it is.  The rule is "every entry
// point clears it but ...", decided here once, not "these entry points clear it": an upload, a fill, a
// standalone or init task, an option change or a halo call may each change an input of the sum or the form
// of the step, and an entry point added later is then safe without anyone thinking of the flag.  The
// exceptions pass keeps_sml: the step itself (no task of it writes an input) and the calls that write no
// device field and no option -- download, sync, get_option, the timing calls, summarize_timestep (the
// queries that never reach here, mpas_get_stream, mpas_field_*, mpas_halo_stats, mpas_last_error, touch
// nothing either)
template <class Fn>
int guarded(mpas_ctx* c, Fn&& fn, bool keeps_sml = false) {
    if (!c) return MPAS_EINVAL;
    if (!keeps_sml) c->sml_valid = false, c->keep_gen = 0;
    try {
        fn();
        if (MPAS_BOUNDS) bounds_check(c);
        return MPAS_OK;
    } catch (const Fail& f) {
        c->err = f.msg;
        return f.code;
    } catch (const std::bad_alloc&) {
        c->err = "out of host memory";
        return MPAS_ENOMEM;
    } catch (const std::exception& ex) {
        c->err = ex.what();
        return MPAS_EINVAL;
    } catch (...) {
        c->err = "unknown error";
        return MPAS_EINVAL;
    }
}

// ---- tiled transport: the cell tiles (TrTiles, mpas_dev.h) ----
void tiles_free(TrTiles& T);
void trt_free(mpas_ctx* c) {
    tiles_free(c->trt);
    c->S.trt = nullptr;
}
template <class V>
V* dev_copy(const std::vector<V>& h) {
    V* d = nullptr;
    hipcheck(hipMalloc(&d, sizeof(V) * (h.empty() ? 1 : h.size())), "hipMalloc");
    if (!h.empty()) hipcheck(hipMemcpy(d, h.data(), sizeof(V) * h.size(), hipMemcpyHostToDevice), "hipMemcpy H2D");
    return d;
}
template <class V>
std::vector<V> dev_read(const void* d, size_t n) {
    std::vector<V> h(n);
    hipcheck(hipMemcpy(h.data(), d, sizeof(V) * n, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    return h;
}

// Compact tiles of at most TRT_CELLS owned cells, grown breadth-first over the cells'
// edge neighbours from the lowest unassigned cell id, within one launch class of a
// decomposed mesh (below), and closed
// before the closure -- the cells whose scalars_old the tile's kernels read, as the ids
// on the device resolve -- would exceed trt_clo LDS columns (default 96: 48 KB at LP = 64,
// three blocks per CU).  Not built (the three-kernel path runs) when an owned cell has more
// than NF edges or one of its edges more than AF advCells.
// The edge groups of k_tr_edge_lds (TrEdgeGroups, mpas_dev.h): TRE_GE consecutive owned
// edges per group; LDS columns in first-use order over the group's edges (advCells, then
// the two cells of the edge).
void tre_free(mpas_ctx* c) {
    TrEdgeGroups& G = c->tre;
    for (void* p : {(void*)G.ucell, (void*)G.ucnt, (void*)G.eslot})
        if (p) (void)hipFree(p);
    G = TrEdgeGroups{};
    c->S.tre = nullptr;
}
void tre_build(mpas_ctx* c) {
    tre_free(c);
    if (!c->tredge || c->halo || c->S.LP != 64) return;
    const DevState& S = c->S;
    const int nE = S.nEdges, nEO = S.nEO;
    if (nEO <= 0) return;
    const auto coe = dev_read<int>(S.f[F_cellsOnEdge], ((size_t)nE + 1) * 2);
    const auto adv = dev_read<int>(S.f[F_advCellsForEdge], ((size_t)nE + 1) * 15);
    const auto nadv = dev_read<int>(S.f[F_nAdvCellsForEdge], (size_t)nE + 1);
    const int ng = (nEO + TRE_GE - 1) / TRE_GE;
    std::vector<int> ucell((size_t)ng * TRE_U, 0), ucnt(ng, 0);
    std::vector<unsigned char> eslot((size_t)nEO * TRE_ROW, 0);
    int nirr = 0;
    for (int g = 0; g < ng; g++) {
        std::vector<int> u;
        bool ok = true;
        auto slot_of = [&](int cell) {
            for (size_t i = 0; i < u.size(); i++)
                if (u[i] == cell) return (int)i;
            u.push_back(cell);
            return (int)u.size() - 1;
        };
        for (int e = g * TRE_GE; e < std::min(nEO, (g + 1) * TRE_GE) && ok; e++) {
            const int na = nadv[e];
            if (na > AF) ok = false;
            unsigned char* r = &eslot[(size_t)e * TRE_ROW];
            for (int j = 0; j < AF && ok; j++) r[j] = (unsigned char)slot_of(adv[(size_t)e * 15 + j]);
            r[AF] = (unsigned char)slot_of(coe[(size_t)e * 2]);
            r[AF + 1] = (unsigned char)slot_of(coe[(size_t)e * 2 + 1]);
            if ((int)u.size() > TRE_U) ok = false;
        }
        if (!ok) {
            ucnt[g] = -1;
            nirr++;
            continue;
        }
        ucnt[g] = (int)u.size();
        for (int i = 0; i < TRE_U; i++) ucell[(size_t)g * TRE_U + i] = i < (int)u.size() ? u[i] : u[0];
    }
    TrEdgeGroups& G = c->tre;
    G.ngroups = ng;
    G.neo = nEO;
    G.nirr = nirr;
    G.ucell = dev_copy(ucell);
    G.ucnt = dev_copy(ucnt);
    std::vector<unsigned> packed(eslot.size() / 4);
    std::memcpy(packed.data(), eslot.data(), eslot.size());
    G.eslot = dev_copy(packed);
    c->S.tre = &c->tre;
}

void tiles_free(TrTiles& T) {
    for (void* p : {(void*)T.tptr, (void*)T.tcell, (void*)T.cptr, (void*)T.ccell, (void*)T.slot, (void*)T.teptr,
                    (void*)T.tedge, (void*)T.erow, (void*)T.terec})
        if (p) (void)hipFree(p);
    T = TrTiles{};
}
// the tiles (into T) of at most `cells` owned cells whose closure fits `clo_max` LDS columns;
// false (T empty) when the mesh does not allow them
bool tiles_build(mpas_ctx* c, TrTiles& T, int max_cells, int clo_max, int te_max = 1 << 30);

void trt_build(mpas_ctx* c) {
    trt_free(c);
    tre_free(c);
    c->trt_dirty = false;
    tre_build(c);
    if (!c->trtile) return;
    if (c->halo && !c->trt_ghosts) return;  // the tiles would read ghosts the local mesh lacks
    if (tiles_build(c, c->trt, c->trt_cells, c->trt_clo)) c->S.trt = &c->trt;
}

// option "etile": dyn_tend's cell kernel E over tiles of cells with the tile's theta_m closure
// in LDS (k_dyn_Et, k_dyn.hip); reference semantics, LP = 64, undecomposed
void ett_free(mpas_ctx* c) {
    tiles_free(c->ett);
    c->S.ett = nullptr;
}
void ett_build(mpas_ctx* c) {
    ett_free(c);
    c->ett_dirty = false;
    if (!c->etile || c->halo || c->S.LP != 64 || c->S.physics == 2) return;
    // (at most 96 edges per tile: the LDS of a block, (closure + 1 + edges) columns, stays < 160 KiB)
    if (tiles_build(c, c->ett, c->ett_cells, c->ett_clo, 96)) c->S.ett = &c->ett;
}
void ett_ensure(mpas_ctx* c) {
    if (c->ett_dirty) ett_build(c);
}

bool tiles_build(mpas_ctx* c, TrTiles& T, int max_cells, int clo_max, int te_max) {
    hipcheck(hipSetDevice(c->device), "hipSetDevice");
    const DevState& S = c->S;
    const int nC = S.nCells, nE = S.nEdges, nCO = S.nCO;
    const int nint = (c->halo && c->halo->interior) ? c->halo->nint[0] : nCO;
    const auto nEoC = dev_read<int>(S.f[F_nEdgesOnCell], (size_t)nC + 1);
    const auto eoc = dev_read<int>(S.f[F_edgesOnCell], ((size_t)nC + 1) * 10);
    const auto coe = dev_read<int>(S.f[F_cellsOnEdge], ((size_t)nE + 1) * 2);
    const auto adv = dev_read<int>(S.f[F_advCellsForEdge], ((size_t)nE + 1) * 15);
    const auto nadv = dev_read<int>(S.f[F_nAdvCellsForEdge], (size_t)nE + 1);
    auto nedges = [&](int x) { return nEoC[x] > 0 ? nEoC[x] : 0; };
    for (int x = 0; x < nCO; x++) {
        if (nEoC[x] > NF) return false;
        for (int i = 0; i < nedges(x); i++)
            if (nadv[eoc[(size_t)x * 10 + i]] > AF) return false;
    }
    // the columns cell x's kernels read: x, both cells of each edge, the edge's advCells
    auto need = [&](int x, auto&& f) {
        f(x);
        for (int i = 0; i < nedges(x); i++) {
            const size_t e = (size_t)eoc[(size_t)x * 10 + i];
            f(coe[e * 2]);
            f(coe[e * 2 + 1]);
            for (int j = 0; j < nadv[e]; j++) f(adv[e * 15 + j]);
        }
    };
    std::vector<int> mark((size_t)nC + 1, -1), seen((size_t)nC + 1, -1), inq((size_t)nC + 1, -1);
    std::vector<char> assigned((size_t)nC + 1, 0);
    std::vector<int> tptr{0}, tcell, cptr{0}, ccell, queue, cells, clo;
    std::vector<int> slot;
    int stamp = 0, maxclo = 0, nt_int = 0;
    std::vector<int> emark((size_t)nE + 1, -1), tmark((size_t)nE + 1, -1), tedge, teptr{0};
    std::vector<unsigned> erow, terec;
    int tebase = 0, maxte = 0;
    // launch classes: 0 = interior cells whose every column is owned (or the zero slot),
    // run beside a halo exchange; 1 = the rest (boundary cells, and interior cells that
    // reach a ghost through advCellsForEdge(edgesOnCell), which the halo's interior
    // classification does not follow), run after it
    std::vector<char> cls_of((size_t)nC + 1, 1);
    for (int x = 0; x < nint; x++) {
        bool own = true;
        need(x, [&](int y) { own = own && (y < nCO || y == nC); });
        cls_of[x] = own ? 0 : 1;
    }
    for (int cls = 0; cls < 2; cls++) {
        const int lo = 0, hi = nCO;
        for (int seed = lo; seed < hi; seed++) {
            if (assigned[seed] || cls_of[seed] != cls) continue;
            const int tid = (int)tptr.size();
            cells.clear();
            clo.clear();
            queue.assign(1, seed);
            inq[seed] = tid;
            int nte = 0;  // the tile's edges so far (tmark: the tile id of an edge's last use)
            for (size_t qh = 0; qh < queue.size() && (int)cells.size() < max_cells; qh++) {
                const int x = queue[qh];
                int add = 0, adde = 0;
                stamp++;
                need(x, [&](int y) {
                    if (mark[y] < 0 && seen[y] != stamp) seen[y] = stamp, add++;
                });
                for (int i = 0; i < nedges(x); i++) adde += tmark[eoc[(size_t)x * 10 + i]] != tid;
                if (!cells.empty() && ((int)clo.size() + add > clo_max || nte + adde > te_max)) continue;
                for (int i = 0; i < nedges(x); i++) {
                    const int e = eoc[(size_t)x * 10 + i];
                    if (tmark[e] != tid) tmark[e] = tid, nte++;
                }
                cells.push_back(x);
                assigned[x] = 1;
                need(x, [&](int y) {
                    if (mark[y] < 0) mark[y] = (int)clo.size(), clo.push_back(y);
                });
                for (int i = 0; i < nedges(x); i++) {
                    const size_t e = (size_t)eoc[(size_t)x * 10 + i];
                    for (int side = 0; side < 2; side++) {
                        const int y = coe[e * 2 + side];
                        if (y >= lo && y < hi && cls_of[y] == cls && !assigned[y] && inq[y] != tid)
                            inq[y] = tid, queue.push_back(y);
                    }
                }
            }
            for (int x : cells) {  // the tile's edges (first use) and each cell's record of them (ETT_REC)
                unsigned char r[ETT_REC] = {};
                const int zero = (int)clo.size();  // (the zero column after the closure's)
                for (int i = 0; i < NF; i++) {
                    unsigned char* ri = r + i * ETT_EB;
                    for (int j = 0; j < AF; j++) ri[1 + j] = (unsigned char)zero;
                    if (i >= nedges(x)) continue;
                    const int e = eoc[(size_t)x * 10 + i];
                    if (emark[e] < 0) {
                        emark[e] = (int)tedge.size() - tebase;
                        tedge.push_back(e);
                        unsigned char er[ETT_ER] = {};  // the edge's advCells' closure columns (zero column past nAdv)
                        for (int j = 0; j < AF; j++) er[j] = (unsigned char)(j < nadv[e] ? mark[adv[(size_t)e * 15 + j]] : zero);
                        const unsigned* ew = (const unsigned*)er;
                        terec.insert(terec.end(), ew, ew + ETT_ER / 4);
                    }
                    ri[0] = (unsigned char)emark[e];
                    for (int j = 0; j < nadv[e]; j++) ri[1 + j] = (unsigned char)mark[adv[(size_t)e * 15 + j]];
                }
                const unsigned* rw = (const unsigned*)r;
                erow.insert(erow.end(), rw, rw + ETT_REC / 4);
            }
            for (int x : cells) {  // the LDS rows
                int row[TRT_ROW] = {};
                row[0] = mark[x];
                for (int i = 0; i < nedges(x); i++) {
                    const size_t e = (size_t)eoc[(size_t)x * 10 + i];
                    int* ri = row + 1 + i * (2 + AF);
                    ri[0] = mark[coe[e * 2]];
                    ri[1] = mark[coe[e * 2 + 1]];
                    for (int j = 0; j < nadv[e]; j++) ri[2 + j] = mark[adv[e * 15 + j]];
                }
                slot.insert(slot.end(), row, row + TRT_ROW);
                tcell.push_back(x);
            }
            for (int y : clo) mark[y] = -1, ccell.push_back(y);
            for (size_t q = tebase; q < tedge.size(); q++) emark[tedge[q]] = -1;
            maxte = std::max(maxte, (int)tedge.size() - tebase);
            tebase = (int)tedge.size();
            teptr.push_back(tebase);
            maxclo = std::max(maxclo, (int)clo.size());
            tptr.push_back((int)tcell.size());
            cptr.push_back((int)ccell.size());
        }
        if (cls == 0) nt_int = (int)tptr.size() - 1;
    }
    T.ntiles = (int)tptr.size() - 1;
    T.nt_int = nt_int;
    T.nco = nCO;
    T.nint = nint;
    T.maxclo = maxclo;
    T.tptr = dev_copy(tptr);
    T.tcell = dev_copy(tcell);
    T.cptr = dev_copy(cptr);
    T.ccell = dev_copy(ccell);
    T.slot = dev_copy(slot);
    T.nclo = (int)ccell.size();
    T.teptr = dev_copy(teptr);
    T.tedge = dev_copy(tedge);
    T.erow = dev_copy(erow);
    T.terec = dev_copy(terec);
    T.maxte = maxte;
    return true;
}
void trt_ensure(mpas_ctx* c) {
    if (c->trt_dirty) trt_build(c);
}

// timing keys: one Regent task, split where its read/write set (B_alg) differs by argument
// (bench.py aggregates the variants per task)
// (sml: option fusesml, the stage's set_smlstep run by this launch first; 2: from the step's flux sum X_smlS)
// (damp: option fusedamp, the previous substep's damping applied by this launch)
// (nold: a fused launch that does not store rtheta_pp_old -- every one but the step's last --
// tagged "-old" so that bench.py credits it no rtheta_pp_old write)
std::string acoustic_name(int small_step, bool damp = false, int sml = 0, bool nold = false) {
    return std::string("atm_advance_acoustic_step_work[") + (sml == 2 ? "ss0+smlS" : sml ? "ss0+sml" : small_step == 0 ? "ss0" : "ss>0") +
           (damp ? "+damp" : "") + (nold ? "-old" : "") + "]";
}
// a tag inside a key's closing bracket: tagged("task[ss0]", "-st") is "task[ss0-st]" (an empty tag: the key)
std::string tagged(std::string key, const char* tag) { return key.insert(key.size() - 1, tag); }

// the buffer pairs of the deferred damping (k_acoustic MODE 2), swapped by atm_srk3 after
// each launch; restored on exit (the ru_p pair by a copy if a step ended on the second
// buffer, which the reference schedule's even number of fused launches never does)
struct FuseBuffers {
    mpas_ctx* c;
    void *rup, *rupB, *dvA, *dvB;
    explicit FuseBuffers(mpas_ctx* c_) : c(c_) {
        rup = c->S.f[F_ru_p];
        rupB = c->S.f[X_rupB];
        dvA = c->S.f[X_dvA];
        dvB = c->S.f[X_dvB];
    }
    // (a decomposed context's halo keeps the ghost state of each buffer: it moves with it)
    void swap_rup() {
        std::swap(c->S.f[F_ru_p], c->S.f[X_rupB]);
        if (c->halo) std::swap(c->halo->stale[F_ru_p], c->halo->stale[X_rupB]);
    }
    void swap_dv() {
        std::swap(c->S.f[X_dvA], c->S.f[X_dvB]);
        if (c->halo) std::swap(c->halo->stale[X_dvA], c->halo->stale[X_dvB]);
    }
    void finish() {
        if (c->S.f[F_ru_p] != rup)
            hipcheck(hipMemcpyAsync(rup, c->S.f[F_ru_p], dev_bytes(c, F_ru_p), hipMemcpyDeviceToDevice, c->stream),
                     "hipMemcpyAsync ru_p");
        restore();
    }
    void restore() {
        const bool moved = c->S.f[X_rupB] != rupB || c->S.f[X_dvA] != dvA;
        c->S.f[F_ru_p] = rup;
        c->S.f[X_rupB] = rupB;
        c->S.f[X_dvA] = dvA;
        c->S.f[X_dvB] = dvB;
        // (ru_p's state moved with its data, which finish() copied back; the scratch
        // buffers hold anything)
        if (c->halo && moved) c->halo->stale[X_rupB] = c->halo->stale[X_dvA] = c->halo->stale[X_dvB] = 1;
    }
    ~FuseBuffers() { restore(); }
};
const char* recover_name(int rk_step) {
    return rk_step == 2 ? "atm_recover_large_step_variables_work[rk2]" : "atm_recover_large_step_variables_work[rk<2]";
}

// the RK3 transport's tasks have the default transport kernels only
void tr_rk_supported(mpas_ctx* c, const char* what) {
    if (c->trtile || c->tredge || c->S.trsu || c->S.trepw == 2)
        throw Fail{MPAS_ENOTSUP, std::string(what) + ": not with trtile, tredge, trsu or trepw = 2"};
}
// dyn_tend's timing key: the variant's read / write set (bench.py parses the tags)
std::string dyn_tend_key(const DynTendArgs& a) {
    return std::string("atm_compute_dyn_tend_work[") + (a.rk_step == 0 ? "rk0" : "rk>0") + (a.cp ? "+copy" : "") +
           (a.defer_out ? "+d4o" : "") + (a.ntu ? "+ntu" : "") + (a.defer_in ? "+d4i" : "") + (a.store_v ? "+v" : "") +
           (a.rud != 0.0 ? "+ru" : "") + (a.smlE ? "+sml" : "") + (a.skipA || a.keptA ? "-A" : "") + "]";
}

// ---- atm_srk3 (rk_timestep.rg:361-500) --------------------------------------------------
// StepForm: everything a step decides before its first launch, each condition once (step_form).  StepRun: what
// changes from launch to launch.  The stage functions below read both; srk3 is their sequence.

// option hfuse = 2: only below this many owned cells (a cell kernel then has fewer than ~16 wavefronts per
// SIMD: the launches do not fill the chip and their fixed cost dominates)
constexpr int hfuse_auto_cells = 16384;

struct StepForm {
    double dt;
    int schedule, gen;  // gen: the kept generation the step runs at (option stepkeep; 0: every launch of the step)
    // the reference's constants (rk_timestep.rg:378-399)
    int dynamics_split;
    double rk_sub_timestep[3];
    int number_sub_steps[3];
    int n_small[3];  // acoustic launches of each stage (Q5; the MPAS form: number_sub_steps), and of the step
    int n_acoustic;
    int rk_of[3];  // the rk_step argument of each stage's dyn_tend (Q4)
    // options as the launches take them, and the switches derived from them (step_form has the reasons)
    int physics, exact, ntu;
    bool trfold, fcopy, fuse, sml, smls, keep, hf2, finish_fused;
    int tme, hf, ddx, fluxf, aco;
    bool defer4, d4_pending, mru, msml, md_fold;
    bool early_state_dead, early_diag_dead, solve0_dead, norz;
    bool stepkeep, vik, a0k, dk, tuk, kept, keep2;
};

StepForm step_form(const mpas_ctx* c, double dt, int schedule, int gen) {
    const DevState& S = c->S;
    StepForm f{dt, schedule, gen};
    f.physics = S.physics, f.exact = c->exact, f.ntu = c->ntu;
    // rk_timestep.rg:378-399
    const int number_of_sub_steps = 2;
    f.dynamics_split = 1;  // constants.rg:62
    const double dt_dynamics = dt;
    f.rk_sub_timestep[0] = dt_dynamics / 3;
    f.rk_sub_timestep[1] = f.rk_sub_timestep[2] = dt_dynamics / number_of_sub_steps;
    f.number_sub_steps[0] = (number_of_sub_steps / 2 > 1) ? number_of_sub_steps / 2 : 1;
    f.number_sub_steps[1] = f.number_sub_steps[0];
    f.number_sub_steps[2] = number_of_sub_steps;
    for (int s = 0; s < 3; s++) {
        f.n_small[s] = f.number_sub_steps[s] + (S.physics ? 0 : 1);  // Q5 (the MPAS form: n)
        f.n_acoustic += f.n_small[s];
        f.rk_of[s] = schedule == 0 ? (int)f.rk_sub_timestep[s] : s;  // Q4: the reference driver passes the stage's time step
    }
    // option trsave: scalars_save's copy folded into the transport's bounds kernel (its tables decided here:
    // the tiled and LDS-edge forms need none of them built, su stored)
    // (transport = 2: the separate copy -- its first stage reads scalars and scalars_old)
    f.trfold = c->transport == 1 && c->trsave && !c->halo && !c->trtile && !c->tredge && !S.trsu;
    // option fusecopy: ru_save / u_2 by stage 0's dyn_tend edge kernel (reads u and ru there;
    // no task between the setup and that kernel reads ru_save or u_2, in any physics mode)
    f.fcopy = c->fusesetup && c->fusecopy;
    // option fusedamp (reference semantics): each damping but the step's last is applied by
    // the next acoustic launch (k_acoustic MODE 2), the last from the div the acoustic step
    // stored (launch_div_damping_div); the same bits as the separate task.  Decomposed (option
    // fusedamp_halo): the div is exchanged where rtheta_pp was, the ring-1 edges stay fresh
    f.fuse = c->fusedamp && S.physics == 0 && (!c->halo || (c->fusedamp_halo && S.ring1 && S.nERing >= S.nEO));
    // option fusesml (with fusedamp): the stage's first acoustic launch runs set_smlstep first
    f.sml = f.fuse && c->fusesml;
    // option tmedge (reference semantics, undecomposed): dyn_tend's edge kernel stores
    // theta_m(cell2) + theta_m(cell1) per edge, which the stage's acoustic substeps and the
    // damping read instead of gathering theta_m at both cells (theta_m unchanged in between)
    f.tme = (c->tmedge && S.physics == 0 && !c->halo) ? 1 : 0;
    // option hfuse (reference semantics, undecomposed): neighbouring kernels that neither
    // read what the other writes share a launch (k_solve.hip combined launches, dyn_tend's
    // rk 0 D beside E); the same values.  2: where the grids do not fill the chip
    f.hf = (S.physics == 0 && !c->halo && (c->hfuse == 1 || (c->hfuse == 2 && S.nCO < hfuse_auto_cells))) ? 1 : 0;
    // hfuse with fusedamp (and the default epw, no tmedge): a stage's last acoustic launch
    // beside its solve_diagnostics vertex / cell kernel, and the stage's edge kernel beside
    // the next stage's dyn_tend A (k_acoustic.hip / k_dyn.hip combined launches)
    f.hf2 = f.hf && f.fuse && !f.tme && S.epw == 2;
    // ... and the last stage's solve_diagnostics edge kernel beside atm_rk_dynamics_substep_finish
    f.finish_fused = f.hf && f.fuse && S.LP == 64 && !c->transport;
    // option smlsum (fast path, with fusesml): the slope-flux sum of set_smlstep formed once per
    // step (X_smlS); each stage's fused set_smlstep then reads one column instead of u_tend at
    // the cell's edges and zb_cell / zb3_cell (none of them written within the step)
    f.smls = f.fuse && c->fusesml && c->smlsum && !c->exact && S.physics == 0;
    // option smlkeep: the step takes X_smlS as it stands -- an undecomposed context whose step uses the sum;
    // srk3_run formed it ahead of the step where its inputs may have changed since it last did (sml_ensure) --
    // no flux launch in the step, so none in a captured one.  Decomposed contexts form it in every step:
    // skipping the kernel there would skip its exchange of u_tend too
    f.keep = f.smls && c->smlkeep && !c->halo;
    // option dd0 (reference semantics): every acoustic launch takes rw_save - rw as 0.0 (ddx 2); without it
    // the launches of a step with smlsum read the difference from X_Dd (ddx 1), the others both columns
    f.ddx = (c->dd0 && S.physics == 0) ? 2 : f.smls ? 1 : 0;
    f.fluxf = f.ddx == 2 ? 2 : 1;  // (the flux body beside the setup: with X_Dd or without)
    // option accoef (reference semantics, where nothing writes theta_m within the step): every acoustic
    // launch forms cofwr / coftz / a_tri itself, with the dts of the setup or vert_imp launch that formed
    // the live coefficient set (StepRun::dts_vi, recorded at each of those launches -- not the acoustic launch's own)
    // (not with option tmedge, off by default: its launches keep loading the stored set -- the exact first
    // launch of that form would lose a wave of occupancy to the three expressions, profiles/r08)
    f.aco = (c->accoef && S.physics == 0 && !f.tme) ? 1 : 0;
    // option defer4: an rk_step 0 stage followed by an rk_step > 0 one leaves its kernel D
    // (tend_u_euler's del4 part; its tend_u is dead: the next stage rewrites it and no task
    // in between reads it in the reference semantics) to the next stage's edge kernel
    f.defer4 = c->defer4 && S.physics == 0;
    // (with option ntu the deferred del4 waits for the last stage's edge kernel, stage_args)
    f.d4_pending = (f.rk_of[0] == 0 && f.rk_of[1] != 0) || (f.rk_of[1] == 0 && f.rk_of[2] != 0);
    // option mru (the MPAS dynamics, fast path): the kernel that forms the stage's final tend_u also
    // stores the first acoustic substep's ru_p = dts tend_u and ruAvg = ru_p (nothing in between reads
    // or writes them; set_smlstep reads tend_u only)
    f.mru = c->mru && S.physics == 2 && !c->exact;
    // option msml (the MPAS dynamics): the stage's set_smlstep (:1503-1528) applied by E to the tend_w it
    // forms -- set_smlstep follows dyn_tend directly and reads tend_u, which B / D have finished
    f.msml = c->msml && S.physics == 2;
    // option mdamp (the MPAS forms): the previous substep's damping in this substep's ru_p kernel, the
    // stage's last one in the recover edge kernel -- each read-modify-write of ru_p goes
    f.md_fold = c->mdamp && S.physics;
    // option ntu, the dead acoustic state of the stages before the last (ntu 1 and 2): the next stage's first
    // substep sets rho_pp, rtheta_pp, rw_p, wwAvg (and ruAvg) before any task reads them; stage 0's vert_imp
    // leaves b_tri / c_tri to stage 1's.  Their dead diagnostics (ntu 1 and 3): stage_diagnostics.  (ntu = 2:
    // every diagnostic stored, 3: every acoustic state stored -- the A/Bs of these parts)
    f.early_state_dead = c->ntu == 1 || c->ntu == 2;
    f.early_diag_dead = c->ntu == 1 || c->ntu == 3;
    // option ntu: stage 0's solve_diagnostics is dead where stage 1 runs at rk_step > 0 (a stage before the last
    // reads nothing it writes; an rk_step 0 stage 1 would read divergence and vorticity)
    f.solve0_dead = c->ntu && S.physics == 0 && !f.hf && f.rk_of[1] != 0;
    // option ntu (reference semantics): the substep finish's rho_zz = rho_zz_old_split is the identity --
    // this step's setup made rho_zz_old_split from rho_zz and nothing writes either in between -- not made
    f.norz = f.early_state_dead && S.physics == 0 && S.LP == 64 && f.dynamics_split == 1;
    // option stepkeep: the step whose launches the kept generation may thin out -- the headline's order
    // (DESIGN.md §4k lists why each condition is there); anywhere else keep_gen stays 0
    f.stepkeep = c->stepkeep && f.keep && c->ntu == 1 && c->defer4 && f.fcopy && c->accoef && !f.hf && !c->tmedge &&
                 !c->etile && !c->transport && !c->forcing && !c->microphysics && !c->pbl && f.rk_of[0] == 0 && f.rk_of[1] != 0 && f.rk_of[2] != 0;
    // option vikeep: stage 0's coefficient set in scratch (every generation of a step stepkeep is active for)
    f.vik = c->vikeep && f.stepkeep;
    // option a0keep: a full step leaves the next step's kdiff in X_kd0; a kept step takes it from there and runs
    // neither stage 0's A nor the finish's edge part (stepkeep's step is the one whose stage 0 takes the
    // form with setup's copies in A: fusecopy, ntu, defer4, horiz_mixing 0, undecomposed, no etile)
    f.a0k = c->a0keep && f.stepkeep;
    // option dynkeep: a kept step launches the guarded instances of stage 0's B, C and E and of stage 1's and 2's
    // E, which decide on X_dkf; a full step clears the flag (in its setup task), a kept one sets it after stage
    // 2's E (in that dyn_tend task): no timing key of its own.  (stepkeep = 2 skips those launches on the host)
    f.dk = c->dynkeep && f.a0k && c->stepkeep == 1;
    // option tukeep: the kept steps' stage-0 and stage-2 edge kernels in their TK instances, k_dyn_B_top behind the
    // latter -- the decision is X_dkf's too (no flag, capture, timing key or scratch column of its own)
    // Not while per-task timing is on: a timed step is the one whose dyn_tend rows are set against the reference
    // task's B_alg (bench.py's roofline record), so its launches do that task's work -- dynkeep's instances, which
    // leave every field and X_tue0 as the TK ones expect to find them (either form may follow the other)
    f.tuk = c->tukeep && f.dk && !c->timing;
    f.kept = gen >= 1;
    // option stepkeep = 2, generation 2: everything stage 0's dyn_tend stores is in place from the
    // generation-1 step (whose stage 0 read the diagnostics the step itself formed, as this one would)
    // -- kdiff, tend_rho, dpdz, ru_save, u_2, the delsq fields, tend_u_euler, tend_w_euler, tend_theta_euler
    // -- but w, which the acoustic launches and the later stages have rewritten since: restored below
    // level L from that step's copy.  Stage 2 then forms tend_u, v and w alone: h_divergence (A) and the
    // theta tendencies (B's flux, E) are final too, and tend_u_euler already holds its del4 part
    f.keep2 = gen == 2 && c->stepkeep == 2;
    return f;
}

// option smlkeep: X_smlS formed here when its inputs may have changed since the kernel last ran
// (mpas_ctx::sml_valid): on the task stream ahead of the step and outside any capture, under the flux task's
// timing key.  With dd0 the kernel reads nothing a step writes; without it X_Dd comes from rw alone (the setup
// that follows stores rw_save = rw, and no task of the step writes rw), so ahead of the setup is the same computation
void sml_ensure(mpas_ctx* c, const StepForm& f) {
    if (!f.keep || c->sml_valid) return;
    run_task(c, "atm_set_smlstep_pert_variables_work[flux]", [&] { return launch_sml_flux(c->S, c->stream, c->dd0 ? 2 : 1); });
    c->sml_valid = true;
}

DynTendArgs stage_args(const StepForm& f, int r) {
    DynTendArgs a{};
    a.rk_step = f.rk_of[r];
    a.dt = f.dt;
    a.horiz_mixing = 0, a.cam_coef = 0.0, a.mix_full = 0, a.rayleigh_damp_u = 0;  // constants.rg:57 "2d_smagorinsky"
    a.exact_q = f.exact;
    a.tme = f.tme;
    a.hfuse = f.hf;
    a.cp = (f.fcopy && r == 0) ? 1 : 0;
    if (f.defer4) {
        a.defer_out = (r < 2 && f.rk_of[r] == 0 && f.rk_of[r + 1] != 0) ? 1 : 0;
        a.defer_in = (r > 0 && f.rk_of[r - 1] == 0 && f.rk_of[r] != 0) ? 1 : 0;
        // (option ntu: the stages before the last read no tend_u_euler -- their edge kernels form no
        // tend_u -- so the deferred del4 goes to the last stage's edge kernel, the first that reads it;
        // its operands, delsq_divergence / delsq_vorticity / rho_edge, are unchanged until then)
        if (f.ntu) a.defer_in = (r == 2 && f.d4_pending) ? 1 : 0;
    }
    // option ntu (reference semantics): a stage before the step's last leaves dead tendencies -- the last
    // stage rewrites tend_u, tend_theta, tend_rtheta_adv and rthdynten, and no task in between reads them
    // (set_smlstep reads u_tend, Q2; the acoustic step reads neither tend_u, Q18, nor tend_theta: theta_m
    // is its tend_rt, Q8): that dyn_tend forms none of them (tend_u only where its D, reading it, does not run)
    if (f.ntu && f.physics == 0 && r < 2) {
        a.nth = 1;
        a.ntu = 1;  // (launch_dyn_tend keeps it off where D runs in the call)
    }
    if (f.mru && f.number_sub_steps[r] > 0) a.rud = f.rk_sub_timestep[r];
    if (f.msml) a.smlE = 1;
    return a;
}

struct StepRun {
    FuseBuffers fb;
    bool pending = false;     // a damping waits for the next acoustic launch (option fusedamp), with coef_prev
    double coef_prev = 0.0;
    int done_acoustic = 0;
    double dts_vi = 0.0;      // the dts of the launch that formed the live vert_imp coefficient set (option accoef)
    bool vi_done = false;     // stage 1's vert_imp ran beside stage 0's solve_diagnostics edges (option hfuse)
    bool vc_done = false;     // the stage's solve_diagnostics vertex / cell kernel ran beside its last acoustic launch
    bool a_done = false;      // the stage's dyn_tend A ran in the launch before it
    bool vdyn_on = false;     // stage 2's dyn_tend stores v (decided there: S.eoe_same is k_prepare's, which the
                              // step's first task may still have to run)
    bool flux_done = false;   // (option smlsum: the step's flux sum, beside setup and A on small grids)
    explicit StepRun(mpas_ctx* c) : fb(c) {}
};

// :400-424 -- the copy the transport starts from, the forcing, setup / moist / stage 0's vert_imp, the flux sum
void step_begin(mpas_ctx* c, const StepForm& f, StepRun& r) {
    const DevState& S = c->S;
    hipStream_t st = c->stream;
    const double dts0 = f.rk_sub_timestep[0];
    if (c->transport && !f.trfold) {
        // the time level the transport starts from (MPAS-A scalars(time level 1)); the
        // copy carries the ghosts of scalars, fresh or not, so scalars_old is as stale
        run_task(c, "scalars_save", [&] {
            hipError_t e = hipMemcpyAsync(S.f[F_scalars_old], S.f[F_scalars], dev_bytes(c, F_scalars),
                                          hipMemcpyDeviceToDevice, st);
            if (S.halo && S.halo->stale[F_scalars]) S.halo->wrote({F_scalars_old});
            return e;
        });
    }
    // option forcing: the physics tendencies of the step, from the state the step starts from; every stage's
    // dyn_tend (the MPAS forms) reads them, no task of the step writes them
    if (c->forcing) run_task(c, "atm_held_suarez_forcing", [&] { return launch_held_suarez_forcing(S, st); });
    if (c->fusesetup && S.physics == 0 && f.hf2) {  // + stage 0's dyn_tend A in the same launch
        const bool fl = f.smls && !f.keep;
        run_task(c, fl ? "hfuse[setup+dyn_A+sml_flux]" : "hfuse[setup+dyn_A]", [&] {
            return launch_hf_setup_dyn_A(S, st, stage_args(f, 0), dts0, f.fcopy ? 0 : 1, fl ? f.fluxf : 0);
        });
        r.a_done = true;
        r.flux_done = fl;
    } else if (c->fusesetup) {  // :404-417 as one column-local launch (same values; MPAS forms under physics)
        // (option ntu: stage 0's vert_imp leaves b_tri / c_tri unstored -- no task reads them and stage 1's
        // vert_imp, which always runs, rewrites both; "-bc")
        const bool nbc = f.early_state_dead;
        const char* key = f.fcopy ? "atm_rk_integration_setup[cells+moist+vert_imp]" : "atm_rk_integration_setup[+moist+vert_imp]";
        run_task(c, tagged(key, nbc ? "-bc" : "").c_str(), [&] {
            if (f.dk && f.gen == 0) {  // (the columns of option dynkeep are stale from here on)
                const hipError_t e = launch_dk_flag(S, st, 0);
                if (e != hipSuccess) return e;
            }
            return launch_setup_moist_vert_imp(S, st, dts0, !f.fcopy, nbc ? 1 : 0, f.aco, f.kept ? 1 : 0, f.vik ? 1 : 0,
                                               f.a0k && f.kept ? 1 : 0);
        });
    } else {
        run_task(c, "atm_rk_integration_setup", [&] { return launch_rk_integration_setup(S, st); });
        run_task(c, "atm_compute_moist_coefficients", [&] { return launch_moist_coefficients(S, st); });
        run_task(c, "atm_compute_vert_imp_coefs", [&] { return launch_vert_imp_coefs(S, st, dts0); });
    }
    r.dts_vi = dts0;
    if (f.smls && !f.keep && !r.flux_done)
        run_task(c, "atm_set_smlstep_pert_variables_work[flux]", [&] { return launch_sml_flux(S, st, f.ddx == 2 ? 2 : 0); });
}

// stage 1's vert_imp, where no combined launch has run it
void stage_vert_imp(mpas_ctx* c, const StepForm& f, StepRun& r, int s) {
    if (s != 1 || r.vi_done) return;
    // (option vikeep, a kept step: a_tri, b_tri, c_tri and the four cof columns hold this call's values)
    run_task(c, "atm_compute_vert_imp_coefs", [&] {
        return f.vik && f.kept ? launch_vert_imp_kept(c->S, c->stream, f.rk_sub_timestep[s])
                               : launch_vert_imp_coefs(c->S, c->stream, f.rk_sub_timestep[s]);
    });
    r.dts_vi = f.rk_sub_timestep[s];
}

// :427-428 -- the stage's dyn_tend and, without fusesml / msml, its set_smlstep; returns the call's arguments
DynTendArgs stage_dyn_tend(mpas_ctx* c, const StepForm& f, StepRun& r, int s) {
    const DevState& S = c->S;
    hipStream_t st = c->stream;
    DynTendArgs a = stage_args(f, s);
    a.skipA = r.a_done ? 1 : 0;
    // option vdyn (reference semantics): the last stage's v (:429-437) is reconstructed by its
    // dyn_tend edge kernel from the edgesOnEdge u it gathers for q -- u is not written between
    // that kernel and the stage's solve_diagnostics, which then skips v
    if (s == 2) r.vdyn_on = c->vdyn && S.physics == 0 && a.rk_step > 0 && S.eoe_same;
    a.store_v = (s == 2 && r.vdyn_on) ? 1 : 0;
    r.a_done = false;
    if (f.keep2 && s == 2) {  // (StepForm::keep2: tend_u, v and w alone)
        a.skipA = 1;
        a.defer_in = 0;
        a.nth = 1;
    }
    // option stepkeep, any kept step: stage 2's A (rk_step > 0: h_divergence alone, from ru and the mesh --
    // no task of the step writes ru) stored the same bits in the full step; B reads them
    if (f.kept && s == 2) a.skipA = 1;
    // option a0keep, any kept step: stage 0's A stored the same bits in the step before -- tend_rho, dpdz,
    // X_wc, ru_save, u_2 -- and the setup launch has put the step's kdiff in place; B as if A had run
    if (f.a0k && f.kept && s == 0) a.keptA = 1;
    // option dynkeep, any kept step: the guarded instances -- the first kept step after a full one runs them as
    // the plain ones and fills X_tue0 / X_w0..2, the later ones copy those back (the same launches: one graph)
    const bool dkept = f.dk && f.kept;
    if (dkept) a.dynkeep = s + 1;
    // option tukeep: stage 0's guarded edge kernel leaves tend_u_euler alone in a fresh pass, stage 2's forms
    // nothing there and k_dyn_B_top tend_u's level L - 1 (stage 1 launches no edge kernel in a kept step)
    if (dkept && f.tuk && s != 1) a.tukeep = 1;
    if (f.keep2 && s == 0) {  // (w below level L from the generation-1 step's copy; nothing else to form)
        run_task(c, "stepkeep_restore_w", [&] { return launch_cell_col_copy(S, st, X_w0, F_w); });
    } else {
        run_task(c, dyn_tend_key(a).c_str(), [&] {
            const hipError_t e = launch_dyn_tend(S, st, a);
            // (option dynkeep: the step's last guarded launch is behind -- the columns hold this step's values)
            return (dkept && s == 2 && e == hipSuccess) ? launch_dk_flag(S, st, 1) : e;
        });
        if (f.gen == 1 && c->stepkeep == 2 && s == 0)  // (the copy a generation-2 step restores)
            run_task(c, "stepkeep_save_w", [&] { return launch_cell_col_copy(S, st, F_w, X_w0); });
    }
    if (!f.sml && !a.smlE)  // (option fusesml: run by the stage's first acoustic launch; option msml: by E)
        run_task(c, "atm_set_smlstep_pert_variables_work", [&] { return launch_set_smlstep(S, st, c->exact); });
    return a;
}

// :440-452 with option fusedamp: substep ss of stage s, the damping before it inside the launch
void stage_acoustic_fused(mpas_ctx* c, const StepForm& f, StepRun& r, int s, int ss) {
    const DevState& S = c->S;
    hipStream_t st = c->stream;
    const double dts = f.rk_sub_timestep[s];
    const bool last_of_stage = ss == f.n_small[s] - 1;
    const int mode = r.pending ? 2 : 1;
    const int sm = (f.sml && ss == 0) ? (f.smls ? 2 : 1) : 0;
    // rtheta_pp_old is read by the separate damping only: the fused one reads the
    // stored div, so the step's last substep alone leaves it (option fusedamp)
    // option ntu (bit 1): a stage's last substep before the step's last stage leaves rho_pp,
    // rtheta_pp, rw_p and wwAvg unstored -- the next stage's first substep sets them before
    // any task reads them (:1615-1636), and the damping reads the stored div
    const int nst = f.early_state_dead && s < 2 && last_of_stage ? 2 : 0;
    const int wold = ((r.done_acoustic + 1 == f.n_acoustic) ? 1 : 0) | nst;
    if (f.hf2 && s < 2 && mode == 2 && ss > 0 && last_of_stage) {
        run_task(c, nst ? "hfuse[acoustic-st+solve_vc]" : "hfuse[acoustic+solve_vc]", [&] {
            return launch_hf_acoustic_solve_vc(S, st, dts, ss, c->exact, r.coef_prev, wold, f.ddx, f.aco, r.dts_vi);
        });
        r.vc_done = true;
    } else {
        // ("-st": option ntu's launch that stores no acoustic state, bench.py's accounting)
        run_task(c, tagged(acoustic_name(ss, r.pending, sm, !(wold & 1)), nst ? "-st" : "").c_str(), [&] {
            // option vikeep: stage 0's launches load cofwt / cofwz from the scratch pair -- a copy of
            // the state whose two field slots point there (the kernels are the same)
            DevState A = S;
            if (f.vik && s == 0) A.f[F_cofwt] = S.f[X_cofwt0], A.f[F_cofwz] = S.f[X_cofwz0];
            return launch_acoustic(A, st, dts, ss, c->exact, mode, r.coef_prev, f.tme, sm, wold, f.ddx, 0, 0, f.aco,
                                   r.dts_vi);
        });
    }
    if (mode == 2) r.fb.swap_rup();
    r.fb.swap_dv();  // this substep's div is read next from X_dvB
    if (++r.done_acoustic == f.n_acoustic) {
        if (f.hf)  // beside the solve_diagnostics vertex / cell kernel that follows
            run_task(c, "hfuse[damp+solve_vc]", [&] { return launch_hf_damp_solve_vc(S, st, dts, f.tme); });
        else
            run_task(c, "atm_divergence_damping_3d", [&] { return launch_div_damping_div(S, st, dts, f.tme); });
        r.pending = false;
    } else {
        r.pending = true;
        r.coef_prev = divdamp_coef(dts);
    }
}

// :440-452 without it: the substep, then its damping (option mdamp: folded into the launch that next reads ru_p)
void stage_acoustic_split(mpas_ctx* c, const StepForm& f, StepRun& r, int s, int ss, bool ru_done) {
    const DevState& S = c->S;
    hipStream_t st = c->stream;
    const double dts = f.rk_sub_timestep[s];
    const int mdp = (f.md_fold && ss > 0) ? (ss == 1 ? 2 : 1) : 0;
    const double cprev = mdp ? divdamp_coef(dts) : 0.0;
    // (option ntu: the last substep of a stage before the last leaves wwAvg unstored -- its recover
    // does not read it (the averages are dead there) and the next stage's first substep sets it)
    const bool nww = S.physics && f.early_state_dead && s < 2 && ss == f.n_small[s] - 1;
    // ("-ru": option mru, this first substep's ru_p / ruAvg were stored by the stage's dyn_tend)
    const bool nru = ss == 0 && ru_done;
    const std::string an = tagged(tagged(acoustic_name(ss, mdp != 0), nww ? "-ww" : ""), nru ? "-ru" : "");
    run_task(c, an.c_str(), [&] {
        return launch_acoustic(S, st, dts, ss, c->exact, 0, cprev, f.tme, 0, nww ? 3 : 1, f.ddx, mdp, nru ? 1 : 0, f.aco,
                               r.dts_vi);
    });
    if (!f.md_fold)
        run_task(c, "atm_divergence_damping_3d", [&] { return launch_div_damping(S, st, dts, ss == 0); });
}

// rk_timestep.rg:460, commented out in the reference (Q7): the MPAS forms only
void stage_recover(mpas_ctx* c, const StepForm& f, int s) {
    if (!c->S.physics) return;
    // option ntu: a stage before the last leaves ruAvg / wwAvg dead -- the next stage's first
    // acoustic substep sets both before any task reads them
    const bool navg = f.early_state_dead && s < 2;
    // (option mdamp: the stage's last damping in the edge kernel; 2: that substep was the stage's first)
    const int ns_r = f.number_sub_steps[s];
    const int dmp = (c->mdamp && ns_r > 0) ? (ns_r == 1 ? 2 : 1) : 0;
    const std::string rn = navg ? (s == 1 ? "atm_recover_large_step_variables_work[rk1-avg]"
                                          : "atm_recover_large_step_variables_work[rk<2-avg]")
                                : recover_name(s);
    run_task(c, tagged(rn, dmp ? "+damp" : "").c_str(), [&] {
        return launch_recover_large_step(c->S, c->stream, ns_r, s, f.dt, navg ? 1 : 0, dmp, f.rk_sub_timestep[s]);
    });
}

// :462-476 -- the stage's solve_diagnostics, in the form the launches around it leave to it
void stage_diagnostics(mpas_ctx* c, const StepForm& f, StepRun& r, int s) {
    const DevState& S = c->S;
    hipStream_t st = c->stream;
    if (f.kept) {
        // option stepkeep: no solve_diagnostics launch -- its outputs are functions of u and h alone, which
        // no task of the step writes: they hold what the last stage of the step before stored (stage 1's
        // [live] outputs are bits of that full kernel's, option ntu's own identity; v as stage 2's B or
        // that kernel stored it)
    } else if (s == 2 && f.finish_fused) {
        // (the vertex / cell kernel ran beside the last damping) the edge kernel beside
        // atm_rk_dynamics_substep_finish, which step_end then does not launch
        run_task(c, tagged(r.vdyn_on ? "hfuse[solve_e-v+finish]" : "hfuse[solve_e+finish]", f.norz ? "-rz" : "").c_str(),
                 [&] { return launch_hf_solve_e_finish(S, st, r.vdyn_on ? 0 : 1, f.norz ? 1 : 0); });
    } else if (f.hf && f.fuse && s == 2) {
        run_task(c, r.vdyn_on ? "atm_compute_solve_diagnostics[e-v]" : "atm_compute_solve_diagnostics[e]",
                 [&] { return launch_solve_diagnostics(S, st, 0, 2, 2, r.vdyn_on ? 1 : 0); });
    } else if (f.hf2 && r.vc_done && s < 2) {
        // (the vertex / cell kernel ran beside the last acoustic launch) the edge kernel
        // beside the next stage's dyn_tend A, and after stage 0 beside stage 1's vert_imp
        const DynTendArgs nx = stage_args(f, s + 1);
        run_task(c, s == 0 ? "hfuse[solve_e+vert_imp+dyn_A]" : "hfuse[solve_e+dyn_A]", [&] {
            return launch_hf_solve_e_dyn_A(S, st, nx, s == 0 ? 1 : 0, f.rk_sub_timestep[1]);
        });
        if (s == 0) r.vi_done = true, r.dts_vi = f.rk_sub_timestep[1];
        r.a_done = true;
        r.vc_done = false;
    } else if (s == 0 && f.solve0_dead) {
        // option ntu: stage 0's solve_diagnostics is dead -- stage 1's dyn_tend (a stage before the last:
        // no A, no tend_u) reads none of its outputs, no other task reads them, and stage 1's and 2's
        // solve_diagnostics rewrite every one (h_edge, ke_edge, pv_edge, divergence, ke, vorticity, pv_vertex)
    } else if (f.hf && s == 0) {  // the edge kernel beside stage 1's vert_imp
        run_task(c, "atm_compute_solve_diagnostics[vc]", [&] { return launch_solve_diagnostics(S, st, 0, 0, 1); });
        run_task(c, "hfuse[solve_e+vert_imp]", [&] { return launch_hf_solve_e_vert_imp(S, st, f.rk_sub_timestep[1]); });
        r.vi_done = true;
        r.dts_vi = f.rk_sub_timestep[1];
    } else {
        const int nv = (s == 2 && r.vdyn_on) ? 1 : 0;
        // option ntu: a call before the last stage's, the next stage at rk_step > 0, stores only what
        // that stage reads -- ke and pv_edge (the MPAS forms: rho_edge too); its divergence, vorticity,
        // h_edge and ke_edge have no reader before the last stage's solve_diagnostics rewrites them
        // (dyn_tend reads divergence and vorticity at rk_step 0 only; nothing reads h_edge, ke_edge)
        const bool live = f.early_diag_dead && s < 2 && f.rk_of[s + 1] != 0;
        run_task(c, live ? "atm_compute_solve_diagnostics[live]"
                         : nv ? "atm_compute_solve_diagnostics[-v]" : "atm_compute_solve_diagnostics",
                 [&] { return launch_solve_diagnostics(S, st, 0, s, live ? 7 : 3, nv); });
    }
}

// :478-492 -- a0keep's kdiff for the next step, the transport, the reconstruction, the substep finish
void step_end(mpas_ctx* c, const StepForm& f, StepRun& r) {
    const DevState& S = c->S;
    hipStream_t st = c->stream;
    const double dt = f.dt;
    // option a0keep, a full step that leaves generation 1: the kdiff stage 0's A of the next step would store --
    // from u and the v stage 2 has just left (its B, or solve_diagnostics) -- into X_kd0; the field keeps this
    // step's.  Kernel A itself, on a state whose kdiff slot points at the scratch column; its other stores write
    // the bytes they hold.  (Not a dyn_tend row: the step's three stay three)
    if (f.a0k && f.gen == 0)
        run_task(c, "a0keep_kdiff", [&] { return launch_dyn_A_kdiff(S, st, stage_args(f, 0), X_kd0); });
    if (c->transport == 2) {
        // MPAS's RK3 transport (dynamics and transport split): every stage from scalars_old with the
        // step's ruAvg / wwAvg / rho_zz_old_split, its high-order fluxes from the stage before
        run_task(c, "atm_advance_scalars", [&] { return launch_advance_scalars(S, st, dt / 3); });
        run_task(c, "atm_advance_scalars", [&] { return launch_advance_scalars(S, st, dt / 2); });
        run_task(c, "atm_advance_scalars_mono_rk", [&] {
            trt_ensure(c);
            return launch_advance_scalars_mono_rk(S, st, dt);
        });
    } else if (c->transport)  // after the last stage's recover: ruAvg / wwAvg / rho_zz of the step
        run_task(c, f.trfold ? "atm_advance_scalars_mono[save]" : "atm_advance_scalars_mono", [&] {
            trt_ensure(c);  // (built before a capture by prepare_mesh)
            return launch_advance_scalars_mono(S, st, dt, f.trfold ? 1 : 0);
        });
    if (S.physics == 2)  // the MPAS dynamics: cell-centre winds for the next step's curvature
        run_task(c, "mpas_reconstruct_2d", [&] { return launch_reconstruct_2d(S, st, 1); });  // (:487, commented)
    // (option a0keep, a kept step: no physics 0 task writes ruAvg, so the edge part's ruAvg_split = ruAvg stored
    // the same bytes in the step before -- the cell part alone)
    if (!f.finish_fused)  // (else it ran beside solve_diagnostics' edges)
        run_task(c, f.norz ? "atm_rk_dynamics_substep_finish[-rz]" : "atm_rk_dynamics_substep_finish", [&] {
            return launch_substep_finish(S, st, 1, f.dynamics_split, f.norz ? 1 : 0, f.a0k && f.kept ? 1 : 0);
        });
    r.fb.finish();
    // option microphysics: the step ends with the Kessler task on the state the step leaves -- behind the transport
    // and the reconstruction; its rt_diabatic_tend is the heating of the next step's dynamics
    if (c->microphysics)
        run_task(c, "atm_kessler_microphysics", [&] { return launch_kessler(S, st, dt, c->precip); });
    // option pbl: then the surface fluxes and the boundary layer (the DCMIP order: microphysics, then simple
    // physics); the tend_ru_physics it leaves is the one the next step's three stages read
    if (c->pbl)
        run_task(c, "atm_surface_pbl", [&] { return launch_surface_pbl(S, st, dt, c->sst, c->sflux); });
    // :492 summarize_timestep(cr, er, false, false, false) (constants.rg:67-69): prints only
}

void srk3(mpas_ctx* c, const StepForm& f) {
    StepRun r(c);
    step_begin(c, f, r);
    for (int s = 0; s < 3; s++) {  // :426-477
        stage_vert_imp(c, f, r, s);
        const DynTendArgs a = stage_dyn_tend(c, f, r, s);
        for (int ss = 0; ss < f.n_small[s]; ss++)
            if (f.fuse) stage_acoustic_fused(c, f, r, s, ss);
            else stage_acoustic_split(c, f, r, s, ss, a.rud != 0.0);
        stage_recover(c, f, s);
        stage_diagnostics(c, f, r, s);
    }
    step_end(c, f, r);
}

void graph_free(mpas_ctx::GraphEntry& g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g.exec = nullptr;
    g.graph = nullptr;
}
void graph_drop(mpas_ctx* c) {
    for (auto& g : c->graphs) graph_free(g);
    c->graphs.clear();
    c->seen_stale0.clear();
}

void prepare_now(mpas_ctx* c) {
    prepare_mesh(c);
    if (c->transport) trt_ensure(c);
    ett_ensure(c);
}

// one atm_srk3 step of form f: replayed from a captured HIP graph when possible
void srk3_run(mpas_ctx* c, const StepForm& f) {
    const double dt = f.dt;
    const int schedule = f.schedule, gen = f.gen;
    Halo* h = c->halo.get();
    const bool halo_graph = h && !h->loop && (h->stub ? c->graph_halo != 0 : (h->rccl && c->graph_halo == 1)) &&
                            !c->graph_refused;
    sml_ensure(c, f);
    if (!c->graph_on || c->timing || (h && !halo_graph)) {
        srk3(c, f);
        return;
    }
    prepare_now(c);  // (synchronous: never inside a capture)
    static const std::vector<uint8_t> none;
    const std::vector<uint8_t>& start = h ? h->stale : none;
    for (auto& g : c->graphs)
        if (g.dt == dt && g.schedule == schedule && g.gen == gen && g.stale0 == start) {
            hipcheck(hipGraphLaunch(g.exec, c->stream), "hipGraphLaunch");
            g.used = ++c->graph_clock;
            c->graph_launches++;
            if (h) {
                h->stale = g.stale1;  // the bookkeeping the captured step made
                h->exchanges += g.exch;
                h->fields_moved += g.fields;
            }
            return;
        }
    if (h && std::find(c->seen_stale0.begin(), c->seen_stale0.end(), h->stale) == c->seen_stale0.end()) {
        // a start state not seen before (e.g. the first step after an upload): one eager step
        if (c->seen_stale0.size() >= 16) c->seen_stale0.erase(c->seen_stale0.begin());
        c->seen_stale0.push_back(h->stale);
        srk3(c, f);
        return;
    }
    mpas_ctx::GraphEntry g;
    g.dt = dt;
    g.schedule = schedule;
    g.gen = gen;
    g.stale0 = start;
    int64_t ex0 = 0, fl0 = 0;
    if (h) {
        ex0 = h->exchanges;
        fl0 = h->fields_moved;
        h->capture_miss = false;
    }
    // a decomposed step whose capture failed: nothing ran, so the halo bookkeeping goes back to the step's start
    // and the step runs eagerly.  refused: the transport refused the capture (a communicator that cannot be
    // captured) -- eager steps from now on (a real error repeats in the eager step)
    auto eager_instead = [&](bool refused) {
        h->stale = g.stale0;
        h->exchanges = ex0;
        h->fields_moved = fl0;
        h->overlapped.clear();  // (the aborted step's overlap record and race flag too)
        h->race.clear();
        h->err.clear();
        if (refused) (void)hipGetLastError(), c->graph_refused = true, c->graph_fallbacks++;
        srk3(c, f);
    };
    hipcheck(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
    try {
        srk3(c, f);
    } catch (...) {
        hipGraph_t gr = nullptr;
        (void)hipStreamEndCapture(c->stream, &gr);
        if (gr) (void)hipGraphDestroy(gr);
        if (!h) throw;
        // (capture_miss: a pack table not built yet, never built inside a capture -- the eager step builds it,
        // the next step captures)
        const bool miss = h->capture_miss;
        h->capture_miss = false;
        eager_instead(!miss);
        return;
    }
    {
        const hipError_t ee = hipStreamEndCapture(c->stream, &g.graph);
        hipError_t ei = ee;
        if (ee == hipSuccess) ei = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        if (h && (ee != hipSuccess || ei != hipSuccess)) {
            graph_free(g);
            eager_instead(true);
            return;
        }
        hipcheck(ee, "hipStreamEndCapture");
        hipcheck(ei, "hipGraphInstantiate");
    }
    c->graph_captures++;
    if (h) {
        g.stale1 = h->stale;
        g.exch = h->exchanges - ex0;
        g.fields = h->fields_moved - fl0;
    }
    g.used = ++c->graph_clock;
    if (c->graphs.size() >= mpas_ctx::kGraphCache) {  // the least recently replayed goes
        auto lru = std::min_element(c->graphs.begin(), c->graphs.end(),
                                    [](const mpas_ctx::GraphEntry& a, const mpas_ctx::GraphEntry& b) { return a.used < b.used; });
        graph_free(*lru);
        c->graphs.erase(lru);
    }
    c->graphs.push_back(g);
    hipcheck(hipGraphLaunch(g.exec, c->stream), "hipGraphLaunch");
    c->graph_launches++;
}

// one sample of the sigma-level statistics (k_stats.hip): the task, under a timing key of its own
void stats_accumulate(mpas_ctx* c) {
    if (!c->stats_ns) throw Fail{MPAS_EINVAL, "atm_sigma_stats_accumulate: no sigma levels configured (mpas_sigma_stats_configure)"};
    if (c->S.physics != 2) throw Fail{MPAS_EINVAL, "atm_sigma_stats_accumulate needs physics = 2 (it samples the MPAS dynamics' state)"};
    run_task(c, "atm_sigma_stats_accumulate",
             [&] { return launch_sigma_stats(c->S, c->stream, c->stats_acc, c->stats_sig, c->stats_ns); });
    c->stats_samples++;
}
void stats_zero(mpas_ctx* c) {
    if (c->stats_acc)
        hipcheck(hipMemsetAsync(c->stats_acc, 0, (size_t)c->S.nCells * stats_rec(c->stats_ns) * sizeof(double), c->stream),
                 "hipMemsetAsync");
    c->stats_samples = 0;
}
void stats_free(mpas_ctx* c) {
    if (c->stats_acc) (void)hipFree(c->stats_acc);
    if (c->stats_sig) (void)hipFree(c->stats_sig);
    c->stats_acc = c->stats_sig = nullptr;
    c->stats_ns = 0;
    c->stats_every = 0;
    c->stats_samples = 0;
}

// the Kessler task's accumulators (mpas_ctx::precip), allocated and zeroed on first use
void precip_ensure(mpas_ctx* c) {
    if (c->precip) return;
    const size_t bytes = 3 * (size_t)c->S.nCells * sizeof(double);
    if (hipMalloc((void**)&c->precip, bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->precip = nullptr;
        throw Fail{MPAS_ENOMEM, "hipMalloc precipitation accumulators"};
    }
    hipcheck(hipMemsetAsync(c->precip, 0, bytes, c->stream), "hipMemsetAsync");
    hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
}

// the surface task's accumulators (mpas_ctx::sflux), allocated and zeroed on first use
void sflux_ensure(mpas_ctx* c) {
    if (c->sflux) return;
    const size_t bytes = 3 * (size_t)c->S.nCells * sizeof(double);
    if (hipMalloc((void**)&c->sflux, bytes) != hipSuccess) {
        (void)hipGetLastError();
        c->sflux = nullptr;
        throw Fail{MPAS_ENOMEM, "hipMalloc surface-flux accumulators"};
    }
    hipcheck(hipMemsetAsync(c->sflux, 0, bytes, c->stream), "hipMemsetAsync");
    hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
}

// one atm_srk3 step, with option stepkeep's bookkeeping: the generation the step runs at, then the one it leaves
void srk3_step(mpas_ctx* c, double dt, int schedule) {
    const bool act = step_form(c, dt, schedule, 0).stepkeep;
    if (!act || c->keep_dt != dt || c->keep_schedule != schedule) c->keep_gen = 0;
    // (the launches of generations 1 and 2 differ with stepkeep = 2 only: one captured graph for both otherwise)
    const int gen = (c->keep_gen == 2 && c->stepkeep != 2) ? 1 : c->keep_gen, next = c->keep_gen < 2 ? c->keep_gen + 1 : 2;
    c->keep_gen = 0;  // (a step that fails promises nothing)
    srk3_run(c, step_form(c, dt, schedule, gen));
    if (act) {
        c->keep_gen = next;
        c->keep_dt = dt;
        c->keep_schedule = schedule;
    }
    // option stats_every: the sample behind the step (after its mpas_reconstruct_2d; the substep finish in between
    // writes nothing the task reads), on the stream and outside the captured graph
    if (c->stats_every > 0 && ++c->stats_step % c->stats_every == 0) stats_accumulate(c);
}

// ---- options: one row per name; mpas_set_option and mpas_get_option walk the table ---------------------
// How mpas_set_option treats a value (then the row's hook runs, then the value is stored):
enum OptTreat {
    O_BOOL,   // any value: stored as value ? 1 : 0
    O_CLAMP,  // stored clamped to [lo, hi]
    O_RANGE,  // refused with the row's text outside [lo, hi]
    O_LIST,   // refused with the row's text unless one of the listed values
    O_ANY,    // stored as given (xcd: speed only, and no caller passes what it has not measured)
    O_QUERY,  // read-only: mpas_set_option does not know the name
};
using OptHook = void (*)(mpas_ctx*, int64_t&);  // preconditions (throws) and side effects of a set
using OptGet = int64_t (*)(mpas_ctx*);
struct OptRow {
    const char* name;
    OptTreat treat;
    int mpas_ctx::*cm;  // where the value lives: a member of mpas_ctx ...
    int DevState::*sm;  // ... or of DevState; neither: the hook stores it, and without get the name is set-only
    int64_t lo, hi;     // (O_LIST: the listed values are list[0 .. lo))
    const char* err;
    OptHook hook;
    OptGet get;  // the read-only queries, and values that live elsewhere
    int64_t list[4];
};
OptRow opt(const char* name, int mpas_ctx::*m, OptTreat t, int64_t lo = 0, int64_t hi = 0, const char* err = nullptr,
           OptHook hook = nullptr, OptGet get = nullptr) {
    return {name, t, m, nullptr, lo, hi, err, hook, get, {}};
}
OptRow opt(const char* name, int DevState::*m, OptTreat t, int64_t lo = 0, int64_t hi = 0, const char* err = nullptr,
           OptHook hook = nullptr, std::initializer_list<int64_t> list = {}) {
    OptRow o{name, t, nullptr, m, lo, hi, err, hook, nullptr, {}};
    std::copy(list.begin(), list.end(), o.list);
    return o;
}
constexpr int mpas_ctx::*kNoMember = nullptr;
OptRow query(const char* name, OptGet get) { return opt(name, kNoMember, O_QUERY, 0, 0, nullptr, nullptr, get); }

void dirty_tiles(mpas_ctx* c, int64_t&) { c->trt_dirty = c->ett_dirty = true; }
void dirty_ett(mpas_ctx* c, int64_t&) { c->ett_dirty = true; }
const char* const kStubLatencyErr = "stub_latency_us: a stub-transport context and 0..100000 us";

const OptRow kOptions[] = {
    opt("exact", &mpas_ctx::exact, O_BOOL),
    opt("graph", &mpas_ctx::graph_on, O_BOOL),
    opt("fusedamp", &mpas_ctx::fusedamp, O_BOOL),
    opt("fusesetup", &mpas_ctx::fusesetup, O_BOOL),
    opt("fusecopy", &mpas_ctx::fusecopy, O_BOOL),
    opt("defer4", &mpas_ctx::defer4, O_BOOL),
    opt("ntu", &mpas_ctx::ntu, O_CLAMP, 0, 3),
    opt("mdamp", &mpas_ctx::mdamp, O_BOOL),
    opt("accoef", &mpas_ctx::accoef, O_RANGE, 0, 1, "accoef must be 0 or 1"),
    opt("dd0", &mpas_ctx::dd0, O_RANGE, 0, 1, "dd0 must be 0 or 1"),
    opt("smlkeep", &mpas_ctx::smlkeep, O_RANGE, 0, 1, "smlkeep must be 0 or 1"),
    opt("stepkeep", &mpas_ctx::stepkeep, O_RANGE, 0, 2, "stepkeep must be 0, 1 or 2"),
    opt("vikeep", &mpas_ctx::vikeep, O_RANGE, 0, 1, "vikeep must be 0 or 1"),
    opt("a0keep", &mpas_ctx::a0keep, O_RANGE, 0, 1, "a0keep must be 0 or 1"),
    opt("dynkeep", &mpas_ctx::dynkeep, O_RANGE, 0, 1, "dynkeep must be 0 or 1"),
    opt("tukeep", &mpas_ctx::tukeep, O_RANGE, 0, 1, "tukeep must be 0 or 1"),
    opt("mru", &mpas_ctx::mru, O_BOOL),
    opt("msml", &mpas_ctx::msml, O_BOOL),
    opt("vdyn", &mpas_ctx::vdyn, O_BOOL),
    opt("tmedge", &mpas_ctx::tmedge, O_BOOL),
    opt("fusesml", &mpas_ctx::fusesml, O_BOOL),
    opt("smlsum", &mpas_ctx::smlsum, O_BOOL),
    opt("fusedamp_halo", &mpas_ctx::fusedamp_halo, O_BOOL),
    opt("hfuse", &mpas_ctx::hfuse, O_CLAMP, 0, 2),
    // (every value but 1 and 2 is 0: below by the clamp, above by the hook)
    opt("graph_halo", &mpas_ctx::graph_halo, O_CLAMP, 0, 3, nullptr,
        [](mpas_ctx* c, int64_t& v) {
            if (v == 3) v = 0;
            c->graph_refused = false;
        }),
    opt("stub_refuse_capture", kNoMember, O_BOOL, 0, 0, nullptr,
               [](mpas_ctx* c, int64_t& v) {
                   if (!c->halo || !c->halo->stub) throw Fail{MPAS_EINVAL, "stub_refuse_capture: a stub-transport context"};
                   c->halo->stub_refuse_capture = (int)v;
               }),
    opt("stub_latency_us", kNoMember, O_RANGE, 0, 100000, kStubLatencyErr,
               [](mpas_ctx* c, int64_t& v) {
                   if (!c->halo || !c->halo->stub) throw Fail{MPAS_EINVAL, kStubLatencyErr};
                   c->halo->stub_latency_us = (int)v;
               },
               [](mpas_ctx* c) -> int64_t { return c->halo ? c->halo->stub_latency_us : 0; }),
    opt("xcd", &DevState::xcd, O_ANY),
    opt("keep_check", &mpas_ctx::keep_check, O_BOOL),
    opt("epw", &DevState::epw, O_LIST, 3, 0, "epw must be 1, 2 or 4", nullptr, {1, 2, 4}),
    opt("vcmix", &DevState::vcmix, O_BOOL),
    opt("physics", &DevState::physics, O_RANGE, 0, 2, "physics must be 0 (reference), 1 (MPAS vertical solver) or 2 (MPAS dynamics)",
        [](mpas_ctx* c, int64_t& v) {
            if (!v) c->transport = 0;
            if (v != 2) c->forcing = 0, c->stats_every = 0, c->microphysics = 0, c->pbl = 0;
            c->ett_dirty = true;
        }),
    opt("trorder_e", &DevState::troe, O_RANGE, 0, 1 << 20, "trorder_e must be 0 (trorder's), 1 or a run length >= 2"),
    opt("cve", &DevState::cve, O_LIST, 4, 0, "cve must be 0, 1, 4 or 8", nullptr, {0, 1, 4, 8}),
    opt("bsplit", &DevState::bsplit, O_RANGE, 0, 2, "bsplit must be 0, 1 or 2"),
    opt("trepw", &DevState::trepw, O_RANGE, 1, 2, "trepw must be 1 or 2"),
    opt("trsu", &DevState::trsu, O_BOOL),
    opt("trorder", &DevState::tro, O_RANGE, 0, 1 << 20, "trorder must be 0, 1 or a run length >= 2"),
    opt("ring1", &DevState::ring1, O_BOOL),
    opt("trtile", &mpas_ctx::trtile, O_BOOL, 0, 0, nullptr, dirty_tiles),
    opt("trsave", &mpas_ctx::trsave, O_BOOL),
    opt("tredge", &mpas_ctx::tredge, O_BOOL, 0, 0, nullptr, dirty_tiles),
    opt("trtile_ghosts", &mpas_ctx::trt_ghosts, O_BOOL, 0, 0, nullptr, dirty_tiles),
    opt("trtcells", &mpas_ctx::trt_cells, O_RANGE, 1, 256, "trtcells must be 1..256", dirty_tiles),
    opt("trtclo", &mpas_ctx::trt_clo, O_RANGE, 1 + NF * (2 + AF), 120, "trtclo must be 67..120 (LDS columns)", dirty_tiles),
    opt("etile", &mpas_ctx::etile, O_BOOL, 0, 0, nullptr, dirty_ett),
    opt("etmode", &DevState::etm, O_RANGE, 0, 2, "etmode must be 0, 1 or 2"),
    opt("etthreads", &DevState::etnt, O_LIST, 2, 0, "etthreads must be 256 or 512", nullptr, {256, 512}),
    opt("etcells", &mpas_ctx::ett_cells, O_RANGE, 1, 40, "etcells must be 1..40 (a tile's edges index in one byte)", dirty_ett),
    opt("etclo", &mpas_ctx::ett_clo, O_RANGE, 20, 160, "etclo must be 20..160 (LDS columns)", dirty_ett),
    opt("transport", &mpas_ctx::transport, O_RANGE, 0, 2, "transport must be 0, 1 (one monotonic update) or 2 (RK3)",
        [](mpas_ctx* c, int64_t& v) {
            if (v && !c->S.physics)
                throw Fail{MPAS_EINVAL, "transport needs physics = 1 (it reads the recovered ruAvg, wwAvg, rho_zz)"};
        }),
    opt("forcing", &mpas_ctx::forcing, O_RANGE, 0, 1, "forcing must be 0 or 1 (Held-Suarez)",
        [](mpas_ctx* c, int64_t& v) {
            if (v && c->S.physics != 2)
                throw Fail{MPAS_EINVAL, "forcing needs physics = 2 (the MPAS forms of dyn_tend consume its tendencies)"};
            if (v && c->pbl)
                throw Fail{MPAS_EINVAL, "forcing and pbl both write tend_ru_physics: Rayleigh friction or the boundary layer"};
        }),
    opt("microphysics", &mpas_ctx::microphysics, O_RANGE, 0, 1, "microphysics must be 0 or 1 (Kessler warm rain)",
        [](mpas_ctx* c, int64_t& v) {
            if (v && c->S.physics != 2)
                throw Fail{MPAS_EINVAL, "microphysics needs physics = 2 (the MPAS forms consume rt_diabatic_tend)"};
            if (v) {
                hipcheck(hipSetDevice(c->device), "hipSetDevice");
                precip_ensure(c);
            }
        }),
    opt("pbl", &mpas_ctx::pbl, O_RANGE, 0, 1, "pbl must be 0 or 1 (simple-physics surface fluxes and boundary layer)",
        [](mpas_ctx* c, int64_t& v) {
            if (v && (c->S.physics != 2 || !c->sst))
                throw Fail{MPAS_EINVAL, "pbl needs physics = 2 and a surface temperature (mpas_surface_set_temperature)"};
            if (v && c->forcing)
                throw Fail{MPAS_EINVAL, "pbl and forcing both write tend_ru_physics: the boundary layer or Rayleigh friction"};
            if (v) {
                hipcheck(hipSetDevice(c->device), "hipSetDevice");
                sflux_ensure(c);
            }
        }),
    opt("stats_every", &mpas_ctx::stats_every, O_RANGE, 0, 0x7fffffff, "stats_every must be >= 0 (steps per sample; 0: none)",
        [](mpas_ctx* c, int64_t& v) {
            if (v && (c->S.physics != 2 || !c->stats_ns))
                throw Fail{MPAS_EINVAL, "stats_every needs physics = 2 and configured sigma levels (mpas_sigma_stats_configure)"};
            c->stats_step = 0;
        }),
    opt("overlap", &mpas_ctx::overlap, O_BOOL, 0, 0, nullptr,
        [](mpas_ctx* c, int64_t& v) {
            if (c->halo) c->halo->overlap = (int)v;
        }),
    opt("self", &mpas_ctx::self_on, O_BOOL, 0, 0, nullptr, [](mpas_ctx* c, int64_t& v) { c->S.selfc = c->self_ok && v; }),
    opt("bounds_probe", kNoMember, O_ANY, 0, 0, nullptr,  // bounds-checked build only
               [](mpas_ctx* c, int64_t& v) {
#if MPAS_BOUNDS
                   hipcheck(hipSetDevice(c->device), "hipSetDevice");
                   hipcheck(launch_bounds_probe(c->S, c->stream, (int)v), "bounds_probe");
#else
                   throw Fail{MPAS_ENOTSUP, "bounds_probe needs the bounds-checked build (libmpasdyn_bounds.so)"};
#endif
               }),
    // the read-only queries
    query("tredge_active", [](mpas_ctx* c) -> int64_t { return trt_ensure(c), c->S.tre != nullptr; }),  // edge groups built for this mesh
    query("tredge_irregular", [](mpas_ctx* c) -> int64_t { return trt_ensure(c), c->tre.nirr; }),
    query("trtile_active", [](mpas_ctx* c) -> int64_t { return trt_ensure(c), c->S.trt ? 1 : 0; }),  // tiles built for this mesh
    query("trtile_count", [](mpas_ctx* c) -> int64_t { return trt_ensure(c), c->trt.ntiles; }),
    query("etile_active", [](mpas_ctx* c) -> int64_t { return ett_ensure(c), c->S.ett ? 1 : 0; }),  // dyn_tend tiles built for this mesh
    query("etile_count", [](mpas_ctx* c) -> int64_t { return ett_ensure(c), c->ett.ntiles; }),
    query("etile_columns", [](mpas_ctx* c) -> int64_t { return ett_ensure(c), c->ett.nclo; }),  // closure columns staged per launch
    query("etile_maxclo", [](mpas_ctx* c) -> int64_t { return ett_ensure(c), c->ett.maxclo; }),
    query("stats_samples", [](mpas_ctx* c) -> int64_t { return c->stats_samples; }),
    query("stepkeep_gen", [](mpas_ctx* c) -> int64_t { return c->keep_gen; }),
    query("dynkeep_fresh", [](mpas_ctx* c) -> int64_t {  // the device flag X_dkf
        int fresh = 0;
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        hipcheck(hipMemcpyAsync(&fresh, c->S.f[X_dkf], sizeof(fresh), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        return fresh;
    }),
    query("tukeep_active", [](mpas_ctx* c) -> int64_t { return step_form(c, 0.0, 1, 0).tuk; }),  // (its kept steps' form)
    query("eoe_same", [](mpas_ctx* c) -> int64_t { return prepare_now(c), c->S.eoe_same; }),
    // (the switches of the step's form that do not depend on dt, schedule or generation)
    query("hfuse_active", [](mpas_ctx* c) -> int64_t { return step_form(c, 0.0, 1, 0).hf; }),
    query("fusedamp_active", [](mpas_ctx* c) -> int64_t { return step_form(c, 0.0, 1, 0).fuse; }),
    query("graph_fallbacks", [](mpas_ctx* c) -> int64_t { return c->graph_fallbacks; }),
    query("graph_refused", [](mpas_ctx* c) -> int64_t { return c->graph_refused ? 1 : 0; }),
    query("graph_captures", [](mpas_ctx* c) -> int64_t { return c->graph_captures; }),
    query("graph_launches", [](mpas_ctx* c) -> int64_t { return c->graph_launches; }),
    query("halo_state", [](mpas_ctx* c) -> int64_t {  // hash of the halo bookkeeping (debug)
        uint64_t hsh = 1469598103934665603ull;
        if (c->halo)
            for (uint8_t v : c->halo->stale) hsh = (hsh ^ v) * 1099511628211ull;
        return (int64_t)(hsh >> 1);
    }),
    query("orphan_edges", [](mpas_ctx* c) -> int64_t { return prepare_now(c), c->S.n_orph; }),  // edges no cell lists (k_prepare)
    query("bounds", [](mpas_ctx*) -> int64_t { return MPAS_BOUNDS; }),  // the bounds-checked build
#if MPAS_BOUNDS
    query("bounds_units", [](mpas_ctx*) -> int64_t {  // kernel units checking / registered
        return ((int64_t)bounds_units() << 32) | (int64_t)bounds_tus().size();
    }),
#endif
    query("selfc", [](mpas_ctx* c) -> int64_t {  // decided now (needs the mesh uploaded)
        if (c->dirty) hipcheck(hipSetDevice(c->device), "hipSetDevice");
        return prepare_mesh(c), c->S.selfc;
    }),
};
const OptRow* find_option(const char* name) {
    if (name)
        for (const OptRow& o : kOptions)
            if (std::strcmp(o.name, name) == 0) return &o;
    return nullptr;
}
Fail unknown_option(const char* name) { return Fail{MPAS_EINVAL, std::string("unknown option ") + (name ? name : "(null)")}; }

}  // namespace

extern "C" {

int mpas_field_count(void) { return F_COUNT; }
int mpas_field_id(const char* name) {
    if (!name) return MPAS_EINVAL;
    for (int f = 0; f < F_COUNT; f++)
        if (std::strcmp(kFields[f].name, name) == 0) return f;
    return MPAS_EINVAL;
}
const char* mpas_field_name(int f) { return (f >= 0 && f < F_COUNT) ? kFields[f].name : nullptr; }
int mpas_field_kind(int f) { return (f >= 0 && f < F_COUNT) ? kFields[f].kind : MPAS_EINVAL; }
int mpas_field_width(int f) { return (f >= 0 && f < F_COUNT) ? kFields[f].width : MPAS_EINVAL; }

static thread_local std::string g_create_err;

int mpas_ctx_create(mpas_ctx** out, int device, const mpas_dims* dims) {
    if (!out || !dims) return MPAS_EINVAL;
    *out = nullptr;
    if (dims->nCells <= 0 || dims->nEdges <= 0 || dims->nVertices <= 0 || dims->nVertLevels < 1 ||
        dims->nVertLevels + 1 > 64) {
        g_create_err = "mpas_ctx_create: need nCells, nEdges, nVertices > 0 and 1 <= nVertLevels <= 63 "
                       "(one wavefront holds a column of nVertLevels + 1 levels)";
        return MPAS_EINVAL;
    }
    mpas_ctx* c = new (std::nothrow) mpas_ctx();
    if (!c) return MPAS_ENOMEM;
    int rc = guarded(c, [&] {
        int n = 0;
        hipcheck(hipGetDeviceCount(&n), "hipGetDeviceCount");
        if (device < 0 || device >= n) throw Fail{MPAS_EINVAL, "no such HIP device"};
        hipcheck(hipSetDevice(device), "hipSetDevice");
        hipDeviceProp_t prop;
        hipcheck(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            throw Fail{MPAS_ENOTSUP, std::string("libmpasdyn is built for gfx950, device is ") + prop.gcnArchName};
        c->device = device;
        c->dims = *dims;
        int LP = 8;
        while (LP < dims->nVertLevels + 1) LP <<= 1;
        c->S.nCells = dims->nCells;
        c->S.nEdges = dims->nEdges;
        c->S.nVertices = dims->nVertices;
        c->S.nCO = dims->nCells;  // all owned until mpas_halo_owned says otherwise
        c->S.nEO = dims->nEdges;
        c->S.nVO = dims->nVertices;
        c->S.L = dims->nVertLevels;
        c->S.LP = LP;
        c->S.epw = 2;  // tools/kbench.py: div_damp -3 %, solve_diagnostics -4 % vs 1
        c->S.vcmix = 1;
        c->S.physics = 0;
        c->S.ring1 = 1;
        c->S.xcd = 64;  // runs of 64 blocks per XCD (tools/kbench.py: -2.5 % step time vs dispatcher order)
        c->S.trepw = 1;
        c->S.tro = 64;  // transport: pair-major within runs of 64 entities (profiles/r03/transport_v5: -1 to -3 %)
        c->S.bsplit = 2;  // dyn_tend's flux kernel split off under the MPAS dynamics (profiles/r05/bsplit)
        c->S.etm = 1;  // (the tiled E's best form: profiles/r06/etile)
        c->S.etnt = 256;
        hipcheck(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate");
        // Field f starts (f % 16) * stagger bytes into its allocation (env MPAS_ALLOC_STAGGER,
        // a multiple of 512: whole columns stay aligned; default 2048): equal-sized arrays
        // read together then do not start on the same HBM channel.  Measured at x1.163842 x 56
        // (interleaved A/B on one box): dyn_tend rk>0 -4 %, rk0 -2 %, step -1.5 % against 0
        size_t stagger = 2048;
        if (const char* v = std::getenv("MPAS_ALLOC_STAGGER")) stagger = (size_t)std::strtoull(v, nullptr, 10) / 512 * 512;
        for (int f = 0; f < X_COUNT; f++) {
            const size_t b = dev_bytes(c, f), off = (size_t)(f % 16) * stagger;
            void* p = nullptr;
            hipError_t e = hipMalloc(&p, b + off);
            if (e != hipSuccess) throw Fail{MPAS_ENOMEM, std::string("hipMalloc ") + kFields[f].name};
            hipcheck(hipMemset(p, 0, b + off), "hipMemset");
            c->raw[f] = p;
            c->S.f[f] = (char*)p + off;
        }
        hipcheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
        bounds_add(c);
    });
    if (rc != MPAS_OK) {
        g_create_err = c->err;
        fprintf(stderr, "mpas_ctx_create: %s\n", c->err.c_str());
        mpas_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return MPAS_OK;
}

int mpas_ctx_destroy(mpas_ctx* c) {
    if (!c) return MPAS_EINVAL;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->raw[0]) bounds_remove(c);
    for (int f = 0; f < X_COUNT; f++)
        if (c->raw[f]) (void)hipFree(c->raw[f]);
    for (auto& t : c->pending) {
        (void)hipEventDestroy(t.e0);
        (void)hipEventDestroy(t.e1);
    }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    graph_drop(c);
    trt_free(c);
    ett_free(c);
    c->halo.reset();
    c->loopgrp.reset();
    for (auto p : c->gid_dev)
        if (p) (void)hipFree(p);
    if (c->sum_scratch) (void)hipFree(c->sum_scratch);
    if (c->keep_flag) (void)hipFree(c->keep_flag);
    stats_free(c);
    if (c->precip) (void)hipFree(c->precip);
    if (c->sst) (void)hipFree(c->sst);
    if (c->sflux) (void)hipFree(c->sflux);
    if (c->sum_out) (void)hipFree(c->sum_out);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return MPAS_OK;
}

const char* mpas_last_error(const mpas_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int mpas_sync(mpas_ctx* c) {
    return guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    }, true);
}

int mpas_get_stream(mpas_ctx* c, void** stream) {
    if (!c || !stream) return MPAS_EINVAL;
    *stream = (void*)c->stream;
    return MPAS_OK;
}

int mpas_set_option(mpas_ctx* c, const char* name, int64_t value) {
    return guarded(c, [&] {
        graph_drop(c);  // every option is baked into a captured step
        const OptRow* o = find_option(name);
        if (!o || o->treat == O_QUERY) throw unknown_option(name);
        int64_t v = value;
        const bool listed = o->treat == O_LIST && std::find(o->list, o->list + o->lo, v) != o->list + o->lo;
        switch (o->treat) {
            case O_BOOL: v = v ? 1 : 0; break;
            case O_CLAMP: v = v < o->lo ? o->lo : v > o->hi ? o->hi : v; break;
            case O_RANGE: if (v < o->lo || v > o->hi) throw Fail{MPAS_EINVAL, o->err}; break;
            case O_LIST: if (!listed) throw Fail{MPAS_EINVAL, o->err}; break;
            default: break;
        }
        if (o->hook) o->hook(c, v);
        if (o->cm) c->*(o->cm) = (int)v;
        if (o->sm) c->S.*(o->sm) = (int)v;
    });
}

int mpas_get_option(mpas_ctx* c, const char* name, int64_t* value) {
    return guarded(c, [&] {
        if (!value) throw Fail{MPAS_EINVAL, "mpas_get_option: null value"};
        const OptRow* o = find_option(name);
        if (o && o->get) *value = o->get(c);
        else if (o && o->cm) *value = c->*(o->cm);
        else if (o && o->sm) *value = c->S.*(o->sm);
        else throw unknown_option(name);  // (the set-only names too)
    }, true);
}

int mpas_upload(mpas_ctx* c, int f, const void* host, int64_t se, int64_t sl, int64_t sc) {
    return guarded(c, [&] {
        if (f < 0 || f >= F_COUNT || !host) throw Fail{MPAS_EINVAL, "mpas_upload: bad field or pointer"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        const FieldInfo& fi = kFields[f];
        const int n = entity_count(c, fi.kind), L = c->S.L, LP = c->S.LP, W = fi.width;
        const char* h = (const char*)host;
        std::vector<char> staged;  // a device view of a 2-D field / ZV: staged through the host
        if (is_device_ptr(host)) {
            if (is_3d(fi.kind)) {  // device to device, no host round trip
                hipcheck(launch_view_copy(c->S.f[f], (void*)host, fi.kind == K_C3B ? 1 : 8, n, W, L, LP, se, sl, sc, 1,
                                          c->stream),
                         "upload view");
                if (fi.kind != K_C3V && fi.kind != K_C3B && W == 1)
                    hipcheck(launch_keep_refresh(c->S, c->stream, f, keep_kind(f)), "keep_refresh");
                hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
                c->dirty = true;
                c->trt_dirty = c->ett_dirty = true;
                graph_drop(c);
                if (c->halo) c->halo->stale[f] = 0;
                return;
            }
            const size_t span = fi.kind == K_ZV ? (size_t)(L * sl + 8)
                                                : view_span(n, W, 0, se, 0, sc, elem_size(fi.kind));
            staged.resize(span);
            hipcheck(hipMemcpy(staged.data(), host, span, hipMemcpyDeviceToHost), "hipMemcpy D2H (view)");
            h = staged.data();
        }
        size_t bytes = dev_bytes(c, f);
        std::vector<char> buf(bytes, 0);
        if (fi.kind == K_C3 || fi.kind == K_E3 || fi.kind == K_V3) {
            double* d = (double*)buf.data();
            for (int e = 0; e < n; e++)
                for (int k = 0; k <= L; k++) d[(size_t)e * LP + lpos(LP, k)] = *(const double*)(h + e * se + k * sl);
            if (W == 1) {  // the keep tails: level L and level 0 of every column (the zero slot's: 0)
                const size_t rows = (size_t)n + 1;
                for (int e = 0; e < n; e++) {
                    d[rows * LP + e] = d[(size_t)e * LP + lpos(LP, L)];
                    d[rows * LP + rows + e] = d[(size_t)e * LP + lpos(LP, 0)];
                }
            }
        } else if (fi.kind == K_C3V) {
            double* d = (double*)buf.data();
            for (int e = 0; e < n; e++)
                for (int i = 0; i < W; i++)
                    for (int k = 0; k <= L; k++)
                        d[vidx(W, LP, e, i, k)] = *(const double*)(h + e * se + k * sl + i * sc);
        } else if (fi.kind == K_C3B) {
            uint8_t* d = (uint8_t*)buf.data();
            for (int e = 0; e < n; e++)
                for (int k = 0; k <= L; k++) d[(size_t)e * LP + lpos(LP, k)] = *(const uint8_t*)(h + e * se + k * sl);
        } else if (fi.kind == K_ZV) {
            double* d = (double*)buf.data();
            for (int k = 0; k <= L; k++) d[k] = *(const double*)(h + k * sl);
        } else if (elem_size(fi.kind) == 4) {
            int32_t* d = (int32_t*)buf.data();
            int tgt = id_target(f);
            int lim = tgt < 0 ? 0 : entity_count(c, tgt);
            // list lengths: the kernels index rows of this width with them (tail loops past
            // the unrolled entries), so a longer list would read past the row -- refused
            const int width = count_width(f);
            for (int e = 0; e < n; e++)
                for (int i = 0; i < W; i++) {
                    int32_t v = *(const int32_t*)(h + e * se + i * sc);
                    if (tgt >= 0 && (v < 0 || v > lim)) v = lim;  // Q1 zero slot
                    if (width > 0 && v > width)
                        throw Fail{MPAS_EINVAL, std::string("mpas_upload: ") + fi.name + " " + std::to_string(v) +
                                                    " at entity " + std::to_string(e) + " exceeds its list width " +
                                                    std::to_string(width)};
                    d[(size_t)e * W + i] = v;
                }
        } else {
            double* d = (double*)buf.data();
            for (int e = 0; e < n; e++)
                for (int i = 0; i < W; i++) d[(size_t)e * W + i] = *(const double*)(h + e * se + i * sc);
        }
        hipcheck(hipMemcpy(c->S.f[f], buf.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
        c->dirty = true;
        c->trt_dirty = c->ett_dirty = true;
        graph_drop(c);
        if (c->halo) c->halo->stale[f] = 0;  // uploaded ghosts are the global values
        // derived mesh arrays: cos()/sin() on the host with the same libm as the oracle
        struct { int src, dst; double (*fn)(double); } der[] = {
            {F_angleEdge, X_cosAngleEdge, ::cos}, {F_angleEdge, X_sinAngleEdge, ::sin},
            {F_latEdge, X_cosLatEdge, ::cos},     {F_lat, X_cosLatCell, ::cos},
            {F_lat, X_sinLatCell, ::sin},         {F_lon, X_cosLonCell, ::cos},      {F_lon, X_sinLonCell, ::sin}};
        for (const auto& dv : der) {
            if (dv.src != f) continue;
            std::vector<double> cs((size_t)n + 1, 0.0);
            const double* d = (const double*)buf.data();
            for (int e = 0; e < n; e++) cs[e] = dv.fn(d[e]);
            cs[n] = dv.fn(0.0);  // zero slot: as the oracle computes it from its zero row
            hipcheck(hipMemcpy(c->S.f[dv.dst], cs.data(), cs.size() * 8, hipMemcpyHostToDevice), "hipMemcpy H2D");
        }
    });
}

int mpas_download(mpas_ctx* c, int f, void* host, int64_t se, int64_t sl, int64_t sc) {
    return guarded(c, [&] {
        if (f < 0 || f >= F_COUNT || !host) throw Fail{MPAS_EINVAL, "mpas_download: bad field or pointer"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        const FieldInfo& fi = kFields[f];
        const int n = entity_count(c, fi.kind), L = c->S.L, LP = c->S.LP, W = fi.width;
        void* dview = nullptr;  // a device view of a 2-D field / ZV: staged through the host
        std::vector<char> staged;
        if (is_device_ptr(host)) {
            if (is_3d(fi.kind)) {
                hipcheck(launch_view_copy(c->S.f[f], host, fi.kind == K_C3B ? 1 : 8, n, W, L, LP, se, sl, sc, 0,
                                          c->stream),
                         "download view");
                hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
                return;
            }
            const size_t span = fi.kind == K_ZV ? (size_t)(L * sl + 8)
                                                : view_span(n, W, 0, se, 0, sc, elem_size(fi.kind));
            staged.resize(span);
            hipcheck(hipMemcpy(staged.data(), host, span, hipMemcpyDeviceToHost), "hipMemcpy D2H (view)");
            dview = host;
            host = staged.data();
        }
        size_t bytes = dev_bytes(c, f);
        std::vector<char> buf(bytes);
        hipcheck(hipMemcpy(buf.data(), c->S.f[f], bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        char* h = (char*)host;
        if (fi.kind == K_C3 || fi.kind == K_E3 || fi.kind == K_V3) {
            const double* d = (const double*)buf.data();
            for (int e = 0; e < n; e++)
                for (int k = 0; k <= L; k++) *(double*)(h + e * se + k * sl) = d[(size_t)e * LP + lpos(LP, k)];
        } else if (fi.kind == K_C3V) {
            const double* d = (const double*)buf.data();
            for (int e = 0; e < n; e++)
                for (int i = 0; i < W; i++)
                    for (int k = 0; k <= L; k++)
                        *(double*)(h + e * se + k * sl + i * sc) = d[vidx(W, LP, e, i, k)];
        } else if (fi.kind == K_C3B) {
            const uint8_t* d = (const uint8_t*)buf.data();
            for (int e = 0; e < n; e++)
                for (int k = 0; k <= L; k++) *(uint8_t*)(h + e * se + k * sl) = d[(size_t)e * LP + lpos(LP, k)];
        } else if (fi.kind == K_ZV) {
            const double* d = (const double*)buf.data();
            for (int k = 0; k <= L; k++) *(double*)(h + k * sl) = d[k];
        } else if (elem_size(fi.kind) == 4) {
            const int32_t* d = (const int32_t*)buf.data();
            for (int e = 0; e < n; e++)
                for (int i = 0; i < W; i++) *(int32_t*)(h + e * se + i * sc) = d[(size_t)e * W + i];
        } else {
            const double* d = (const double*)buf.data();
            for (int e = 0; e < n; e++)
                for (int i = 0; i < W; i++) *(double*)(h + e * se + i * sc) = d[(size_t)e * W + i];
        }
        if (dview)  // the staged image back into the device view (the bytes between its
                    // elements came from it, so they are unchanged)
            hipcheck(hipMemcpy(dview, staged.data(), staged.size(), hipMemcpyHostToDevice), "hipMemcpy H2D (view)");
    }, true);
}

int mpas_fill_synthetic(mpas_ctx* c, uint64_t seed) {
    return guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        hipcheck(launch_fill_synthetic(c->S, c->stream, seed), "fill_synthetic");
        keep_refresh_all(c);
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        if (c->halo)  // filled from global ids: ghosts hold the global values
            for (auto& v : c->halo->stale) v = 0;
    });
}

// ---- decomposition (mpasdyn/decomp.py builds the local state and the plan) ----------
namespace {
Halo* halo_of(mpas_ctx* c) {
    if (!c->halo) {
        c->halo.reset(new Halo());
        c->halo->stale.assign(X_COUNT, 0);
        c->S.halo = c->halo.get();
    }
    return c->halo.get();
}
int* dev_ints(const int32_t* h, int n) {
    int* d = nullptr;
    hipcheck(hipMalloc(&d, sizeof(int) * (size_t)(n > 0 ? n : 1)), "hipMalloc");
    if (n > 0) hipcheck(hipMemcpy(d, h, sizeof(int) * (size_t)n, hipMemcpyHostToDevice), "hipMemcpy H2D");
    return d;
}
}  // namespace

int mpas_halo_owned(mpas_ctx* c, int32_t nCellsOwned, int32_t nEdgesOwned, int32_t nVerticesOwned) {
    return guarded(c, [&] {
        graph_drop(c);
        if (nCellsOwned < 0 || nCellsOwned > c->S.nCells || nEdgesOwned < 0 || nEdgesOwned > c->S.nEdges ||
            nVerticesOwned < 0 || nVerticesOwned > c->S.nVertices)
            throw Fail{MPAS_EINVAL, "mpas_halo_owned: owned counts exceed the local counts"};
        c->S.nCO = nCellsOwned;
        c->S.nEO = nEdgesOwned;
        c->S.nVO = nVerticesOwned;
        c->dirty = true;
        c->trt_dirty = c->ett_dirty = true;
    });
}

int mpas_halo_ring1(mpas_ctx* c, int32_t nEdgesRing1, int32_t nVerticesRing1) {
    return guarded(c, [&] {
        graph_drop(c);
        if (nEdgesRing1 < c->S.nEO || nEdgesRing1 > c->S.nEdges || nVerticesRing1 < c->S.nVO ||
            nVerticesRing1 > c->S.nVertices)
            throw Fail{MPAS_EINVAL, "mpas_halo_ring1: needs owned <= count <= local, edges and vertices"};
        c->S.nERing = nEdgesRing1;
        c->S.nVRing = nVerticesRing1;
    });
}

int mpas_halo_interior(mpas_ctx* c, int32_t nCI, int32_t nEI, int32_t nVI) {
    return guarded(c, [&] {
        graph_drop(c);
        if (nCI < 0 || nCI > c->S.nCO || nEI < 0 || nEI > c->S.nEO || nVI < 0 || nVI > c->S.nVO)
            throw Fail{MPAS_EINVAL, "mpas_halo_interior: interior counts exceed the owned counts"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        Halo* h = halo_of(c);
        h->nint[0] = nCI;
        h->nint[1] = nEI;
        h->nint[2] = nVI;
        h->interior = true;
        h->overlap = c->overlap;
        c->trt_dirty = c->ett_dirty = true;
        if (!h->comm) {  // the halo stream, at the device's highest priority
            int least = 0, greatest = 0;
            hipcheck(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
            hipcheck(hipStreamCreateWithPriority(&h->comm, hipStreamNonBlocking, greatest), "hipStreamCreate");
            hipcheck(hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming), "hipEventCreate");
            hipcheck(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming), "hipEventCreate");
        }
    });
}

int mpas_halo_plan(mpas_ctx* c, int kind, int peer, const int32_t* send_ids, int32_t nsend, const int32_t* recv_ids,
                   int32_t nrecv) {
    return guarded(c, [&] {
        if (kind < 0 || kind > 2 || peer < 0 || nsend < 0 || nrecv < 0 || (nsend && !send_ids) || (nrecv && !recv_ids))
            throw Fail{MPAS_EINVAL, "mpas_halo_plan: bad arguments"};
        const int lim = kind == 0 ? c->S.nCells : kind == 1 ? c->S.nEdges : c->S.nVertices;
        const int own = kind == 0 ? c->S.nCO : kind == 1 ? c->S.nEO : c->S.nVO;
        for (int i = 0; i < nsend; i++)
            if (send_ids[i] < 0 || send_ids[i] >= own) throw Fail{MPAS_EINVAL, "mpas_halo_plan: send id not owned"};
        for (int i = 0; i < nrecv; i++)
            if (recv_ids[i] < own || recv_ids[i] >= lim) throw Fail{MPAS_EINVAL, "mpas_halo_plan: recv id not a ghost"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        Halo* h = halo_of(c);
        HaloPeer p;
        p.peer = peer;
        p.nsend = nsend;
        p.nrecv = nrecv;
        p.d_send = dev_ints(send_ids, nsend);
        p.d_recv = dev_ints(recv_ids, nrecv);
        h->peers[kind].push_back(p);
        h->clear_tabs();  // the pack / unpack tables follow the plan
        c->graph_refused = false;
        graph_drop(c);
    });
}

int mpas_set_global_ids(mpas_ctx* c, int kind, const int32_t* gids, int32_t n) {
    return guarded(c, [&] {
        const int lim = kind == 0 ? c->S.nCells : kind == 1 ? c->S.nEdges : c->S.nVertices;
        if (kind < 0 || kind > 2 || n != lim || !gids) throw Fail{MPAS_EINVAL, "mpas_set_global_ids: bad arguments"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        if (c->gid_dev[kind]) hipcheck(hipFree(c->gid_dev[kind]), "hipFree");
        c->gid_dev[kind] = dev_ints(gids, n);
        c->S.gid[kind] = c->gid_dev[kind];
    });
}

int mpas_halo_loopback(mpas_ctx** ctxs, int n) {
    if (!ctxs || n < 1) return MPAS_EINVAL;
    for (int i = 0; i < n; i++)
        if (!ctxs[i] || ctxs[i]->device != ctxs[0]->device) return MPAS_EINVAL;
    for (int i = 0; i < n; i++) ctxs[i]->sml_valid = false, ctxs[i]->keep_gen = 0;
    return guarded(ctxs[0], [&] {
        hipcheck(hipSetDevice(ctxs[0]->device), "hipSetDevice");
        auto g = std::make_shared<LoopGroup>();
        g->n = n;
        g->packed.resize(n);
        g->copied.resize(n);
        for (int i = 0; i < n; i++) {
            hipcheck(hipEventCreateWithFlags(&g->packed[i], hipEventDisableTiming), "hipEventCreate");
            hipcheck(hipEventCreateWithFlags(&g->copied[i], hipEventDisableTiming), "hipEventCreate");
            hipcheck(hipEventRecord(g->copied[i], ctxs[i]->stream), "hipEventRecord");
        }
        for (int i = 0; i < n; i++) {
            Halo* h = halo_of(ctxs[i]);
            hipcheck(h->reserve(ctxs[i]->S.LP), "halo buffers");
            h->nranks = n;
            h->rank = i;
            h->loop = g.get();
            g->members.push_back(h);
            g->streams.push_back(ctxs[i]->stream);
            ctxs[i]->loopgrp = g;
        }
    });
}

int mpas_rccl_unique_id(void* out128) {
    if (!out128) return MPAS_EINVAL;
    std::string err;
    if (rccl_unique_id(out128, err) != 0) {
        g_create_err = err;
        return MPAS_ERCCL;
    }
    return MPAS_OK;
}

int mpas_halo_rccl(mpas_ctx* c, int nranks, int rank, const void* id128) {
    return guarded(c, [&] {
        if (nranks < 1 || rank < 0 || rank >= nranks || !id128) throw Fail{MPAS_EINVAL, "mpas_halo_rccl: bad arguments"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        Halo* h = halo_of(c);
        hipcheck(h->reserve(c->S.LP), "halo buffers");
        std::string err;
        if (rccl_init(h, nranks, rank, id128, err) != 0) throw Fail{MPAS_ERCCL, err};
    });
}

int mpas_halo_socket(mpas_ctx* c, int nranks, int rank, const char* host, int base_port) {
    return guarded(c, [&] {
        if (nranks < 1 || rank < 0 || rank >= nranks || !host || base_port <= 0 || base_port + nranks > 65535)
            throw Fail{MPAS_EINVAL, "mpas_halo_socket: bad arguments"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        Halo* h = halo_of(c);
        if (h->rccl || h->loop || h->stub || h->sock) throw Fail{MPAS_EINVAL, "mpas_halo_socket: the context already has a transport"};
        hipcheck(h->reserve(c->S.LP), "halo buffers");
        std::string err;
        if (sock_init(h, nranks, rank, host, base_port, err) != 0) throw Fail{MPAS_EINVAL, err};
        graph_drop(c);
    });
}

int mpas_halo_stub(mpas_ctx* c) {
    return guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        Halo* h = halo_of(c);
        if (h->rccl || h->loop || h->sock) throw Fail{MPAS_EINVAL, "mpas_halo_stub: the context already has a transport"};
        hipcheck(h->reserve(c->S.LP), "halo buffers");
        h->stub = true;
        graph_drop(c);
    });
}

int mpas_halo_stats(mpas_ctx* c, int64_t* exchanges, int64_t* fields) {
    if (!c || !exchanges || !fields) return MPAS_EINVAL;
    *exchanges = c->halo ? c->halo->exchanges : 0;
    *fields = c->halo ? c->halo->fields_moved : 0;
    return MPAS_OK;
}

#define MPAS_TASK(NAME, CALL) \
    return guarded(c, [&] { run_task(c, NAME, [&] { return CALL; }); })

int mpas_atm_rk_integration_setup(mpas_ctx* c) {
    MPAS_TASK("atm_rk_integration_setup", launch_rk_integration_setup(c->S, c->stream));
}
int mpas_atm_compute_moist_coefficients(mpas_ctx* c) {
    MPAS_TASK("atm_compute_moist_coefficients", launch_moist_coefficients(c->S, c->stream));
}
int mpas_atm_compute_vert_imp_coefs(mpas_ctx* c, double dts) {
    MPAS_TASK("atm_compute_vert_imp_coefs", launch_vert_imp_coefs(c->S, c->stream, dts));
}
int mpas_atm_compute_dyn_tend_work(mpas_ctx* c, int rk_step, double dt, int horiz_mixing, double cam_coef, int mix_full,
                                   int rayleigh_damp_u) {
    if (!c) return MPAS_EINVAL;
    DynTendArgs a{rk_step, dt, horiz_mixing, cam_coef, mix_full, rayleigh_damp_u, c->exact};
    MPAS_TASK(rk_step == 0 ? "atm_compute_dyn_tend_work[rk0]" : "atm_compute_dyn_tend_work[rk>0]",
              launch_dyn_tend(c->S, c->stream, a));
}
int mpas_atm_set_smlstep_pert_variables_work(mpas_ctx* c) {
    MPAS_TASK("atm_set_smlstep_pert_variables_work", launch_set_smlstep(c->S, c->stream, c->exact));
}
int mpas_atm_advance_acoustic_step_work(mpas_ctx* c, double dts, int small_step) {
    MPAS_TASK(acoustic_name(small_step).c_str(), launch_acoustic(c->S, c->stream, dts, small_step, c->exact));
}
int mpas_atm_divergence_damping_3d(mpas_ctx* c, double dts) {
    MPAS_TASK("atm_divergence_damping_3d", launch_div_damping(c->S, c->stream, dts));
}
int mpas_atm_compute_solve_diagnostics(mpas_ctx* c, int hollingsworth, int rk_step) {
    MPAS_TASK("atm_compute_solve_diagnostics", launch_solve_diagnostics(c->S, c->stream, hollingsworth, rk_step));
}
int mpas_atm_rk_dynamics_substep_finish(mpas_ctx* c, int substep, int split) {
    if (split == 0) return MPAS_EINVAL;
    MPAS_TASK("atm_rk_dynamics_substep_finish", launch_substep_finish(c->S, c->stream, substep, split));
}

int mpas_atm_recover_large_step_variables_work(mpas_ctx* c, int ns, int rk_step, double dt) {
    if (ns == 0) return MPAS_EINVAL;
    MPAS_TASK(recover_name(rk_step), launch_recover_large_step(c->S, c->stream, ns, rk_step, dt));
}
int mpas_reconstruct_2d(mpas_ctx* c, int includeHalos, int on_a_sphere) {
    (void)includeHalos;  // :1909-1912: the range is nCells either way
    MPAS_TASK("mpas_reconstruct_2d", launch_reconstruct_2d(c->S, c->stream, on_a_sphere ? 1 : 0));
}
// (the init tasks write state fields at every level from outside the step: the keep tails
// follow them, mpas_dev.h)
int mpas_atm_compute_damping_coefs(mpas_ctx* c, double config_zd, double config_xnutr) {
    return guarded(c, [&] {
        run_task(c, "atm_compute_damping_coefs",
                 [&] { return launch_damping_coefs(c->S, c->stream, config_zd, config_xnutr); });
        keep_refresh_all(c);
    });
}
int mpas_atm_init_coupled_diagnostics(mpas_ctx* c) {
    return guarded(c, [&] {
        run_task(c, "atm_init_coupled_diagnostics", [&] { return launch_init_coupled_diagnostics(c->S, c->stream); });
        keep_refresh_all(c);
    });
}
// the mesh tasks of atm_core_init (k_mesh.hip); the adv lists feed k_prepare's edge
// records and the transport tiles, so they are re-derived before the next task
int mpas_atm_compute_signs(mpas_ctx* c) { MPAS_TASK("atm_compute_signs", launch_compute_signs(c->S, c->stream)); }
int mpas_atm_adv_coef_compression(mpas_ctx* c) {
    return guarded(c, [&] {
        run_task(c, "atm_adv_coef_compression", [&] { return launch_adv_coef_compression(c->S, c->stream); });
        c->dirty = true;
        c->trt_dirty = c->ett_dirty = true;
        graph_drop(c);
    });
}
int mpas_atm_couple_coef_3rd_order(mpas_ctx* c, double config_coef_3rd_order) {
    MPAS_TASK("atm_couple_coef_3rd_order", launch_couple_coef_3rd_order(c->S, c->stream, config_coef_3rd_order));
}
int mpas_atm_compute_mesh_scaling(mpas_ctx* c, int config_h_ScaleWithMesh) {
    MPAS_TASK("atm_compute_mesh_scaling", launch_mesh_scaling(c->S, c->stream, config_h_ScaleWithMesh));
}
int mpas_atm_core_init(mpas_ctx* c) {
    // atm_core.rg:22-42 in order (physics_init is a stub, OUT OF SCOPE; the namelist values
    // config_coef_3rd_order = 0.25, config_h_ScaleWithMesh = true, config_zd = 22000,
    // config_xnutr = 0.2)
    return guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        const DevState& S = c->S;
        hipStream_t st = c->stream;
        run_task(c, "atm_compute_signs", [&] { return launch_compute_signs(S, st); });
        run_task(c, "atm_adv_coef_compression", [&] { return launch_adv_coef_compression(S, st); });
        c->dirty = true;  // (k_prepare re-derives the edge records before the next task)
        c->trt_dirty = c->ett_dirty = true;
        graph_drop(c);
        run_task(c, "atm_couple_coef_3rd_order", [&] { return launch_couple_coef_3rd_order(S, st, 0.25); });
        run_task(c, "atm_init_coupled_diagnostics", [&] { return launch_init_coupled_diagnostics(S, st); });
        run_task(c, "atm_compute_solve_diagnostics", [&] { return launch_solve_diagnostics(S, st, 0, -1); });
        run_task(c, "mpas_reconstruct_2d", [&] { return launch_reconstruct_2d(S, st, 1); });
        run_task(c, "atm_compute_mesh_scaling", [&] { return launch_mesh_scaling(S, st, 1); });
        run_task(c, "atm_compute_damping_coefs", [&] { return launch_damping_coefs(S, st, 22000.0, 0.2); });
        keep_refresh_all(c);  // (the init tasks write the state from outside the step)
    });
}
int mpas_atm_advance_scalars_mono(mpas_ctx* c, double dt) {
    if (!c) return MPAS_EINVAL;
    return guarded(c, [&] {
        run_task(c, "atm_advance_scalars_mono", [&] {
            trt_ensure(c);
            return launch_advance_scalars_mono(c->S, c->stream, dt);
        });
    });
}
int mpas_atm_advance_scalars(mpas_ctx* c, double dt) {
    if (!c) return MPAS_EINVAL;
    return guarded(c, [&] {
        tr_rk_supported(c, "atm_advance_scalars");
        run_task(c, "atm_advance_scalars", [&] { return launch_advance_scalars(c->S, c->stream, dt); });
    });
}
int mpas_atm_advance_scalars_mono_rk(mpas_ctx* c, double dt) {
    if (!c) return MPAS_EINVAL;
    return guarded(c, [&] {
        tr_rk_supported(c, "atm_advance_scalars_mono_rk");
        run_task(c, "atm_advance_scalars_mono_rk", [&] {
            trt_ensure(c);
            return launch_advance_scalars_mono_rk(c->S, c->stream, dt);
        });
    });
}
int mpas_atm_held_suarez_forcing(mpas_ctx* c) {
    MPAS_TASK("atm_held_suarez_forcing", launch_held_suarez_forcing(c->S, c->stream));
}
// ---- the Kessler microphysics (k_kessler.hip): the task (a field-writing call like any other), and its
// accumulators, which are no fields (reading or zeroing them leaves what the step keeps as it is)
int mpas_atm_kessler_microphysics(mpas_ctx* c, double dt) {
    return guarded(c, [&] {
        if (c->S.physics != 2) throw Fail{MPAS_EINVAL, "atm_kessler_microphysics needs physics = 2 (the MPAS dynamics' state)"};
        if (!(dt > 0.0)) throw Fail{MPAS_EINVAL, "atm_kessler_microphysics: dt must be positive"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        precip_ensure(c);
        run_task(c, "atm_kessler_microphysics", [&] { return launch_kessler(c->S, c->stream, dt, c->precip); });
    });
}
int mpas_precip_read(mpas_ctx* c, int which, double* out, int64_t stride_cell) {
    return guarded(c, [&] {
        if (which < 0 || which > 2 || !out) throw Fail{MPAS_EINVAL, "mpas_precip_read: which must be 0..2, out not null"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        precip_ensure(c);
        const int nCO = c->S.nCO;
        std::vector<double> h((size_t)nCO);
        if (nCO)
            hipcheck(hipMemcpyAsync(h.data(), c->precip + (size_t)which * c->S.nCells, h.size() * sizeof(double),
                                    hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync D2H");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        for (int e = 0; e < nCO; e++) *(double*)((char*)out + e * stride_cell) = h[(size_t)e];
    }, true);
}
int mpas_precip_reset(mpas_ctx* c) {
    return guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        precip_ensure(c);
        hipcheck(hipMemsetAsync(c->precip, 0, 3 * (size_t)c->S.nCells * sizeof(double), c->stream), "hipMemsetAsync");
    }, true);
}
// ---- the surface fluxes and the boundary layer (k_pbl.hip): the task, the surface temperature it reads and its
// accumulators, which are no fields.  A new surface temperature changes what a step with option pbl computes but
// not its launches: the captured graph reads the same buffer
int mpas_atm_surface_pbl(mpas_ctx* c, double dt) {
    return guarded(c, [&] {
        if (c->S.physics != 2) throw Fail{MPAS_EINVAL, "atm_surface_pbl needs physics = 2 (the MPAS dynamics' state)"};
        if (!(dt > 0.0)) throw Fail{MPAS_EINVAL, "atm_surface_pbl: dt must be positive"};
        if (!c->sst) throw Fail{MPAS_EINVAL, "atm_surface_pbl needs a surface temperature (mpas_surface_set_temperature)"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        sflux_ensure(c);
        run_task(c, "atm_surface_pbl", [&] { return launch_surface_pbl(c->S, c->stream, dt, c->sst, c->sflux); });
    });
}
int mpas_surface_set_temperature(mpas_ctx* c, const double* ts, int64_t stride_cell) {
    return guarded(c, [&] {
        if (!ts) throw Fail{MPAS_EINVAL, "mpas_surface_set_temperature: ts must not be null"};
        const int nCO = c->S.nCO;
        // (the cells past the owned ones are never read; they hold the last owned value)
        std::vector<double> h((size_t)c->S.nCells + 1, 0.0);
        for (int e = 0; e < nCO; e++) {
            const double v = *(const double*)((const char*)ts + e * stride_cell);
            if (!std::isfinite(v) || !(v > 0.0))
                throw Fail{MPAS_EINVAL, "mpas_surface_set_temperature: cell " + std::to_string(e) + " is not a positive finite temperature"};
            h[(size_t)e] = v;
        }
        for (size_t e = (size_t)nCO; e < h.size(); e++) h[e] = nCO ? h[(size_t)nCO - 1] : 300.0;
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        if (!c->sst && hipMalloc((void**)&c->sst, h.size() * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            c->sst = nullptr;
            throw Fail{MPAS_ENOMEM, "hipMalloc surface temperature"};
        }
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        hipcheck(hipMemcpy(c->sst, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy H2D");
    }, true);
}
int mpas_surface_flux_read(mpas_ctx* c, int which, double* out, int64_t stride_cell) {
    return guarded(c, [&] {
        if (which < 0 || which > 2 || !out) throw Fail{MPAS_EINVAL, "mpas_surface_flux_read: which must be 0..2, out not null"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        sflux_ensure(c);
        const int nCO = c->S.nCO;
        std::vector<double> h((size_t)nCO);
        if (nCO)
            hipcheck(hipMemcpyAsync(h.data(), c->sflux + (size_t)which * c->S.nCells, h.size() * sizeof(double),
                                    hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync D2H");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        for (int e = 0; e < nCO; e++) *(double*)((char*)out + e * stride_cell) = h[(size_t)e];
    }, true);
}
int mpas_surface_flux_reset(mpas_ctx* c) {
    return guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        sflux_ensure(c);
        hipcheck(hipMemsetAsync(c->sflux, 0, 3 * (size_t)c->S.nCells * sizeof(double), c->stream), "hipMemsetAsync");
    }, true);
}
// ---- the sigma-level statistics (k_stats.hip).  None of these calls writes a field or changes the form of the
// step, so what the step keeps from the one before (guarded's keeps_sml) stays valid
int mpas_sigma_stats_configure(mpas_ctx* c, int nsigma, const double* sigma) {
    return guarded(c, [&] {
        if (nsigma < 0 || nsigma > kStatsMaxSigma || (nsigma && !sigma))
            throw Fail{MPAS_EINVAL, "mpas_sigma_stats_configure: nsigma must be 0..64"};
        for (int j = 0; j < nsigma; j++)
            if (!(sigma[j] > 0.0 && sigma[j] <= 1.0) || (j && !(sigma[j] < sigma[j - 1])))
                throw Fail{MPAS_EINVAL, "mpas_sigma_stats_configure: sigma levels must lie in (0, 1] and decrease strictly"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        stats_free(c);
        if (!nsigma) return;
        double h[2 * kStatsMaxSigma] = {};
        for (int j = 0; j < nsigma; j++) h[j] = sigma[j], h[kStatsMaxSigma + j] = std::log(sigma[j]);
        const size_t bytes = (size_t)c->S.nCells * stats_rec(nsigma) * sizeof(double);
        if (hipMalloc((void**)&c->stats_acc, bytes) != hipSuccess || hipMalloc((void**)&c->stats_sig, sizeof h) != hipSuccess) {
            (void)hipGetLastError();
            stats_free(c);
            throw Fail{MPAS_ENOMEM, "hipMalloc sigma stats"};
        }
        c->stats_ns = nsigma;
        hipcheck(hipMemcpy(c->stats_sig, h, sizeof h, hipMemcpyHostToDevice), "hipMemcpy H2D");
        stats_zero(c);
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    }, true);
}
int mpas_sigma_stats_reset(mpas_ctx* c) {
    return guarded(c, [&] {
        if (!c->stats_ns) throw Fail{MPAS_EINVAL, "mpas_sigma_stats_reset: no sigma levels configured"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        stats_zero(c);
    }, true);
}
int mpas_sigma_stats_read(mpas_ctx* c, int stat, double* out, int64_t stride_cell, int64_t stride_level) {
    return guarded(c, [&] {
        if (!c->stats_ns) throw Fail{MPAS_EINVAL, "mpas_sigma_stats_read: no sigma levels configured"};
        if (stat < 0 || stat > kStatsMoments || !out) throw Fail{MPAS_EINVAL, "mpas_sigma_stats_read: stat must be 0..9, out not null"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        const int ns = c->stats_ns, rec = stats_rec(ns), nCO = c->S.nCO;
        const int off = stat * ns, cnt = stat == kStatsMoments ? 3 : ns;
        std::vector<double> h((size_t)nCO * rec);
        if (nCO)
            hipcheck(hipMemcpyAsync(h.data(), c->stats_acc, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream),
                     "hipMemcpyAsync D2H");
        hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
        for (int e = 0; e < nCO; e++)
            for (int j = 0; j < cnt; j++)
                *(double*)((char*)out + e * stride_cell + j * stride_level) = h[(size_t)e * rec + off + j];
    }, true);
}
int mpas_atm_sigma_stats_accumulate(mpas_ctx* c) {
    return guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        stats_accumulate(c);
    }, true);
}
int mpas_atm_compute_output_diagnostics(mpas_ctx* c) {
    MPAS_TASK("atm_compute_output_diagnostics", launch_output_diagnostics(c->S, c->stream));
}
int mpas_summarize_timestep(mpas_ctx* c, int detailed, int global_vel, int global_sca, double* out) {
    (void)global_sca;  // prints a blank line only (rk_timestep.rg:352-357)
    return guarded(c, [&] {
        if (!out) throw Fail{MPAS_EINVAL, "mpas_summarize_timestep: null out"};
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        double h[31] = {0};
        if (detailed || global_vel) {
            if (!c->sum_scratch) hipcheck(hipMalloc(&c->sum_scratch, summarize_scratch_bytes()), "hipMalloc");
            if (!c->sum_out) hipcheck(hipMalloc((void**)&c->sum_out, 31 * sizeof(double)), "hipMalloc");
            run_task(c, "summarize_timestep", [&] { return launch_summarize(c->S, c->stream, c->sum_scratch, c->sum_out); });
            hipcheck(hipMemcpyAsync(h, c->sum_out, sizeof h, hipMemcpyDeviceToHost, c->stream), "hipMemcpy D2H");
            hipcheck(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
            if (!detailed)
                for (int i = 0; i < 27; i++) h[i] = 0.0;
            if (!global_vel)
                for (int i = 27; i < 31; i++) h[i] = 0.0;
        }
        std::memcpy(out, h, sizeof h);
    }, true);
}

int mpas_atm_srk3(mpas_ctx* c, double dt, int schedule) {
    const int rc = guarded(c, [&] {
        hipcheck(hipSetDevice(c->device), "hipSetDevice");
        if (c->transport == 2) tr_rk_supported(c, "atm_srk3 with transport = 2");  // (never inside a capture)
        srk3_step(c, dt, schedule);
    }, true);
    if (c && rc != MPAS_OK) c->sml_valid = false, c->keep_gen = 0;  // (a failed step promises nothing)
    return rc;
}
int mpas_atm_timestep(mpas_ctx* c, double dt) { return mpas_atm_srk3(c, dt, 0); }

int mpas_timing_enable(mpas_ctx* c, int on) {
    return guarded(c, [&] { c->timing = on != 0; }, true);
}
int mpas_timing_reset(mpas_ctx* c) {
    return guarded(c, [&] {
        harvest(c);
        for (auto& x : c->task_calls) x = 0;
        for (auto& x : c->task_ms) x = 0.0;
    }, true);
}
int mpas_timing_count(mpas_ctx* c) {
    if (!c) return MPAS_EINVAL;
    int rc = guarded(c, [&] { harvest(c); }, true);
    return rc != MPAS_OK ? rc : (int)c->task_names.size();
}
int mpas_timing_get(mpas_ctx* c, int idx, const char** name, int64_t* calls, double* total_ms) {
    return guarded(c, [&] {
        harvest(c);
        if (idx < 0 || idx >= (int)c->task_names.size()) throw Fail{MPAS_EINVAL, "timing index"};
        if (name) *name = c->task_names[idx].c_str();
        if (calls) *calls = c->task_calls[idx];
        if (total_ms) *total_ms = c->task_ms[idx];
    }, true);
}

}  // extern "C"
