/* mpas_dyn.h -- C-ABI of libmpasdyn, the MI355X (gfx950) drop-in for the RK3 dynamics
 * hot path of alexaiken/mpas-regent (dynamics/rk_timestep.rg:361-519 and the leaf
 * tasks of dynamics/dynamics_tasks.rg).
 *
 * Boundary.  Each Regent leaf task of the path becomes one extern "C" entry point with
 * the task's name (prefixed mpas_) and its scalar parameters in the task's order.  The
 * task's region arguments (cr, cpr, er, vr, vert_r) are the device-resident state owned
 * by an mpas_ctx; fields move across the boundary with mpas_upload / mpas_download,
 * which take a plain host pointer and byte strides, so the Legion SOA layout a Regent
 * binding would hand over (legion_accessor_array_*_raw_rect_ptr: entity stride, level
 * stride; fortran/examples.rg:21-46) is accepted as is.  Field ids are the Regent field
 * names (data_structures.rg), looked up with mpas_field_id.
 *
 * Conventions.  Every function returns 0 on success or a negative MPAS_E* code; the
 * message is in mpas_last_error(ctx).  No C++ exception crosses the ABI.  A context owns
 * one HIP device and its streams and is single-threaded; separate contexts may be
 * driven from separate host threads.  Task calls are stream-ordered (asynchronous);
 * mpas_sync waits.  The host arrays passed to upload/download are borrowed for the call.
 * There is no CPU fallback: without a usable gfx950 device mpas_ctx_create fails.
 */
#ifndef MPAS_DYN_H
#define MPAS_DYN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPAS_OK 0
#define MPAS_EINVAL (-1)
#define MPAS_EHIP (-2)
#define MPAS_ERCCL (-3)
#define MPAS_ENOMEM (-4)
#define MPAS_ENOTSUP (-5)
/* bounds-checked build only (libmpasdyn_bounds.so, `make -C mpas-regent_amd/csrc bounds`):
 * a kernel of the call accessed a field outside its rows; the message names the field.
 * Option "bounds" (read-only) is 1 in that build; "bounds_units" (read-only) packs the
 * translation units whose kernels check (high 32 bits) and those registered (low);
 * "bounds_probe" = n makes it read field u n columns past its end (the check's own test). */
#define MPAS_EBOUNDS (-6)

typedef struct mpas_ctx mpas_ctx;

/* mesh dimensions; constants.rg:18-26 (nCells, nEdges, nVertices, nVertLevels) */
typedef struct {
    int32_t nCells;
    int32_t nEdges;
    int32_t nVertices;
    int32_t nVertLevels; /* L; fields carry L+1 levels (main.rg:21-24), L+1 <= 64 */
} mpas_dims;

/* ---- context and residency ---------------------------------------------------- */
int mpas_ctx_create(mpas_ctx** out, int device, const mpas_dims* dims);
int mpas_ctx_destroy(mpas_ctx* ctx);
const char* mpas_last_error(const mpas_ctx* ctx);
int mpas_sync(mpas_ctx* ctx);
/* the HIP stream (hipStream_t) the tasks run on, for callers that time with events */
int mpas_get_stream(mpas_ctx* ctx, void** stream);
/* options: "exact" = 1 makes the reassociated kernels (Q10 q sum, acoustic scan, set_smlstep's
 * slope-flux sum) evaluate the reference's literal order (bit-identical to the oracle, slower);
 * "xcd" = 0 dispatcher block order, 1 one contiguous eighth of the columns per XCD,
 * G > 1 runs of G blocks per XCD inside windows of 8G (default 64); "epw" = 1, 2 (default)
 * or 4 entities per column slot in div_damping / solve_diagnostics; "cve" = 1, 4 or 8
 * vertices per wavefront in dyn_tend's delsq_vorticity (default 0: 4); "vcmix" = 1 (default)
 * interleaves the vertex and cell blocks of the mixed grids; "overlap" = 1 (default)
 * computes interior entities beside the halo exchange of a decomposed mesh; "self" = 0
 * disables the SELF gathers; "graph" = 1 (default) makes mpas_atm_srk3 capture its step once
 * per (dt, schedule) as a HIP graph and replay it (any option change or mesh upload
 * re-captures; per-task timing runs the launches directly; read-only "graph_captures" /
 * "graph_launches" count them).  "graph_halo" does the same on a decomposed context: 2
 * (default) with the stub transport, 1 with the RCCL transport too (opt-in: its grouped
 * send / recv has been captured on a 1-rank communicator only), 0 never; a step is
 * captured per halo state at its start (a start state met twice; up to 4 kept), and a
 * capture the transport refuses falls back to eager steps (read-only "graph_fallbacks").  "stub_latency_us" (stub transport only) adds a
 * device-side wait of that many microseconds to every exchange (tools/rank_sim.py).  All but
 * "exact" and "physics" change only speed, never results.
 * Cross-task fusion in mpas_atm_srk3 (reference semantics):
 * "fusedamp" = 1 (default) applies each divergence damping inside the next acoustic launch
 * (read-only "fusedamp_active"); "fusesml" = 1 (default, with fusedamp) runs each stage's
 * set_smlstep inside its first acoustic launch; "smlsum" = 1 (default, with fusesml, exact = 0)
 * forms set_smlstep's slope-flux sum once per step (u_tend, zb_cell and zb3_cell are not written
 * within a step) and the stages' fused set_smlstep read it; "fusesetup" = 1 (default) runs setup, moist
 * and stage 0's vert_imp as one launch; "fusecopy" = 1 (default, with fusesetup) makes
 * setup's edge copies in stage 0's dyn_tend edge kernel (decomposed contexts and every
 * "physics" mode too); "defer4" = 1
 * (default) applies rk_step 0's del4 of tend_u_euler (dyn_tend kernel D) in the next stage's
 * rk_step > 0 edge kernel; "vdyn" = 1 (default) has the last stage's dyn_tend edge kernel store
 * solve_diagnostics' v from the u it gathers (when edgesOnEdge_ECP = edgesOnEdge, read-only
 * "eoe_same"); "ntu" = 1 (default; reference semantics, with defer4) leaves out what the stages
 * before the step's last would compute only for values no task reads before the last stage
 * rewrites them: their dyn_tend forms no tend_u and no theta tendencies (tend_theta,
 * tend_rtheta_adv, rthdynten), the last acoustic substep of stages 0 and 1 stores no rho_pp,
 * rtheta_pp, rw_p or wwAvg (the next stage's first substep sets them; the damping reads the div
 * that substep stores), stage 0's solve_diagnostics is not run and stage 1's stores ke and
 * pv_edge alone (its divergence, vorticity, h_edge and ke_edge are dead); every field after a step
 * is bit-identical with it off; 2 = the same with stage 1's solve_diagnostics whole, 3 = with the
 * acoustic state stored (A/Bs);
 * "etile" = 1 (default 0, measured, not kept) forms dyn_tend's theta advection fluxes from tiles
 * of cells in LDS ("etcells", "etclo", "etmode", "etthreads"; read-only "etile_active");
 * "bsplit" (fast path, speed only) puts dyn_tend's per-edge theta flux (and the MPAS dynamics' w
 * flux) in an edge kernel of its own beside the edge kernel B: 1 always, 2 (default) under
 * "physics" = 2 only, where B's registers would otherwise hold it to 3 waves per SIMD, 0 never.
 * "keep_check" = 1 (default 0; debug, slow) compares every field's keep tail -- the value of
 * each column's slot the reference never writes, which the kernels store back so that every
 * column is written as whole lines -- with the field after every task and fails the task
 * (MPAS_EINVAL, naming the task, the field and the first entity) on a mismatch.  "tmedge" = 1 (default 0) has
 * dyn_tend store theta_m(cell1) + theta_m(cell2) per edge for the acoustic substeps;
 * "hfuse" = 1 puts independent neighbouring kernels in one launch, 2 (default) only below
 * 16384 owned cells, undecomposed (read-only "hfuse_active"). "fusedamp_halo" = 1 (default)
 * applies fusedamp and fusesml on decomposed meshes too (with "ring1"): the div is exchanged
 * where rtheta_pp was.  Under "physics" >= 1 "fusesetup" runs setup, moist and stage 0's
 * vert_imp in their MPAS forms as one launch.
 * "physics" = 1 selects the MPAS vertical solver: vert_imp with Q16/Q17
 * fixed, the acoustic step with the ru_p update (Q18), the MPAS statement order (Q19/Q20)
 * and the tridiagonal back substitution (Q21), tend_rt = tend_theta (Q8), recover_large_step
 * with Q24 fixed, and in mpas_atm_srk3 number_sub_steps acoustic substeps (Q5) followed by
 * recover (Q7); every other task as the reference.
 * "physics" = 2 adds the MPAS dynamics (every remaining quirk of the path fixed, so the JW
 * state evolves as a dynamical core): dyn_tend with the w tendency in tend_w computed from
 * the state w (Q8, Q13, Q14), q once (Q10), the MPAS curvature (Q12) and wdtz (Q15);
 * solve_diagnostics with h = rho_zz, rho_edge = h_edge, divergence sign*u (Q9) and v over
 * every edgesOnEdge entry (Q23); set_smlstep on tend_u / tend_w (Q2); setup also saving
 * theta_m_save; moist setting cqu (Q25); mpas_reconstruct_2d after the RK loop; the substep
 * finish keeping rho_zz; atm_compute_output_diagnostics also writing surface_pressure.
 * Default 0: the reference's semantics.
 * "transport" = 1 (needs "physics" >= 1) makes mpas_atm_srk3 copy scalars
 * to scalars_old first and run mpas_atm_advance_scalars_mono(dt) after the last stage's
 * recover, before atm_rk_dynamics_substep_finish.  "transport" = 2 (the same need) integrates
 * the scalars with MPAS-A's three-stage RK3 instead: after the same copy and at the same place,
 * mpas_atm_advance_scalars(dt/3), mpas_atm_advance_scalars(dt/2), then
 * mpas_atm_advance_scalars_mono_rk(dt), every stage with the step's ruAvg, wwAvg and
 * rho_zz_old_split (third order in time where the limiter is idle; the copy is always the
 * separate one; MPAS_ENOTSUP with "trtile", "tredge", "trsu" or "trepw" = 2).  Any other value:
 * MPAS_EINVAL.  Default 0.  "trorder" (speed only)
 * orders the transport's column slots: 0 entity-major, 1 pair-major, R >= 2 pair-major
 * within runs of R consecutive entities, one run per XCD (default 64); "trorder_e" the same
 * for the transport's edge kernel alone (0, the default: trorder's).  "trsu" = 1 (speed only; measured
 * slower, default 0): the transport's update forms the upwind update su again instead of
 * storing and reading it.  "trsave" = 1 (default; speed only) folds mpas_atm_srk3's scalars_save
 * copy into the transport (undecomposed, the default transport kernels): they read the old scalars
 * from scalars and the bounds kernel stores scalars_old.  "mdamp" = 1 (default; speed only; the MPAS
 * forms) applies each divergence damping in the kernel that next reads ru_p (the next substep's ru_p
 * kernel, the stage's recover edge kernel); "mru" = 1 (default; the MPAS dynamics, fast path) has
 * the kernel forming a stage's final tend_u store its first acoustic substep's ru_p and ruAvg;
 * "msml" = 1 (default; the MPAS dynamics) applies each stage's set_smlstep in dyn_tend's cell
 * kernel.  "accoef" = 1 (default; speed only; mpas_atm_srk3 in the reference semantics, not with
 * "tmedge"): the acoustic launches form cofwr, coftz and a_tri from the columns they hold (zz, theta_m,
 * cofwz, cofwt) by vert_imp's own expressions instead of loading the stored columns, and stage 0's setup
 * launch leaves the three unstored (stage 1's vert_imp stores them): every field after a step
 * bit-identical; mpas_atm_advance_acoustic_step_work always reads the stored columns; a value other
 * than 0 or 1: MPAS_EINVAL.  "dd0" = 1 (default; speed only; mpas_atm_srk3 in the reference semantics):
 * the acoustic launches take rw_save - rw, their only use of the two columns, as the constant 0.0 and
 * load neither -- the step's setup stores rw_save = rw where the difference is read and no task of the
 * step writes rw: every field after a step bit-identical for finite rw (where rw is not finite the
 * reference's NaN from rw_save - rw no longer enters); mpas_atm_advance_acoustic_step_work always
 * reads the stored columns; a value other than 0 or 1: MPAS_EINVAL.  "smlkeep" = 1 (default; speed
 * only; with "smlsum", undecomposed contexts): set_smlstep's slope-flux sum is formed ahead of a
 * step only when its inputs may have changed since it was last formed, not in every step.  Every
 * call of this interface makes the next step form it again, except mpas_atm_srk3 / mpas_atm_timestep
 * themselves and the calls that write no field and no option (mpas_download, mpas_sync,
 * mpas_get_option, mpas_get_stream, mpas_timing_*, mpas_field_*, mpas_halo_stats, mpas_last_error,
 * mpas_summarize_timestep): a changed u_tend / zb_cell / zb3_cell counts at the very next step.
 * Device memory of a context written behind this interface is not seen.  A value other than 0 or
 * 1: MPAS_EINVAL.  "stepkeep" = 1 (default; speed only; where "smlkeep" applies, with "ntu" = 1, "defer4",
 * "fusesetup", "fusecopy" and "accoef" on, "hfuse", "tmedge", "etile", the transport and the forcing off,
 * stage 0 at rk_step 0 and stages 1, 2 at rk_step > 0): no task of the reference-semantics step writes u,
 * ru, rw, rho_zz, theta_m, rho_p, rtheta_p, h, zz, exner or the base fields, so a step that follows a full
 * step with the same dt and schedule, and no call in between but those "smlkeep" lists, runs no
 * solve_diagnostics launch and stores none of the setup's copies of those fields nor qtot / cqw: they hold
 * what it would store.  "stepkeep" = 2 also drops stage 0's dyn_tend from the third such step on (its w is
 * restored from a copy; stage 2 forms tend_u, v and w alone): every field bit-identical either way, but the
 * per-task timing of such a step has no rk_step 0 dyn_tend row.  0: every launch in every step.  A non-finite
 * value in one of those fields then no longer re-enters each step.  Any other value: MPAS_EINVAL.  Read-only
 * "stepkeep_gen": the steps completed since the last call that could have changed a field or the form of
 * the step (0, 1, or 2 for two and more).  "vikeep" = 1 (default; speed only; exactly where "stepkeep" is
 * active): every input of atm_compute_vert_imp_coefs is a field no task of the step writes, so each of the
 * step's two coefficient sets is the same in every consecutive step but for alpha_tri / gamma_tri (the
 * recurrence over calls).  Stage 0's set is kept in scratch columns -- cofwt, cofwz, cofwr, coftz, a_tri, b_tri
 * and c_tri hold stage 1's after any step, as before -- and a step at "stepkeep_gen" >= 1 forms alpha_tri and
 * gamma_tri alone, from the stored a, b, c and the gamma_tri it finds.  Such a step also runs stage 2's
 * dyn_tend without the kernel that stores h_divergence (a function of ru and the mesh), with or without
 * "vikeep".  Every field bit-identical; 0: both sets formed in every step.  Any other value: MPAS_EINVAL.
 * "a0keep" = 1 (default; speed only; exactly where "stepkeep" is active): what stage 0's dyn_tend stores in its
 * first cell kernel -- tend_rho, dpdz, ru_save, u_2 -- is a function of fields no task of the step writes, but
 * for kdiff, which reads v.  A full step ends with one launch that forms the next step's kdiff in a scratch
 * column (timing key "a0keep_kdiff"; the field keeps the step's own); a step at "stepkeep_gen" >= 1 takes kdiff
 * from there, runs stage 0's dyn_tend without that kernel (its row tagged -A) and
 * atm_rk_dynamics_substep_finish without its edge part (ruAvg has no writer, so ruAvg_split = ruAvg is in
 * place).  Every field bit-identical; 0: every one of those launches in every step.  Any other value:
 * MPAS_EINVAL.
 * "dynkeep" = 1 (default; speed only; exactly where "a0keep" is active and "stepkeep" is 1): what the dyn_tend
 * calls of a step at "stepkeep_gen" >= 1 still form -- stage 0's edge, vertex and cell kernels, every stage's
 * last cell kernel -- is a function of fields no task of the step writes.  Such a step launches guarded
 * instances of those kernels, which load a flag in device memory: the first such step after a full one runs
 * them as before and also leaves tend_u_euler (before the deferred del4) and each stage's w in scratch columns;
 * the later ones copy those columns back and form nothing else.  The launches, the timing keys and the captured
 * graph are the same for both.  Read-only "dynkeep_fresh": the flag (1: the columns hold the running sequence's
 * values; a full step clears it).  Every field bit-identical; 0: the plain kernels.  Any other value:
 * MPAS_EINVAL.
 * "tukeep" = 1 (default; speed only; where "dynkeep" is active, in steps without per-task timing): between two steps at "stepkeep_gen" 2
 * the last stage's dyn_tend edge kernel stores other bits at one level of one column only -- tend_u below the
 * top, which reads w at the top -- so with the flag 1 its guarded instance returns and one small kernel behind
 * it, in the same task, forms that level from tend_u_euler as stored; stage 0's edge kernel then leaves
 * tend_u_euler alone.  With the flag 0 every launch works as under "dynkeep" alone.  The same launches, timing
 * keys and captured graph.  A step with
 * per-task timing on makes "dynkeep"'s launches, so that its dyn_tend rows time the task's whole work.
 * Read-only "tukeep_active": 1 where a kept step of this context would take that form now.
 * Every field bit-identical; 0: "dynkeep"'s launches.  Any other value: MPAS_EINVAL.
 * "trepw" = 2 (speed only; measured within 2 %, default 1): two
 * edges per wavefront in the transport's edge kernel.  "trtile" = 1
 * (speed only, default 0) runs the transport as two tiled kernels with the scalars of
 * compact cell tiles in LDS and no edge scratch, when every cell has at most 6 edges with
 * at most 9 advCells each (bit-identical; measured slower); "trtcells" and
 * "trtclo" bound a tile's cells (default 16) and LDS columns (default 96); read-only
 * "trtile_active" / "trtile_count" report whether tiles are built and how many.
 * "tredge" = 1 (speed only, default 0) stages each group of 16 consecutive edges' scalars_old
 * columns in LDS for the transport's edge kernel (bit-identical; measured slower, DESIGN.md
 * §7; read-only "tredge_active", "tredge_irregular").  On a decomposed context the tiles are built only with "trtile_ghosts" = 1, which declares that
 * the ghosts close over advCellsForEdge(edgesOnCell) (mpasdyn.decomp.Decomposition(...,
 * tiled_transport=True); lib.setup_subdomain sets it). */
int mpas_set_option(mpas_ctx* ctx, const char* name, int64_t value);
/* reads every option above ("self", default 1: when every cell is
 * among the cellsOnEdge of its own edges -- mpas-mode ids -- the cell kernels gather
 * only the other cell of an edge) and "selfc" (read-only: whether the SELF gathers are
 * in use for the uploaded mesh). */
int mpas_get_option(mpas_ctx* ctx, const char* name, int64_t* value);

/* field registry (include/mpas_fields.def order) */
int mpas_field_count(void);
int mpas_field_id(const char* name);
const char* mpas_field_name(int field_id);
int mpas_field_kind(int field_id);  /* 0 C3,1 C3V,2 E3,3 V3,4 C2F,5 C2I,6 E2F,7 E2I,8 V2F,9 V2I,10 C3B,11 ZV */
int mpas_field_width(int field_id);

/* Host <-> device copy of one field.  Element (entity e, level k, component i) is at
 * byte offset e*stride_entity + k*stride_level + i*stride_comp of host (levels 0..L,
 * entities 0..n-1; components only for array fields).  Element type: double for fp64
 * fields, int32 for integer fields, uint8 for masks.  Entity-id fields are clamped
 * on upload so that any id outside [0, n] resolves to the zero slot n; a list
 * length (nEdgesOnCell, nEdgesOnEdge, nAdvCellsForEdge) past its row width is refused.
 * The view may be device memory (a Legion instance in framebuffer memory, a torch tensor;
 * hipPointerGetAttributes decides): 3-D fields then move device to device with a strided
 * copy kernel, never through the host (non-negative strides); 2-D fields are staged. */
int mpas_upload(mpas_ctx* ctx, int field_id, const void* host, int64_t stride_entity, int64_t stride_level,
                int64_t stride_comp);
int mpas_download(mpas_ctx* ctx, int field_id, void* host, int64_t stride_entity, int64_t stride_level,
                  int64_t stride_comp);
/* Fill every synthetic-distribution field (mpas_fields.def DIST != M) on the device
 * with the counter-based generator of mpas_synth.h (benchmark inputs). */
int mpas_fill_synthetic(mpas_ctx* ctx, uint64_t seed);

/* ---- the hot-path tasks (dynamics_tasks.rg) ------------------------------------ */
/* :747  atm_rk_integration_setup(cr, er) */
int mpas_atm_rk_integration_setup(mpas_ctx* ctx);
/* :460  atm_compute_moist_coefficients(cr, er) */
int mpas_atm_compute_moist_coefficients(mpas_ctx* ctx);
/* :513  atm_compute_vert_imp_coefs(cr, vert_r, dts) */
int mpas_atm_compute_vert_imp_coefs(mpas_ctx* ctx, double dts);
/* :814  atm_compute_dyn_tend_work(cr, er, vr, vert_r, rk_step, dt, config_horiz_mixing,
 *       config_mpas_cam_coef, config_mix_full, config_rayleigh_damp_u);
 *       horiz_mixing: 0 "2d_smagorinsky", 1 "2d_fixed", 2 other */
int mpas_atm_compute_dyn_tend_work(mpas_ctx* ctx, int rk_step, double dt, int config_horiz_mixing,
                                   double config_mpas_cam_coef, int config_mix_full, int config_rayleigh_damp_u);
/* :1503 atm_set_smlstep_pert_variables_work(cpr, er, vert_r); cpr = field cprMask */
int mpas_atm_set_smlstep_pert_variables_work(mpas_ctx* ctx);
/* :1546 atm_advance_acoustic_step_work(cr, er, vert_r, dts, small_step) */
int mpas_atm_advance_acoustic_step_work(mpas_ctx* ctx, double dts, int small_step);
/* :1726 atm_divergence_damping_3d(cpr, er, dts); cpr's isShared = field isShared */
int mpas_atm_divergence_damping_3d(mpas_ctx* ctx, double dts);
/* :328  atm_compute_solve_diagnostics(cr, er, vr, hollingsworth, rk_step) */
int mpas_atm_compute_solve_diagnostics(mpas_ctx* ctx, int hollingsworth, int rk_step);
/* :1951 atm_rk_dynamics_substep_finish(cr, er, dynamics_substep, dynamics_split) */
int mpas_atm_rk_dynamics_substep_finish(mpas_ctx* ctx, int dynamics_substep, int dynamics_split);

/* ---- operators defined beside the RK3 loop but not run inside it ------------------ */
/* :1766 atm_recover_large_step_variables_work(cr, er, vert_r, ns, rk_step, dt); commented
 *       out of atm_srk3 (rk_timestep.rg:460, Q7); Q24 literal */
int mpas_atm_recover_large_step_variables_work(mpas_ctx* ctx, int ns, int rk_step, double dt);
/* :1893 mpas_reconstruct_2d(cr, er, includeHalos, on_a_sphere); atm_core_init
 *       (atm_core.rg:33); commented out of atm_srk3 (rk_timestep.rg:487) */
int mpas_reconstruct_2d(mpas_ctx* ctx, int includeHalos, int on_a_sphere);
/* :729 atm_compute_output_diagnostics(cr), main.rg:70 after the time loop: rho = rho_zz * zz,
 *       pressure = pressure_base + pressure_p on levels 0..nVertLevels-1 (theta is in the
 *       task's write set but its statement is commented out in the reference: unchanged) */
int mpas_atm_compute_output_diagnostics(mpas_ctx* ctx);
/* init_atm_case_jw (vertical_init/init_atm_cases.rg:366-432), host side, no context: the
 * per-column hydrostatic iteration of the JW initial state (10 temperature x 25 pressure
 * passes) for nCells columns of nVertLevels levels, arrays [cell][level] row-major:
 * latCell[nCells]; pb, rb, zz (base pressure, base density, zz) in; dzw, dzu, fzm, fzp the
 * vertical grid (length nVertLevels+1); pressure_p, rho_p, temperature out.  Split over
 * nthreads host threads (<= 0: all).  mpasdyn/jw.py calls it for the large meshes. */
int mpas_jw_hydrostatic(int32_t nCells, int32_t nVertLevels, const double* latCell, const double* pb,
                        const double* rb, const double* zz, const double* dzw, const double* dzu, const double* fzm,
                        const double* fzp, double* pressure_p, double* rho_p, double* temperature, int32_t nthreads);
/* One-time tasks of atm_core_init (atm_core.rg:22-42) that run on the device:
 * :274 atm_compute_damping_coefs(config_zd, config_xnutr, cr) (atm_core.rg:41, defaults
 *       22000.0 and 0.2): dss of the upper damping layer */
int mpas_atm_compute_damping_coefs(mpas_ctx* ctx, double config_zd, double config_xnutr);
/* :651 atm_init_coupled_diagnostics(cr, er, vert_r) (atm_core.rg:31): rho_zz /= zz, ru, rw,
 *       rho_p, rtheta_base, rtheta_p, exner, exner_base, pressure_p, pressure_base */
int mpas_atm_init_coupled_diagnostics(mpas_ctx* ctx);
/* The mesh tasks of atm_core_init (k_mesh.hip; ids compared as uploaded, the bounds the
 * reference leaves undefined as oracle/mpas_oracle.c states them; a decomposed context
 * computes its owned entities, its ghosts keep the uploaded values):
 * :46  atm_compute_signs(cr, er, vr) (atm_core.rg:22): edgesOnVertexSign, edgesOnCellSign,
 *       kiteForCell; zb_cell / zb3_cell (:88-110, the copy of er.zb / zb3 that
 *       init_atm_case_jw writes) stay as uploaded: the state keeps no er.zb, the host that
 *       builds the initial state uploads the copy (mpasdyn/jw.py) */
int mpas_atm_compute_signs(mpas_ctx* ctx);
/* :133 atm_adv_coef_compression(cr, er) (atm_core.rg:24): advCellsForEdge,
 *       nAdvCellsForEdge (the index of the list's last cell, :184), adv_coefs and
 *       adv_coefs_3rd from cellsOnCell, dcEdge, dvEdge and deriv_two (never initialised by
 *       the reference, Q2: upload zeros for its semantics) */
int mpas_atm_adv_coef_compression(mpas_ctx* ctx);
/* :303 atm_couple_coef_3rd_order(config_coef_3rd_order, cr, er) (atm_core.rg:27, 0.25):
 *       adv_coefs_3rd and zb3_cell (level 0) scaled */
int mpas_atm_couple_coef_3rd_order(mpas_ctx* ctx, double config_coef_3rd_order);
/* :595 atm_compute_mesh_scaling(cr, cpr, csr, cgr, er, config_h_ScaleWithMesh)
 *       (atm_core.rg:39, true): meshScalingDel2 / Del4 from meshDensity (the regional
 *       relaxation factors it also writes are read by no task of the path) */
int mpas_atm_compute_mesh_scaling(mpas_ctx* ctx, int config_h_ScaleWithMesh);
/* atm_core.rg:22 atm_core_init: every task in the reference's order -- compute_signs,
 *       adv_coef_compression, couple_coef_3rd_order(0.25), init_coupled_diagnostics,
 *       solve_diagnostics(hollingsworth = false, rk_step = -1), mpas_reconstruct_2d(false,
 *       true), compute_mesh_scaling(true), compute_damping_coefs(config_zd = 22000,
 *       config_xnutr = 0.2; constants.rg:103-104).  physics_init is a stub (OUT OF SCOPE).
 *       Needs the raw mesh uploaded: connectivity (incl. cellsOnCell, cellsOnVertex),
 *       dcEdge, dvEdge, deriv_two, meshDensity. */
int mpas_atm_core_init(mpas_ctx* ctx);
/* Monotonic scalar transport.  Replaces no reference entry point: the
 *       reference has none (Q26 -- scalars:double[8], data_structures.rg:36, is declared and
 *       never used; the north star names the transport).  MPAS-A's atm_advance_scalars_mono
 *       (flux-corrected transport): the 8 scalars of scalars_old are advected over dt by the
 *       mass fluxes ruAvg (edges) and wwAvg (interfaces) from density rho_zz_old_split to
 *       rho_zz with 3rd-order fluxes (adv_coefs, adv_coefs_3rd; flux3 vertically, coef 0.25)
 *       limited so that no new extrema appear; result in scalars (levels 0..nVertLevels-1).
 *       Statement order: oracle/mpas_oracle.c ora_mpas_advance_scalars_mono.  Decomposed
 *       contexts exchange scalars_old and the scratch on their ghosts like every task. */
int mpas_atm_advance_scalars_mono(mpas_ctx* ctx, double dt);
/* One unlimited stage of MPAS-A's atm_advance_scalars (the first two stages of its RK3 scalar
 *       transport; no reference entry point, Q26).  With s_old = scalars_old, s_flux = scalars as
 *       found, ro = rho_zz_old_split, u = ruAvg, w = wwAvg (interfaces 0 and nVertLevels carry no
 *       flux and are not read), sg = +1 where the cell is cellsOnEdge(e,0), else -1:
 *         H(e,k)  = u sum_j (adv_coefs_j + sign(u) adv_coefs_3rd_j) s_flux(advCell_j,k)
 *         V(c,kk) = the interface high-order flux of mpas_atm_advance_scalars_mono on s_flux
 *         D(c,k)  = invAreaCell sum_e sg dvEdge u + rdzw(k) (w(k+1) - w(k))
 *         rho_int = ro - dt D                      (MPAS's advance_density: a constant stays constant)
 *         scalars = (s_old ro - dt (invAreaCell sum_e sg H + rdzw(k) (V(k+1) - V(k)))) / rho_int
 *       Writes scalars (levels 0..nVertLevels-1) only; rho_zz is neither read nor written.
 *       MPAS_ENOTSUP with "trtile", "tredge", "trsu" or "trepw" = 2 set. */
int mpas_atm_advance_scalars(mpas_ctx* ctx, double dt);
/* mpas_atm_advance_scalars_mono with its two high-order fluxes (the edge sum over the adv list and
 *       the interface flux) evaluated on scalars as found -- the previous stage's estimate -- and
 *       everything else (upwind fluxes, bounds, the upwind update, R+ / R-) on scalars_old: the
 *       last stage of the RK3 scalar transport.  Bit-identical to mpas_atm_advance_scalars_mono
 *       when scalars equals scalars_old on entry.  MPAS_ENOTSUP as above. */
int mpas_atm_advance_scalars_mono_rk(mpas_ctx* ctx, double dt);
/* The Held-Suarez (1994) forcing: Newtonian relaxation of temperature to a prescribed radiative
 *       equilibrium and Rayleigh friction below sigma_b -- the two physics tendencies the MPAS forms
 *       of dyn_tend read ("physics" = 2).  No reference entry point (SURVEY scopes the reference's
 *       physics out, and it is stubs).  Reads the state as found.  With sigma_b = 0.7, k_f = 1/86400,
 *       k_a = 1/(40 86400), k_s = 1/(4 86400) (1/s), dTy = 60 K, dthz = 10 K, floor = 200 K,
 *       p0 = 1e5 Pa, g = 9.80616 and c2 = cos(latCell)^2 (glibc cos on the host, at upload), per
 *       owned cell c and level k < nVertLevels, rq(k) = rho_zz(k) (1 + qtot(k)):
 *         p     = pressure_base + pressure_p
 *         ps    = 0.5 (1 / rdzw(0)) g (1.25 rq(0) - 0.25 rq(1)) + pressure_p(0) + pressure_base(0)
 *                 (atm_compute_output_diagnostics' surface pressure; level 1 as found at nVertLevels = 1)
 *         sigma = p / ps;  w = max(0, (sigma - sigma_b) / (1 - sigma_b))
 *         kv    = k_f w;   kT = k_a + (k_s - k_a) w c2 c2
 *         theq  = max(floor / exner, 315 - dTy (1 - c2) - dthz log(p / p0) c2)
 *         tend_rtheta_physics = -kT rho_zz (theta_m - theq)
 *       and per owned edge e of cells c1, c2 = cellsOnEdge(e, 0:1):
 *         tend_ru_physics = -(0.5 (kv(c1,k) + kv(c2,k))) ru(e,k)
 *       Dry: theta_m stands for theta, the scalars stay passive.  Writes those two fields on levels
 *       0..nVertLevels-1 and no other field; level nVertLevels and the zero slot keep their values.
 *       Statement order: tests/forcing_ref.py (bit for bit but for log).  Decomposed contexts
 *       exchange the kv scratch on their ghost cells like every gathered field.
 *       Option "forcing" = 1 (needs "physics" = 2, else MPAS_EINVAL; a value other than 0 or 1:
 *       MPAS_EINVAL; default 0; reset to 0 when "physics" leaves 2) makes mpas_atm_srk3 run this
 *       task once per step, ahead of stage 0's setup: the tendencies are held over the three stages. */
int mpas_atm_held_suarez_forcing(mpas_ctx* ctx);
/* Time-mean statistics on sigma levels (k_stats.hip): what turns a forced run into a climate.  No reference
 *       entry point.  One call of the task samples the state as found on every owned cell column and adds the
 *       sample's first and second moments to per-cell fp64 accumulators ("physics" = 2, else MPAS_EINVAL; dry:
 *       theta_m stands for theta).  Per owned cell c and level k < nVertLevels:
 *         p(k) = pressure_base + pressure_p
 *         ps   = mpas_atm_held_suarez_forcing's, term for term (atm_compute_output_diagnostics' surface pressure)
 *         s(k) = p(k) / ps;   T(k) = theta_m(k) exner(k);   u(k) = uReconstructZonal, v(k) = uReconstructMeridional
 *       and per configured target sigma_j (j < nsigma <= 64; lsig_j = log(sigma_j), glibc log on the host at
 *       configure time):
 *         kb  = the lowest k in 0..nVertLevels-2 with s(k) >= sigma_j > s(k+1), decided on s itself, never on its
 *               logarithm (well defined for a column that is not monotone); none: the pair (c, j) takes no
 *               sample in this call
 *         a   = (lsig_j - log s(kb)) / (log s(kb+1) - log s(kb))
 *         X_j = X(kb) + a (X(kb+1) - X(kb))            for X in u, v, T
 *       The accumulators per (owned cell, j), each `acc += x` in call order: n (the sample count, as a double), u,
 *       v, T, uu, vv, TT, uv, vT -- stat 0..8 of mpas_sigma_stats_read -- and per cell [sum ps, sum ps^2, calls]
 *       (stat 9, three "levels").  They are not registry fields (mpas_field_count is unchanged); the task writes
 *       no field.  No floating-point atomics and no reduction across cells: two runs give the same bits.
 *       Statement order: tests/stats_ref.py (bit for bit but for log).  A decomposed context samples its owned
 *       cells; no exchange is needed.
 * mpas_sigma_stats_configure allocates and zeroes the accumulators for the nsigma targets sigma[0..nsigma)
 *       (nsigma = 0 frees them and sets "stats_every" to 0); MPAS_EINVAL for nsigma outside 0..64, a sigma outside
 *       (0, 1] or a list that does not decrease strictly.  mpas_sigma_stats_reset zeroes them.
 * mpas_sigma_stats_read copies one accumulator of the owned cells to out (the call synchronises): element
 *       (cell e, target j) at byte offset e*stride_cell + j*stride_level; stat 9: j = 0..2.
 * Option "stats_every" = N >= 0 (default 0; N > 0 needs "physics" = 2 and configured targets, else MPAS_EINVAL; a
 *       negative value: MPAS_EINVAL; reset to 0 when "physics" leaves 2) makes mpas_atm_srk3 run the task after
 *       every N-th step since the option was set, behind the step's mpas_reconstruct_2d: launched on the stream
 *       after the step (after the replay of a captured step -- the task is in no captured graph, so
 *       "graph_captures" is what it is without the option), under its own timing key
 *       "atm_sigma_stats_accumulate".  With 0 the step is launch for launch the step without the feature.
 *       Read-only "stats_samples": runs of the task since the accumulators were last zeroed. */
int mpas_sigma_stats_configure(mpas_ctx* ctx, int32_t nsigma, const double* sigma);
int mpas_sigma_stats_reset(mpas_ctx* ctx);
int mpas_sigma_stats_read(mpas_ctx* ctx, int32_t stat, double* out, int64_t stride_cell, int64_t stride_level);
int mpas_atm_sigma_stats_accumulate(mpas_ctx* ctx);
/* Kessler warm-rain microphysics (k_kessler.hip) in the form of the DCMIP-2016 moist test cases (Klemp et al.
 *       2015): the first writer of rt_diabatic_tend and the first reader of the transported scalars.  No reference
 *       entry point ("physics" = 2, else MPAS_EINVAL; dt > 0).  Scalars 0, 1, 2 are qv, qc, qr (kg/kg).  Per owned
 *       cell column, levels k = 0..L-1 (L = nVertLevels, 0 the lowest), every input as found:
 *         rho_d = zz rho_zz;   m = rho_zz / rdzw (layer mass, kg/m2: the metric the transport conserves)
 *         dz = 1 / (rdzw zz);  pi = exner, held fixed over the call;   rvord = 461.6 / 287
 *         theta = theta_m / (1 + rvord qv);   T = pi theta (from the current theta in every subcycle)
 *       constants f2x = 17.27, Lv = 2.5e6, cp = 1003, f5 = 237.3 f2x Lv / cp, xk = 0.2875, psl = 1000:
 *         r = 0.001 rho_d;   pc = 3.8 / (pi^(1/xk) psl);   vt = 36.34 (qr r)^0.1364 sqrt(rho_d(0) / rho_d)
 *         x = max_k vt(k) dt / (0.8 dz(k));   n = max(1, ceil(x)) (at most 4096);   dt0 = dt / n
 *       n is the column's and fixed for the call; vt is formed again before every subcycle but the first.  One
 *       subcycle, a finite-volume sedimentation on the model's layers, then the DCMIP scheme's sources:
 *         F(k) = rho_d qr vt, F(L) = 0;   P += dt0 F(0) (kg/m2 = mm);   sed = dt0 (F(k+1) - F(k)) / m
 *         qrprod = qc - (qc - dt0 max(0.001 (qc - 0.001), 0)) / (1 + dt0 2.2 qr^0.875)
 *         qc = max(qc - qrprod, 0);   qr = max(qr + qrprod + sed, 0)
 *         qvs = pc exp(f2x (T - 273) / (T - 36));   prod = (qv - qvs) / (1 + qvs f5 / (T - 36)^2)
 *         ern = min(dt0 ((1.6 + 124.9 (r qr)^0.2046) (r qr)^0.525 / (2.55e6 pc / (3.8 qvs) + 5.4e5))
 *                   max(qvs - qv, 0) / (r qvs),  max(-prod - qc, 0),  qr)
 *         cond = max(prod, -qc);   theta += Lv / (cp pi) (cond - ern)
 *         qv = max(qv - cond + ern, 0);   qc += cond;   qr -= ern
 *       The powers of r qr are exp(a log(r qr)) on one logarithm per evaluation point, taken as -inf (every
 *       power 0) where r qr <= 0 -- a rain the transport's limiter left a rounding below zero gives no NaN and
 *       the subcycle's max(., 0) lifts it; qr^0.875 = exp(0.875 (log(r qr) - log r)); max and min are selects on
 *       > and <.  Written, with theta', qv' the values
 *       after the last subcycle:
 *         theta_m' = theta_m + (theta' - theta)(1 + rvord qv') + theta rvord (qv' - qv)
 *         rt_diabatic_tend = (theta_m' - theta_m) / dt;   rtheta_p' = rtheta_p + rho_zz (theta_m' - theta_m)
 *         exner, pressure_p from rtheta_p' by atm_recover_large_step_variables_work's two expressions (MPAS form)
 *         scalars 0, 1, 2
 *       and no other field (rho_zz is not written; scalars 3..7, level nVertLevels and the zero slot keep their
 *       bits).  The increment forms are deliberate: a cell in which no subcycle had a non-zero cond or ern keeps
 *       theta_m, rtheta_p, qv and qc bit for bit and gets rt_diabatic_tend = +0.0.  Contract: rdzw, zz > 0, T > 36,
 *       qv, qc, qr >= 0, x < 4096; any other input leaves the result undefined, but the call still writes only its
 *       own fields.  Statement order: tests/kessler_ref.py (device pow / exp / log against the host's are the only
 *       differences).  A decomposed context runs its owned cells; no gather, the written fields' ghosts go stale.
 *       Per owned cell three accumulators, plain `+=` in call order, one writer each (two runs give the same
 *       bits): 0 the accumulated rain P (mm), 1 the last call's P, 2 the number of calls (as a double).  They are
 *       not registry fields (mpas_field_count is unchanged) and are allocated, zeroed, on first use.
 * mpas_precip_read copies accumulator `which` (0..2) of the owned cells to out (the call synchronises): cell e at
 *       byte offset e*stride_cell.  mpas_precip_reset zeroes all three.
 * Option "microphysics" = 1 (needs "physics" = 2, else MPAS_EINVAL; a value other than 0 or 1: MPAS_EINVAL;
 *       default 0; reset to 0 when "physics" leaves 2) makes mpas_atm_srk3 end every step with the task over the
 *       step's dt: behind the transport, mpas_reconstruct_2d and the substep finish, ahead of a "stats_every"
 *       sample, inside the captured graph, under the timing key "atm_kessler_microphysics".  With 0 the step is
 *       launch for launch the step without the feature.  It does not require "transport" (the driver pairs them).
 *       The dynamics do not yet feel water loading (qtot, cqw, cqu stay atm_compute_moist_coefficients' constants).
 *       "forcing" and "stats_every" combine with it unchanged: their T = theta_m exner is then the virtual
 *       temperature. */
int mpas_atm_kessler_microphysics(mpas_ctx* ctx, double dt);
int mpas_precip_read(mpas_ctx* ctx, int32_t which, double* out, int64_t stride_cell);
int mpas_precip_reset(mpas_ctx* ctx);
/* Surface fluxes and boundary layer (k_pbl.hip): the bulk surface fluxes of momentum, heat and moisture over an
 *       ocean of prescribed temperature and the implicit boundary-layer diffusion of the simple-physics package
 *       of Reed & Jablonowski (2012), the lower boundary the DCMIP-2016 moist cases pair with Kessler.  It is that
 *       scheme on the model's own layers and layer mass instead of pressure thicknesses, and the mixing ratio qv
 *       stands where the source has specific humidity; the package's large-scale condensation is left out
 *       (Kessler's saturation adjustment covers it).  No reference entry point ("physics" = 2, dt > 0 and a
 *       configured surface temperature, else MPAS_EINVAL).  Per owned cell column, levels k = 0..L-1
 *       (L = nVertLevels, 0 the lowest), every input as found:
 *         m = rho_zz / rdzw (Kessler's layer mass);   dz = 1 / (rdzw zz);   rho_d = zz rho_zz
 *         p = pressure_base + pressure_p;   pi = exner, held fixed over the call;   rvord = 461.6 / 287
 *         qv = scalar 0;   theta = theta_m / (1 + rvord qv);   ua = uReconstructZonal;   va = uReconstructMeridional
 *         ps: mpas_atm_held_suarez_forcing's surface-pressure expression, term for term;   Ts: the cell's
 *         configured surface temperature;   za = 0.5 dz(0);   wind = sqrt(ua(0)^2 + va(0)^2)
 *         Cd = wind < 20 ? 7e-4 + 6.5e-5 wind : 2e-3;   Ch = 1.1e-3
 *         qss = 0.622 / ps * 610.78 * exp(-(2.5e6 / 461.5) (1 / Ts - 1 / 273.16))
 *         am = Cd wind dt / za;   ah = Ch wind dt / za
 *       The surface step, implicit, level 0 only (the other levels carry over):
 *         u1(0) = ua(0) / (1 + am);   v1(0) = va(0) / (1 + am)
 *         th1(0) = (theta(0) + ah Ts / pi(0)) / (1 + ah);   q1(0) = (qv(0) + ah qss) / (1 + ah)
 *         E = m(0) (q1(0) - qv(0))   (kg/m2 = mm: the evaporation of the call)
 *       The mixing at the interfaces k = 1..L-1, between levels k-1 and k, with D(0) = D(L) = 0:
 *         s = dz(k) + dz(k-1);   pint = (dz(k) p(k-1) + dz(k-1) p(k)) / s;   rhoi likewise from rho_d;   dzc = 0.5 s
 *         f = pint >= 85000 ? 1 : exp(-((85000 - pint) / 10000)^2)
 *         Dm(k) = rhoi Cd wind za f / dzc;   Dh(k) = the same with Ch
 *       then one implicit flux-form step per quantity, with Dm for u1 and v1 and Dh for th1 and q1:
 *         a(k) = -dt D(k) / m(k);   c(k) = -dt D(k+1) / m(k);   b = 1 - a - c
 *         a(k) X2(k-1) + b(k) X2(k) + c(k) X2(k+1) = X1(k)
 *       solved by the Thomas algorithm level by level in the order tests/pbl_ref.py states (one reciprocal per
 *       level, shared by the two right-hand sides of a system); each step conserves sum_k m X.  Cd and f are
 *       continuous at their switches.  Written, by Kessler's increment forms from th2 and q2:
 *         theta_m' = theta_m + (th2 - theta)(1 + rvord q2) + theta rvord (q2 - qv)
 *         rtheta_p' = rtheta_p + rho_zz (theta_m' - theta_m)
 *         exner, pressure_p from rtheta_p' by atm_recover_large_step_variables_work's two expressions (MPAS form)
 *         scalar 0 = q2 (scalar 1, which shares its 16-byte pair, is stored back as found)
 *       and, per owned edge with cells c1, c2 and A = angleEdge, the momentum change as a tendency:
 *         Fu = rho_zz (u2 - ua) / dt;   Fv = rho_zz (v2 - va) / dt   (per cell, scratch)
 *         tend_ru_physics = 0.5 (Fu(c1) + Fu(c2)) cos A + 0.5 (Fv(c1) + Fv(c2)) sin A
 *       and no other field: rt_diabatic_tend, uReconstructZonal / Meridional and u are not written, scalars 1..7,
 *       level nVertLevels and the zero slot keep their bits.  Momentum goes through tend_ru_physics, as MPAS-A
 *       projects its boundary-layer wind tendencies onto the edges (a direct write of u would leave
 *       solve_diagnostics' ke, pv_edge and v stale); heat and moisture are time-split state updates like Kessler's,
 *       because the transport has no scalar tendency slot.  A column with wind = 0 keeps theta_m, rtheta_p and qv
 *       bit for bit (exner and pressure_p where they satisfy the two expressions as found) and gets
 *       Fu = Fv = +0.0 and E = +0.0; L = 1 is the surface step alone.  exp, sqrt and the exner expression's pow
 *       are the only libm calls.  Statement order: tests/pbl_ref.py.  A decomposed context runs its owned cells
 *       and edges; the edge part gathers Fu, Fv of the ghost cells by an exchange of the scratch.
 *       Per owned cell three accumulators, plain `+=` in call order, one writer each (two runs give the same
 *       bits): 0 the accumulated evaporation E (mm), 1 the last call's E, 2 the number of calls (as a double).
 *       They are not registry fields (mpas_field_count is unchanged) and are allocated, zeroed, on first use.
 * mpas_surface_set_temperature: Ts of the owned cells in kelvin, cell e at byte offset e*stride_cell; a value that
 *       is not finite or not > 0 returns MPAS_EINVAL and leaves the configured temperatures as they were.
 * mpas_surface_flux_read copies accumulator `which` (0..2) of the owned cells to out (the call synchronises): cell
 *       e at byte offset e*stride_cell.  mpas_surface_flux_reset zeroes all three.
 * Option "pbl" = 1 (needs "physics" = 2 and a configured Ts, else MPAS_EINVAL; a value other than 0 or 1:
 *       MPAS_EINVAL; default 0; reset to 0 when "physics" leaves 2) makes mpas_atm_srk3 end every step with the
 *       task over the step's dt: behind mpas_reconstruct_2d, the substep finish and the Kessler task (the DCMIP
 *       order, microphysics then simple physics), ahead of a "stats_every" sample, inside the captured graph,
 *       under the timing key "atm_surface_pbl".  The tendency it leaves is the one the next step's three stages
 *       read; the first step reads what was uploaded.  With 0 the step is launch for launch the step without the
 *       feature.  "pbl" = 1 together with "forcing" = 1 is MPAS_EINVAL in whichever order they are set: both
 *       write tend_ru_physics, and Held-Suarez's Rayleigh layer and this boundary layer are alternatives. */
int mpas_atm_surface_pbl(mpas_ctx* ctx, double dt);
int mpas_surface_set_temperature(mpas_ctx* ctx, const double* ts, int64_t stride_cell);
int mpas_surface_flux_read(mpas_ctx* ctx, int32_t which, double* out, int64_t stride_cell);
int mpas_surface_flux_reset(mpas_ctx* ctx);
/* rk_timestep.rg:29 summarize_timestep(cr, er, config_print_detailed_minmax_vel,
 *       config_print_global_minmax_vel, config_print_global_minmax_sca): the values the
 *       reference prints, into out[31] (host memory; the call synchronises):
 *       out[0..24] five records {value, index, k, lat_deg, lon_deg}: min w, max w, min u,
 *       max u, max wind speed; out[25], out[26] NaN seen in w, u; out[27..30] the
 *       regentlib min/max folds from 0.0 of w and of u.  Blocks whose flag is 0 stay 0
 *       (the reference calls it with every flag false, rk_timestep.rg:492). */
int mpas_summarize_timestep(mpas_ctx* ctx, int config_print_detailed_minmax_vel, int config_print_global_minmax_vel,
                            int config_print_global_minmax_sca, double* out);

/* ---- the driver (rk_timestep.rg:361-500) ---------------------------------------- */
/* schedule 0: the reference's atm_srk3 (Q4: rk_sub_timestep[rk_step] truncated into
 * dyn_tend's rk_step; Q5: n+1 acoustic substeps); schedule 1: dyn_tend rk_step = 0,1,2
 * (the MPAS schedule used by the benchmark). */
int mpas_atm_srk3(mpas_ctx* ctx, double dt, int schedule);
/* rk_timestep.rg:503 atm_timestep = atm_srk3 with the reference schedule */
int mpas_atm_timestep(mpas_ctx* ctx, double dt);

/* ---- horizontal decomposition (rk_timestep.rg runs on Legion partitions) --
 * A context may hold one subdomain: the local entities are its owned ones first, then
 * its ghosts (everything its owned entities reach through an index array), then the
 * zero slot; mpasdyn/decomp.py builds the local state and the plan.  Every task then
 * computes owned entities only, and before each kernel the fields it gathers that an
 * earlier kernel wrote are exchanged on the ghosts (RCCL send/recv per peer, or the
 * in-process loopback).  Every rank must call the same tasks in the same order. */
/* owned counts (the first entities of each kind); default: all local entities */
int mpas_halo_owned(mpas_ctx* ctx, int32_t nCellsOwned, int32_t nEdgesOwned, int32_t nVerticesOwned);
/* the first n*Interior owned entities of each kind reach no ghost through any index array
 * (mpasdyn/decomp.py numbers them first): a kernel whose gathered fields need an exchange
 * then computes them while the exchange runs on the context's halo stream, and the
 * remaining (boundary) owned entities after it (SURVEY §8.6 overlap; option "overlap") */
int mpas_halo_interior(mpas_ctx* ctx, int32_t nCellsInterior, int32_t nEdgesInterior, int32_t nVerticesInterior);
/* ring-1 ghosts (mpasdyn/decomp.py numbers them first among the ghosts): local edges
 * [0, nEdgesRing1) are the owned edges and the ghost edges of owned cells, local vertices
 * [0, nVerticesRing1) the owned vertices and the ghost vertices of owned edges.  With
 * option "ring1" (default 1) atm_divergence_damping_3d (reference semantics) also updates
 * those edges and atm_compute_solve_diagnostics those vertices, from inputs fresh there,
 * so the acoustic step's ru_p and the edge kernels' vorticity / pv_vertex gathers need no
 * halo exchange.  Every rank must make the same call. */
int mpas_halo_ring1(mpas_ctx* ctx, int32_t nEdgesRing1, int32_t nVerticesRing1);
/* kind 0 cells, 1 edges, 2 vertices: columns this rank sends to / receives from `peer`,
 * as local ids, in the order the peer receives / sends them */
int mpas_halo_plan(mpas_ctx* ctx, int kind, int peer, const int32_t* send_ids, int32_t nsend,
                   const int32_t* recv_ids, int32_t nrecv);
/* global id of every local entity of `kind` (n = local count): mpas_fill_synthetic then
 * generates the same values as on the undecomposed mesh */
int mpas_set_global_ids(mpas_ctx* ctx, int kind, const int32_t* gids, int32_t n);
/* transports: RCCL (one process per GPU; rank 0 makes the 128-byte id, the caller
 * broadcasts it) or loopback (n contexts of one process on one device, rank = index,
 * each driven by its own host thread) */
int mpas_rccl_unique_id(void* id128);
/* (after every mpas_halo_plan call of the context: the transports size their buffers) */
int mpas_halo_rccl(mpas_ctx* ctx, int nranks, int rank, const void* id128);
int mpas_halo_loopback(mpas_ctx** ctxs, int n);
/* host-staged TCP transport: nranks processes (they may share one device -- RCCL refuses
 * two ranks on one GPU), rank r listening on host:base_port + r; each exchange copies the
 * packed regions to the host, swaps them with the peers over the sockets and copies them
 * back (synchronous; never captured in a graph).  The multi-process test of the same
 * plan / pack / unpack code the RCCL transport runs (tests/test_gpu_multiproc.py). */
int mpas_halo_socket(mpas_ctx* ctx, int nranks, int rank, const char* host, int base_port);
/* stub transport (measurement only): every exchange packs the send columns of each peer,
 * stands in for the wire with one device copy of the received bytes out of the send
 * buffer, and unpacks -- one rank's whole launch sequence on one GPU, everything but the
 * wire time; the ghosts do NOT receive their neighbours' values */
int mpas_halo_stub(mpas_ctx* ctx);
/* halo exchanges made so far and fields moved by them */
int mpas_halo_stats(mpas_ctx* ctx, int64_t* exchanges, int64_t* fields);

/* ---- instrumentation ------------------------------------------------------------ */
/* With timing on, every task call is bracketed by HIP events on the task stream and its
 * device time accumulated per task name; mpas_timing_get returns calls and total ms. */
int mpas_timing_enable(mpas_ctx* ctx, int on);
int mpas_timing_reset(mpas_ctx* ctx);
int mpas_timing_count(mpas_ctx* ctx);
int mpas_timing_get(mpas_ctx* ctx, int idx, const char** name, int64_t* calls, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif
