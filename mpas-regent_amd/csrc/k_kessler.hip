// k_kessler.hip -- Kessler warm-rain microphysics for gfx950, in the form of the DCMIP-2016 moist test cases
// (Klemp et al. 2015): the first writer of rt_diabatic_tend, the heating dyn_tend adds to tend_theta and the last
// stage's recover takes out again (MPAS-A's time-split coupling), and the first task that reads the transported
// scalars (0, 1, 2 = qv, qc, qr).  No reference task exists; the formulas are stated in include/mpas_dyn.h
// (mpas_atm_kessler_microphysics) and restated in NumPy, in this operand order, by tests/kessler_ref.py.
// Same column mapping as the rest of the library: one wavefront per cell column (LP = 64; 64 / LP columns below
// it), lane = level.  Every input is the cell's own column: no gather, no halo.  A translation unit of its own: no
// kernel of the step is compiled with it.
#include "mpas_dev.h"
#include "mpas_halo.h"

namespace mpas {

// (selects, never fmax / fmin: the restatement's np.where on the same comparison, so -0.0 and the arm taken agree)
__device__ __forceinline__ double kmx(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double kmn(double a, double b) { return a < b ? a : b; }
// the shared logarithm of the powers of y = r qr: -inf for y <= 0, so that every power of it is 0 -- log's own value
// at 0, and no NaN from a rain the transport's limiter left a rounding below zero (the max(., 0) of the subcycle
// then lifts it to 0)
__device__ __forceinline__ double klog(double y) { return y > 0.0 ? log(y) : -__builtin_inf(); }

// One cell column.  Six own columns in three paired 16-B loads and exner_base, the cell's scalar pairs 0 (qv, qc)
// and 1 (qr, scalar 3) in one 16-B load each; level k + 1's flux and level 0's density by lane shuffles inside the
// column's LP lanes.  The subcycle count n is the COLUMN's: x is reduced over the column's LP lanes only, the loop
// runs to the wavefront's largest n (wave-uniform: the shuffles inside it are convergent) and a column past its
// own n keeps its values by selects.  The four powers of r qr and qr^0.875 share one logarithm per evaluation
// point: exp(a log(r qr)), qr^0.875 = exp(0.875 (log(r qr) - log r)); the logarithm of r qr <= 0 is -inf (klog),
// which gives the power 0.  The levels from L up compute on stand-in values and store what they hold (level L of
// a keep field its kept value, the padding zeros, the scalar pairs as loaded): every line whole.
template <int LP>
__global__ __launch_bounds__(256) void k_kessler(DevState S, double dt, double* __restrict__ precip) {
    ColMap<LP> m(S, KC);
    const int L = S.L, k = m.k;
    const bool own = m.ent < S.nCO;  // (no early return: the wavefront's columns meet in the shuffles below)
    const int c = own ? m.ent : S.nCO - 1;
    const bool lv = k < L;
    auto kL = [&](int f) { return keepv<LP>(S, f, KC, c); };
    const double kl_tm = kL(F_theta_m), kl_rtp = kL(F_rtheta_p), kl_ex = kL(F_exner), kl_pp = kL(F_pressure_p);
    const double kl_rtd = kL(F_rt_diabatic_tend);
    double tm, rtp, rz, zz, ex, rtb;
    gather2<LP>(fd(S, F_theta_m), c, fd(S, F_rtheta_p), c, k, tm, rtp);
    gather2<LP>(fd(S, F_rho_zz), c, fd(S, F_zz), c, k, rz, zz);
    gather2<LP>(fd(S, F_exner), c, fd(S, F_rtheta_base), c, k, ex, rtb);
    const double exb = colk(fd(S, F_exner_base), c);
    double2* sc = (double2*)fw(S, F_scalars) + (size_t)(uint32_t)c * (kPairW / 2) * LP + k;
    double2* p0 = (double2*)MPAS_CHK(fd(S, F_scalars), sc, 16);
    double2* p1 = (double2*)MPAS_CHK(fd(S, F_scalars), sc + LP, 16);
    const double2 s01 = *p0, s23 = *p1;
    double rdzw = fd(S, F_rdzw)[k];
    // the levels from L up: stand-ins that keep the arithmetic finite; nothing of them is stored or shuffled in
    if (!lv) tm = 300.0, rz = 1.0, zz = 1.0, ex = 1.0, rdzw = 1.0;
    const double qv0 = lv ? s01.x : 0.0;
    double qv = qv0, qc = lv ? s01.y : 0.0, qr = lv ? s23.x : 0.0;

    const double rvord = kKsRv / kRgas;
    const double rho_d = zz * rz;
    const double ms = rz / rdzw;
    const double dz = 1.0 / (rdzw * zz);
    const double pi = ex;
    const double theta0 = tm / (1.0 + rvord * qv0);
    double theta = theta0;
    const double r = 0.001 * rho_d;
    const double lr = log(r);
    const double pc = 3.8 / (pow(pi, 1.0 / kKsXk) * kKsPsl);
    const double srho = sqrt(__shfl(rho_d, 0, LP) / rho_d);
    const double lcp = kKsLv / (kKsCp * pi);
    const double f5 = 237.3 * kKsF2x * kKsLv / kKsCp;

    double lg = klog(r * qr);
    double vt = 36.34 * exp(0.1364 * lg) * srho;
    double x = lv ? vt * dt / (0.8 * dz) : 0.0;
#pragma unroll
    for (int o = LP / 2; o >= 1; o >>= 1) x = kmx(x, __shfl_xor(x, o, LP));
    // (n <= kKsMaxSub: beyond it only outside the contract; a NaN x gives 1)
    const int n = x > 1.0 ? (x < (double)kKsMaxSub ? (int)ceil(x) : kKsMaxSub) : 1;
    int nw = n;
#pragma unroll
    for (int o = LP; o < 64; o <<= 1) nw = max(nw, __shfl_xor(nw, o, 64));
    nw = __builtin_amdgcn_readfirstlane(nw);
    const double dt0 = dt / (double)n;
    double P = 0.0;
    for (int j = 0; j < nw; j++) {
        const bool act = j < n;
        if (j) {  // (vt from the rain the subcycle before left)
            lg = klog(r * qr);
            vt = 36.34 * exp(0.1364 * lg) * srho;
        }
        const double F = rho_d * qr * vt;
        const double Fu = __shfl_down(F, 1, LP);
        const double Fup = k + 1 < L ? Fu : 0.0;
        const double Pn = P + dt0 * F;
        const double sed = dt0 * (Fup - F) / ms;
        const double q875 = exp(0.875 * (lg - lr));
        const double qrprod = qc - (qc - dt0 * kmx(0.001 * (qc - 0.001), 0.0)) / (1.0 + dt0 * 2.2 * q875);
        const double qc1 = kmx(qc - qrprod, 0.0);
        const double qr1 = kmx(qr + qrprod + sed, 0.0);
        const double T = pi * theta;
        const double qvs = pc * exp(kKsF2x * (T - 273.0) / (T - 36.0));
        const double prod = (qv - qvs) / (1.0 + qvs * f5 / ((T - 36.0) * (T - 36.0)));
        const double lg1 = klog(r * qr1);
        const double e1 = dt0 * ((1.6 + 124.9 * exp(0.2046 * lg1)) * exp(0.525 * lg1) / (2.55e6 * pc / (3.8 * qvs) + 5.4e5)) *
                          kmx(qvs - qv, 0.0) / (r * qvs);
        const double ern = kmn(kmn(e1, kmx(-prod - qc1, 0.0)), qr1);
        const double cond = kmx(prod, -qc1);
        const double th1 = theta + lcp * (cond - ern);
        const double qv1 = kmx(qv - cond + ern, 0.0);
        P = act ? Pn : P;
        theta = act ? th1 : theta;
        qv = act ? qv1 : qv;
        qc = act ? qc1 + cond : qc;
        qr = act ? qr1 - ern : qr;
    }
    const double dth = theta - theta0;
    const double tm1 = tm + dth * (1.0 + rvord * qv) + theta0 * rvord * (qv - qv0);
    const double dtm = tm1 - tm;
    const double rtp1 = rtp + rz * dtm;
    const double ex1 = pow(zz * (kRgas / kP0) * (rtp1 + rtb), kRgas / (kCp - kRgas));
    const double pp1 = zz * kRgas * (ex1 * rtp1 + rtb * (ex1 - exb));
    if (!own) return;
    put2f<LP>(fw(S, F_theta_m), c, fw(S, F_rtheta_p), c, k, KEEPW(tm1, kl_tm), KEEPW(rtp1, kl_rtp));
    put2f<LP>(fw(S, F_exner), c, fw(S, F_pressure_p), c, k, KEEPW(ex1, kl_ex), KEEPW(pp1, kl_pp));
    colk(fw(S, F_rt_diabatic_tend), c) = KEEPW(dtm / dt, kl_rtd);
    *p0 = lv ? make_double2(qv, qc) : s01;
    *p1 = lv ? make_double2(qr, s23.y) : s23;
    if (k == 0) {  // one writer per slot, plain read-add-write in call order: two runs give the same bits
        const size_t nC = (size_t)S.nCells;
        precip[c] += P;
        precip[nC + c] = P;
        precip[2 * nC + c] += 1.0;
    }
}

template <int LP>
static hipError_t kessler_lp(const DevState& S, hipStream_t st, double dt, double* precip) {
    const int ncb = col_blocks<LP>(S, KC);
    if (ncb) k_kessler<LP><<<ncb, 256, 0, st>>>(S, dt, precip);
    // owned cells only, every input the cell's own: no gather; the ghosts of what it wrote are stale
    HALO_WROTE(S, F_theta_m, F_rtheta_p, F_exner, F_pressure_p, F_rt_diabatic_tend, F_scalars);
    return hipGetLastError();
}
hipError_t launch_kessler(const DevState& S, hipStream_t st, double dt, double* precip) {
    if (!precip) return hipErrorInvalidValue;
    MPAS_LP_DISPATCH(S.LP, kessler_lp, S, st, dt, precip);
}

}  // namespace mpas
