// ac_ieks.hpp — batched iterated extended Kalman smoother: Gauss-Newton on the maximum-a-posteriori trajectory of a whole log
// (ac_ieks_pass_f32, ac_ieks_cost_f32, ac_ieks_candidates_f32, ac_ieks_accept_f32, ac_ieks_solve_f32).
// Built on the chart, h and H of ac_ekf.hpp and on [-] of ac_rts.hpp; the backward sweep is ac_ekf_smooth_f32 as it stands.
//
// Nominal Xbar [T+1][13][n]: Xbar[0] is node -1 (the initial node), Xbar[k+1] is filter node k.  Prior (x0, P0).
// MAP cost per instance, J = J_prior + J_proc + J_meas:
//     J_prior = 1/2 e0' P0^-1 e0,  e0 = Xbar[0] [-] x0                   plain Cholesky of P0, one triangular solve
//     J_proc  = 1/2 sum_k sum_j w_kj^2 / Qd_j,  w_k = Xbar[k+1] [-] F(Xbar[k], U_k, dt)     (a row with Qd_j = 0 adds nothing and
//                                                                          sets AC_IEKS_QZERO_DEFECT when w_kj != 0)
//     J_meas  = 1/2 sum_k sum_{used i} (z_ki - h_i(Xbar[k+1]))^2 / Rd_i                     (used: mask bit set and z finite)
// One linearised pass about Xbar: F_k = F(Xbar[k], U_k, dt) and A_k = dF/dx come from ONE sensitivity launch over the T n
// units; k_ieks_filter then runs the whole forward recursion of an affine Kalman filter through those fixed linearisations.
// It carries the deviation d in R^12 about the nominal and P; it starts from d = x0 [-] Xbar[0], P = P0.  Step k:
//     Abar_k = E(F_k) A_k G(Xbar[k])                   the filter's own expression, in the filter's own operation order
//     c_k    = F_k [-] Xbar[k+1]
//     d-     = c_k + Abar_k d,     P- = 1/2 (X + X') + diag(Qd),  X = Abar P Abar'      (ekf_step_group's bits on equal operands)
//     nu_i   = z_i - h_i(Xbar[k+1]) and H AT THE NOMINAL; the fifteen scalar updates in row order with ekf_step_group's
//     recursion and rejection rule, started from d = d-:  rho = nu_i - h_i d
// Records of step k in ac_ekf_filter_rec_f32's shapes: Xs[k] = Xbar[k+1] [+] d_k, Ps[k], Xpreds[k] = Xbar[k+1] [+] d-_k, Ppreds[k],
// Abars[k], nu, S, nis, used, status, and ll summed in step order.  As in the filter, no reset Jacobian and no chart-change
// Jacobian is applied: moving the base point of the deviation from F_k to Xbar[k+1] is the first-order `+ c_k`.  The fixed point
// of the iteration is therefore stationary for J to second order in the deviations only.
// A step is NOT FINITE (AC_EKF_NONFINITE) when Xbar[k], Xbar[k+1], F_k, a row of A_k, d- or P- is not finite.  Then no row is
// applied at that node (used 0, nu, S 0), and the recursion restarts there: d = 0, P = P- if all of P- is finite, else P0; the
// node's records are Xs[k] = Xbar[k+1] bit for bit, Ps[k] = that P; Xpreds, Ppreds, Abars hold what was computed.
//
// Kernels (ieks_inst.hip):
//   k_ieks_filter       one launch for the whole forward recursion; one instance per 16-lane group, sixteen per workgroup
//                       (k_ekf_step's mapping); lane r owns row r of P and Abar; d (in every lane) and P (row r) stay in registers
//                       from step to step; what every lane reads goes through LDS mirrors of row stride 13 (the rows of A_k too:
//                       lane r loads row r, the attitude lanes read rows 6-9 from the mirror).  The operands of step k+1 are
//                       requested as soon as those of step k are consumed (IeksLane::nxt).
//   k_ieks_candidates   one lane per (node, candidate, instance): Xc = Xbar [+] alpha_c (X^s [-] Xbar), column c n + i, and U
//                       replicated beside it.
//   k_ieks_cost_nodes   the nodes are independent given F: the grid runs over (blocks of columns) x (chunks of kIeksChunk
//                       consecutive nodes), workgroup b on chunk b / gb (k_ekf_em_nodes' order); one lane per column, so every
//                       load is a full coalesced row segment.  Per node one float32 process term and one float32 measurement
//                       term (rows in row order), summed in float64 in node order; the chunk's sums go to the workspace.
//   k_ieks_cost_reduce  one lane per column: the chunks in chunk order, J_prior, J rounded to float32 once.
//   k_ieks_accept       one lane per (node, instance): the first candidate with J(alpha) < J(0) is copied into Xbar.
// No atomics, every sum in a fixed order: an instance's bits depend neither on n, on reps nor on where it sits in the batch.
// They do depend on kIeksChunk (where the float64 sums are cut), which is therefore part of the contract.
// The per-lane code is shared with the host build (tests/host_ieks, -DAC_HOST_CHECK), which runs the 16 lanes of a group one
// after the other, phase by phase: a phase reads from the mirrors only what an EARLIER phase wrote.
#pragma once
#include "ac_rts.hpp"

namespace ac {

constexpr int kIeksGroups = kEkfGroups;  // instances per workgroup of k_ieks_filter (four waves)
constexpr int kIeksBlock = 256;          // lanes per workgroup of the candidate, cost and accept kernels
constexpr int kIeksChunk = 32;           // consecutive nodes per float64 partial sum of the cost
constexpr int kIeksMaxCand = 8;          // longest ladder

// status bits of the cost and of the solve, per instance (the pass reports ac_ekf_step_f32's bits per step)
constexpr int AC_IEKS_P0_NOT_PD = 1;      // a pivot of the Cholesky of P0 was <= 0 or not finite: J_prior is meaningless
constexpr int AC_IEKS_NONFINITE = 2;      // a node of the trajectory, an F or J itself is not finite
constexpr int AC_IEKS_QZERO_DEFECT = 4;   // a row with Qd_j = 0 has a defect w_kj != 0 (it adds nothing to J)
constexpr int AC_IEKS_NO_DECREASE = 8;    // no candidate of the ladder lowered J: the nominal was kept

struct IeksLadder {
    float a[kIeksMaxCand];
    int count;
};

// ---- the forward recursion ---------------------------------------------------------------------------------------------------------
// What the launch reads and writes ([T][rows][n] arrays; ll, nu, S, nis, used, status may be NULL).
struct IeksIo {
    const float *X0, *P0;   // [13][n], [12][12][n]: the prior
    const float* Xbar;      // [T+1][13][n]
    const float *F, *A;     // [T][13][n], [T][13][13][n]: the sensitivity launch's outputs on Xbar[0 .. T-1]
    const float *Z, *Qd, *Rd;
    const int* mask;        // [T][n] or NULL (all rows)
    float *Xs, *Ps, *ll, *nu, *S, *nis;
    int *used, *status;
    float *Xpred, *Ppred, *Abar;
    long n, T;
};

// The mirrors of one instance (LDS on the device).
struct IeksShared {
    float m[3][kEkfLanes][kEkfLd];  // P | Abar | the unsymmetrised P-
    float c[2][kEkfLanes];          // P h' of the current row (two in flight)
    float red[kEkfLanes];           // per-lane flags of a reduction: 1 row r of P- is not finite, 2 an operand of lane r is not
    float dm[kEkfLanes];            // d-
    float rd[kEkfLanes];            // Rd
    float z[kEkfLanes];             // z_k
    float nu[kEkfLanes];            // z_k - h(Xbar[k+1])
    float f[kEkfLanes];             // F_k
    float xn[kEkfLanes];            // Xbar[k+1]
    float pad[16];
};
// 784 dwords = 16 mod 32 banks: the two groups of a 32-lane half never share a bank
static_assert(sizeof(IeksShared) / 4 % 32 == 16, "IeksShared: neighbouring groups on disjoint LDS banks");

// What lane r reads of one step.
struct IeksOps {
    float f, xn;          // element r of F_k and of Xbar[k+1] (lanes 13-15: element 0 again)
    float z;              // row r of z_k (lane 15: row 0 again)
    float a[13];          // row r of A_k (lanes 13-15: row 0 again); every lane reads the rows it needs from the mirror
    int mask;
};

// What lane r of a group keeps in registers: the filter's lane (xm is the nominal node) and the step that was loaded ahead.
struct IeksLane {
    EkfLane e;
    IeksOps nxt;
    float q;       // Qd of component r
    float llsum;
    bool opfin, dfin;
};

AC_DI void ieks_load(const IeksIo& io, long k, long i, int r, IeksOps& o) {
    const long n = io.n;
    const float* const f = io.F + (size_t)k * 13 * n;
    const float* const xn = io.Xbar + (size_t)(k + 1) * 13 * n;
    const float* const z = io.Z + (size_t)k * kEkfZ * n;
    const float* const A = io.A + (size_t)k * 169 * n + i;
    const int row = r < 13 ? r : 0;
    o.f = f[row * n + i];
    o.xn = xn[row * n + i];
    o.z = z[(r < kEkfZ ? r : 0) * n + i];
    o.mask = io.mask ? io.mask[(size_t)k * n + i] : 0x7fff;
#pragma unroll
    for (int c = 0; c < 13; ++c) o.a[c] = A[(row * 13 + c) * n];
}

// What was loaded ahead goes into the mirrors: row r of A and of z, element r of F and of the next nominal node (m[2] is free between the last scalar update of a step
// and the next step's X); is the row of A finite?
AC_DI void ieks_stage(IeksLane& L, IeksShared& s, int r) {
    bool fin = true;
    s.z[r] = L.nxt.z;
    s.f[r] = L.nxt.f;
    s.xn[r] = L.nxt.xn;
#pragma unroll
    for (int c = 0; c < 13; ++c) {
        s.m[2][r][c] = L.nxt.a[c];
        fin = fin && ekf_finite(L.nxt.a[c]);
    }
    L.opfin = fin;
}

// The forward recursion of instance i.  G: the group (device: one lane and a barrier after every phase; host: a loop over the
// lanes).  store false: a group past the end of the batch, which stores nothing.
template <class G>
AC_DI void ieks_filter_group(G& grp, IeksShared& s, const ac_ekf_opts& o, float eps, const IeksIo& io, long i, bool store) {
    AC_EKF_FP
    const long n = io.n, T = io.T;
    // ---- d = x0 [-] Xbar[0], row r of P0, the noise; the operands of step 0 ------------------------------------------------------
    grp.each([&](IeksLane& L, int r) AC_EKF_INLINE {
        const int rr = r < kEkfN ? r : 0;
        float x0[13];
#pragma unroll
        for (int c = 0; c < 13; ++c) {
            x0[c] = io.X0[c * n + i];
            L.e.xm[c] = io.Xbar[c * n + i];
        }
        rts_minus(x0, L.e.xm, L.e.d);
#pragma unroll
        for (int j = 0; j < 12; ++j) L.e.p[j] = io.P0[(rr * 12 + j) * n + i];
        s.rd[r] = io.Rd[(r < kEkfZ ? r : 0) * n + i];
        L.q = io.Qd[rr * n + i];
        L.llsum = 0.f;
        ieks_load(io, 0, i, r, L.nxt);
        ieks_stage(L, s, r);
    });
    for (long k = 0; k < T; ++k) {
        // ---- row r of Abar_k = E(F_k) A_k G(Xbar[k]); element r of d- = c_k + Abar_k d; the loads of the next step -----------------
        grp.each([&](IeksLane& L, int r) AC_EKF_INLINE {
            const IeksOps& q = L.nxt;
            float xh[13], f[13], t[13], Gq[4][3];
            bool fin = L.opfin;
#pragma unroll
            for (int c = 0; c < 13; ++c) {
                xh[c] = L.e.xm[c];
                f[c] = s.f[c];
                L.e.xm[c] = s.xn[c];
                fin = fin && ekf_finite(xh[c]) && ekf_finite(f[c]) && ekf_finite(L.e.xm[c]);
            }
            int zf = 0;
#pragma unroll
            for (int c = 0; c < kEkfZ; ++c) zf |= ekf_finite(s.z[c]) ? (1 << c) : 0;
            L.e.usedbits = zf & q.mask & 0x7fff;
            if (r >= 6 && r < 9) {  // an attitude row of E(F_k): four rows of A
                float Eq[3][4], e[4];
                ekf_Eq(f, Eq);
#pragma unroll
                for (int c = 0; c < 4; ++c) e[c] = r == 6 ? Eq[0][c] : r == 7 ? Eq[1][c] : Eq[2][c];
#pragma unroll
                for (int c = 0; c < 13; ++c)
                    t[c] = fmaf(e[0], s.m[2][6][c], fmaf(e[1], s.m[2][7][c], fmaf(e[2], s.m[2][8][c], e[3] * s.m[2][9][c])));
            } else {
                const int row = r < 6 ? r : r < kEkfN ? r + 1 : 0;
#pragma unroll
                for (int c = 0; c < 13; ++c) t[c] = s.m[2][row][c];
            }
            L.opfin = fin;
            ekf_Gq(xh, Gq);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (j < 6) L.e.a[j] = t[j];
                else if (j < 9) L.e.a[j] = fmaf(t[6], Gq[0][j - 6], fmaf(t[7], Gq[1][j - 6], fmaf(t[8], Gq[2][j - 6], t[9] * Gq[3][j - 6])));
                else L.e.a[j] = t[j + 1];
                s.m[0][r][j] = L.e.p[j];
                s.m[1][r][j] = L.e.a[j];
            }
            float c[12], cr = 0.f, acc = 0.f;
            rts_minus(f, L.e.xm, c);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (r == j) cr = c[j];
                acc = fmaf(L.e.a[j], L.e.d[j], acc);
            }
            s.dm[r] = cr + acc;
            L.e.nis = 0.f;
            L.e.ll = 0.f;
            L.e.applied = 0;
            L.e.rejected = false;
            if (k + 1 < T) ieks_load(io, k + 1, i, r, L.nxt);
        });
        // ---- M = Abar P, X = M Abar' --------------------------------------------------------------------------------------------
        grp.each([&](IeksLane& L, int r) AC_EKF_INLINE {
            float mr[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) mr[j] = 0.f;
#pragma unroll
            for (int c = 0; c < 12; ++c)
#pragma unroll
                for (int j = 0; j < 12; ++j) mr[j] = fmaf(L.e.a[c], s.m[0][c][j], mr[j]);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 12; ++c) acc = fmaf(mr[c], s.m[1][j][c], acc);  // Abar[j][c]: column j of Abar'
                L.e.p[j] = acc;
                s.m[2][r][j] = acc;
            }
        });
        // ---- P- = 1/2 (X + X') + diag(Qd); d-; are they finite?; the prediction's records; nu and H at the nominal; P h' of row 0 ---
        grp.each([&](IeksLane& L, int r) AC_EKF_INLINE {
            const int rc = r < kEkfN ? r : 0;
            bool fin = true, dfin = true;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float v = 0.5f * (L.e.p[j] + s.m[2][j][rc]);
                if (j == r) v += L.q;
                L.e.p[j] = v;
                fin = fin && ekf_finite(v);
                L.e.d[j] = s.dm[j];
                dfin = dfin && ekf_finite(L.e.d[j]);
            }
            L.dfin = dfin;
            s.red[r] = ((r < kEkfN && !fin) ? 1.0f : 0.f) + (L.opfin ? 0.f : 2.0f);
            float xp[13];
            ekf_inject(L.e.xm, L.e.d, xp);
            if (store) {
                float* const xo = io.Xpred + (size_t)k * 13 * n;
#pragma unroll
                for (int c = 0; c < 13; ++c)
                    if (r == c) xo[c * n + i] = xp[c];
                if (r < kEkfN) {
                    float* const po = io.Ppred + (size_t)k * 144 * n;
                    float* const ao = io.Abar + (size_t)k * 144 * n;
#pragma unroll
                    for (int j = 0; j < 12; ++j) {
                        po[(r * 12 + j) * n + i] = L.e.p[j];
                        ao[(r * 12 + j) * n + i] = L.e.a[j];
                    }
                }
            }
            EkfMeas m;
            ekf_measure<true>(eps, o.mag_ned, L.e.xm, m);
            float hv = m.h[0];
#pragma unroll
            for (int c = 1; c < kEkfZ; ++c)
                if (r == c) hv = m.h[c];
            s.nu[r] = s.z[r] - hv;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int j = 0; j < 6; ++j) L.e.Ha[c][j] = m.Ha[c][j];
#pragma unroll
                for (int j = 0; j < 3; ++j) L.e.Hm[c][j] = m.Hm[c][j];
            }
            L.e.ph = ekf_hdot(L.e, L.e.p, 0);
            s.c[0][r] = L.e.ph;
        });
        // ---- the fifteen scalar updates, in row order (ekf_step_group's recursion), from d = d- -------------------------------------
#pragma unroll
        for (int z = 0; z < kEkfZ; ++z) {
            grp.each([&](IeksLane& L, int r) AC_EKF_INLINE {
                if (z == 0) {
                    int fl = 0;
#pragma unroll
                    for (int c = 0; c < kEkfLanes; ++c) fl |= (int)s.red[c];
                    L.e.predok = L.dfin && fl == 0;
                    // the restart: d = 0, P = P- if it is finite, else P0
#pragma unroll
                    for (int j = 0; j < 12; ++j) L.e.d[j] = L.e.predok ? L.e.d[j] : 0.f;
                    if (fl & 1) {
                        int rr = r < kEkfN ? r : 0;
                        AC_OPAQUE_V(rr);  // (the addresses of this rare path are formed here, not kept in registers over the loop)
#pragma unroll
                        for (int j = 0; j < 12; ++j) L.e.p[j] = io.P0[(rr * 12 + j) * n + i];
                    }
                }
                float ph[12];
#pragma unroll
                for (int j = 0; j < 12; ++j) ph[j] = s.c[z & 1][j];
                const float sz = s.rd[z] + ekf_hdot(L.e, ph, z);
                const float rho = s.nu[z] - ekf_hdot(L.e, L.e.d, z);
                const bool used = L.e.predok && ((L.e.usedbits >> z) & 1);
                const bool ok = used && sz > 0.f && sz <= kEkfFltMax;
                if (used && !ok) L.e.rejected = true;
                if (ok) {
                    const float w = 1.0f / sz;
                    const float g = rho * w;
#pragma unroll
                    for (int j = 0; j < 12; ++j) {
                        L.e.d[j] = fmaf(ph[j], g, L.e.d[j]);
                        L.e.p[j] = fmaf(-(L.e.ph * ph[j]), w, L.e.p[j]);
                    }
                    const float e = (rho * rho) * w;
                    L.e.nis += e;
                    L.e.ll += logf(sz) + kEkfLog2Pi + e;
                    L.e.applied += 1;
                }
                if (store && r == 0) {
                    if (io.nu) io.nu[((size_t)k * kEkfZ + z) * n + i] = used ? rho : 0.f;
                    if (io.S) io.S[((size_t)k * kEkfZ + z) * n + i] = used ? sz : 0.f;
                }
                if (z + 1 < kEkfZ) {
                    L.e.ph = ekf_hdot(L.e, L.e.p, z + 1);
                    s.c[(z + 1) & 1][r] = L.e.ph;
                } else {
                    // ---- node k: Xbar[k+1] [+] d and the by-products ----------------------------------------------------------------
                    float xo[13];
                    ekf_inject(L.e.xm, L.e.d, xo);
                    const float ll = L.e.applied > 0 ? -0.5f * L.e.ll : 0.f;
                    L.llsum = k > 0 ? L.llsum + ll : ll;
                    if (store) {
                        float* const xs = io.Xs + (size_t)k * 13 * n;
#pragma unroll
                        for (int c = 0; c < 13; ++c)
                            if (r == c) xs[c * n + i] = L.e.predok ? xo[c] : L.e.xm[c];
                        if (r < kEkfN) {
                            float* const ps = io.Ps + (size_t)k * 144 * n;
#pragma unroll
                            for (int j = 0; j < 12; ++j) ps[(r * 12 + j) * n + i] = L.e.p[j];
                        }
                        if (r == 0) {
                            if (io.nis) io.nis[(size_t)k * n + i] = L.e.nis;
                            if (io.used) io.used[(size_t)k * n + i] = L.e.predok ? L.e.usedbits : 0;
                            if (io.status)
                                io.status[(size_t)k * n + i] = (L.e.rejected ? AC_EKF_REJECTED : 0) | (L.e.predok ? 0 : AC_EKF_NONFINITE);
                            if (io.ll && k == T - 1) io.ll[i] = L.llsum;
                        }
                    }
                    if (k + 1 < T) ieks_stage(L, s, r);
                }
            });
        }
    }
}

// ---- the candidates ------------------------------------------------------------------------------------------------------------------
struct IeksCandIo {
    const float *Xbar, *Xs0, *Xs, *U;  // [T+1][13][n], [13][n], [T][13][n], [T][7][n]
    float *Xc, *Uc;                    // [T+1][13][C n], [T][7][C n]
    IeksLadder lad;
    long n, T;
};

// k_ieks_candidates' unit: node k (0 .. T), candidate c, instance i
AC_DI void ieks_candidate_unit(const IeksCandIo& io, long k, int c, long i) {
    AC_EKF_FP
    const long n = io.n, cols = n * io.lad.count, col = (long)c * n + i;
    const float* const xs = k > 0 ? io.Xs + (size_t)(k - 1) * 13 * n : io.Xs0;
    float xb[13], x[13], e[12], xo[13];
#pragma unroll
    for (int r = 0; r < 13; ++r) {
        xb[r] = io.Xbar[((size_t)k * 13 + r) * n + i];
        x[r] = xs[r * n + i];
    }
    rts_minus(x, xb, e);
    const float al = io.lad.a[c];
#pragma unroll
    for (int j = 0; j < 12; ++j) e[j] = al * e[j];
    ekf_inject(xb, e, xo);
#pragma unroll
    for (int r = 0; r < 13; ++r) io.Xc[((size_t)k * 13 + r) * cols + col] = xo[r];
    if (k < io.T) {
#pragma unroll
        for (int r = 0; r < 7; ++r) io.Uc[((size_t)k * 7 + r) * cols + col] = io.U[((size_t)k * 7 + r) * n + i];
    }
}

// ---- the cost ------------------------------------------------------------------------------------------------------------------------
// Columns: reps n trajectories; the data (x0, P0, Z, mask, Qd, Rd) of column c are those of instance c mod n.
struct IeksCostIo {
    const float *X0, *P0;
    const float *Xt, *Ft;     // [T+1][13][cols], [T][13][cols]: the trajectories and F(Xt[k], U[k], dt)
    const float *Z, *Qd, *Rd;
    const int* mask;
    double* part;             // [chunks][2][cols]: process, measurement
    int* pst;                 // [chunks][cols]
    float *J, *Jprior, *Jproc, *Jmeas;  // [cols]; the three terms may be NULL
    int* status;              // [cols]
    float mag[3], eps;
    long n, reps, T;
};

constexpr long ieks_chunks(long T) { return (T + kIeksChunk - 1) / kIeksChunk; }

// k_ieks_cost_nodes' unit: the nodes of chunk ch of column col
AC_DI void ieks_cost_nodes_unit(const IeksCostIo& io, long col, long ch) {
    AC_EKF_FP
    const long n = io.n, cols = n * io.reps, i = col % n;
    const long k0 = ch * kIeksChunk, k1 = k0 + kIeksChunk < io.T ? k0 + kIeksChunk : io.T;
    float qd[12], rd[kEkfZ];
#pragma unroll
    for (int j = 0; j < 12; ++j) qd[j] = io.Qd[j * n + i];
#pragma unroll
    for (int j = 0; j < kEkfZ; ++j) rd[j] = io.Rd[j * n + i];
    double ap = 0.0, am = 0.0;
    int st = 0;
    for (long k = k0; k < k1; ++k) {
        float x[13], f[13], w[12];
        bool fin = true;
#pragma unroll
        for (int r = 0; r < 13; ++r) {
            x[r] = io.Xt[((size_t)(k + 1) * 13 + r) * cols + col];
            f[r] = io.Ft[((size_t)k * 13 + r) * cols + col];
            fin = fin && ekf_finite(x[r]) && ekf_finite(f[r]);
        }
        if (!fin) st |= AC_IEKS_NONFINITE;
        rts_minus(x, f, w);
        float tp = 0.f;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            if (qd[j] > 0.f) tp += (w[j] * w[j]) / qd[j];
            else if (w[j] != 0.f) st |= AC_IEKS_QZERO_DEFECT;
        }
        EkfMeas m;
        ekf_measure<false>(io.eps, io.mag, x, m);
        const int mk = io.mask ? io.mask[(size_t)k * n + i] : 0x7fff;
        float tm = 0.f;
#pragma unroll
        for (int r = 0; r < kEkfZ; ++r) {
            const float z = io.Z[((size_t)k * kEkfZ + r) * n + i];
            if (((mk >> r) & 1) && ekf_finite(z)) {
                const float v = z - m.h[r];
                tm += (v * v) / rd[r];
            }
        }
        ap += (double)tp;
        am += (double)tm;
    }
    io.part[((size_t)ch * 2 + 0) * cols + col] = ap;
    io.part[((size_t)ch * 2 + 1) * cols + col] = am;
    io.pst[(size_t)ch * cols + col] = st;
}

constexpr int ieks_tri(int r, int c) { return r * (r + 1) / 2 + c; }

// k_ieks_cost_reduce's unit: column col over the chunks in chunk order, J_prior, J
AC_DI void ieks_cost_reduce_unit(const IeksCostIo& io, long col) {
    AC_EKF_FP
    const long n = io.n, cols = n * io.reps, i = col % n, chunks = ieks_chunks(io.T);
    double sp = 0.0, sm = 0.0;
    int st = 0;
    for (long c = 0; c < chunks; ++c) {
        sp += io.part[((size_t)c * 2 + 0) * cols + col];
        sm += io.part[((size_t)c * 2 + 1) * cols + col];
        st |= io.pst[(size_t)c * cols + col];
    }
    // J_prior = 1/2 |L^-1 e0|^2 with L L' = P0 (the lower triangle of P0 is read), every sum in index order
    float x0[13], xb[13], e[12], l[78], y[12];
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 13; ++r) {
        x0[r] = io.X0[r * n + i];
        xb[r] = io.Xt[(size_t)r * cols + col];
        fin = fin && ekf_finite(x0[r]) && ekf_finite(xb[r]);
    }
    if (!fin) st |= AC_IEKS_NONFINITE;
    rts_minus(xb, x0, e);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        float d = io.P0[(j * 12 + j) * n + i];
#pragma unroll
        for (int c = 0; c < j; ++c) d = fmaf(-l[ieks_tri(j, c)], l[ieks_tri(j, c)], d);
        if (!(d > 0.f && d <= kEkfFltMax)) {
            bad = true;
            d = 1.0f;
        }
        const float w = 1.0f / sqrtf(d);
        l[ieks_tri(j, j)] = w;  // 1 / L_jj
#pragma unroll
        for (int r = j + 1; r < 12; ++r) {
            float t = io.P0[(r * 12 + j) * n + i];
#pragma unroll
            for (int c = 0; c < j; ++c) t = fmaf(-l[ieks_tri(r, c)], l[ieks_tri(j, c)], t);
            l[ieks_tri(r, j)] = t * w;
        }
    }
    float jp = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        float t = e[j];
#pragma unroll
        for (int c = 0; c < j; ++c) t = fmaf(-l[ieks_tri(j, c)], y[c], t);
        y[j] = t * l[ieks_tri(j, j)];
        jp = fmaf(y[j], y[j], jp);
    }
    jp = 0.5f * jp;
    if (bad) st |= AC_IEKS_P0_NOT_PD;
    const double jproc = 0.5 * sp, jmeas = 0.5 * sm;
    const float J = (float)((double)jp + jproc + jmeas);
    if (!ekf_finite(J)) st |= AC_IEKS_NONFINITE;
    io.J[col] = J;
    if (io.Jprior) io.Jprior[col] = jp;
    if (io.Jproc) io.Jproc[col] = (float)jproc;
    if (io.Jmeas) io.Jmeas[col] = (float)jmeas;
    io.status[col] = st;
}

// ---- the accept decision -------------------------------------------------------------------------------------------------------------
struct IeksAcceptIo {
    const float *Jcur, *Jc;  // [n], [C n]
    const int* stc;          // [C n]: the candidates' cost status
    const float* Xc;         // [T+1][13][C n]
    float *Xbar, *alpha, *Jout;
    int* status;             // [n], in and out: bits are added
    IeksLadder lad;
    long n, T;
};

// k_ieks_accept's unit: node k (0 .. T) of instance i.  The first candidate with J < J(0) and a finite trajectory is taken.
AC_DI void ieks_accept_unit(const IeksAcceptIo& io, long k, long i) {
    const long n = io.n, cols = n * io.lad.count;
    const float j0 = io.Jcur[i];
    int sel = -1;
    for (int c = 0; c < io.lad.count; ++c)
        if (sel < 0 && io.Jc[(size_t)c * n + i] < j0 && !(io.stc[(size_t)c * n + i] & AC_IEKS_NONFINITE)) sel = c;
    if (sel >= 0) {
#pragma unroll
        for (int r = 0; r < 13; ++r) io.Xbar[((size_t)k * 13 + r) * n + i] = io.Xc[((size_t)k * 13 + r) * cols + (size_t)sel * n + i];
    }
    if (k == 0) {
        io.alpha[i] = sel >= 0 ? io.lad.a[sel] : 0.f;
        io.Jout[i] = sel >= 0 ? io.Jc[(size_t)sel * n + i] : j0;
        io.status[i] = io.status[i] | (sel >= 0 ? io.stc[(size_t)sel * n + i] : AC_IEKS_NO_DECREASE);
    }
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launchers (defined in ieks_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; none allocates or
// synchronises.  `grid`, `lds` receive the launch dimension and the static LDS (ac_last_launch).
hipError_t ieks_launch_filter(const ac_ekf_opts& o, float eps, const IeksIo& io, hipStream_t st, int* grid, int* lds);
hipError_t ieks_launch_candidates(const IeksCandIo& io, hipStream_t st, int* grid);
hipError_t ieks_launch_cost(const IeksCostIo& io, hipStream_t st, int* grid);
hipError_t ieks_launch_accept(const IeksAcceptIo& io, hipStream_t st, int* grid);
}  // namespace ac
#endif
