// ac_em.hpp — batched EM statistics for the noise variances of the extended Kalman filter (ac_ekf_em_f32).
// Reads the records of ac_ekf_filter_rec_f32 and the smoothed trace of ac_ekf_smooth_f32; ac_ekf.hpp defines the chart and h.
//
// Per instance, with diagonal Q and R (the Qd, Rd the records were made with), over the nodes k = 0 .. T-1:
//   process noise, innovations form.  The filter is linear in the error state, d_k = Abar_k d_{k-1} + w_k with Var d_k = P-_k and
//   Cov(w_k, d_k) = Q, and given d_k the noise w_k is independent of the data from k on.  With e = x^s_k [-] x-_k (rts_minus's [-]):
//       E[w_k w_k' | all data] = Q + G (e e' - (P-_k - P^s_k)) G',   G = Q (P-_k)^-1
//   whose diagonal is  t_kj = Q_j + Q_j^2 (y_j^2 - W_jj),  y = (P-_k)^-1 e,  W = (P-_k)^-1 (P-_k - P^s_k) (P-_k)^-1;
//       Qsum_j = sum_k t_kj over the counted nodes, nq their number.
//   (It equals m m' + P^s_k - Abar C_k P^s_k - P^s_k C_k' Abar' + Abar P^s_{k-1} Abar' with m = e - Abar_k C_k e, as I - Abar_k C_k =
//   Q (P-_k)^-1; this form reads neither C, Abar nor node k-1 and keeps the small variances 30 x more accurate in float32.)
//   sensor noise, relinearised at the smoothed state.  For every node and row i whose `used` bit is set and whose z is finite:
//       Rsum_i += (z_i - h_i(x^s_k))^2 + h_i P^s_k h_i',   nr_i += 1         (h, H: ekf_measure's, at x^s_k)
// Status of node k: AC_EM_NONFINITE when an operand (x-_k, P-_k, x^s_k, P^s_k, Qd) is not finite: the node adds nothing; else
// AC_EM_NOT_PD when a pivot of the plain Cholesky of P-_k is <= 0 or not finite: the node adds nothing to Q, its R terms count.
//
// Kernels (em_inst.hip):
//   k_ekf_em_nodes   the nodes are independent, so the grid runs over (groups of 16 instances) x (chunks of kEmChunk consecutive
//                    nodes).  One instance per 16-lane group, sixteen per workgroup (k_ekf_step's mapping); lane r owns row r of
//                    P-_k and P^s_k.  Per node: the operands into LDS mirrors of row stride 13 (the next node is loaded ahead),
//                    the twelve Cholesky columns, then lane j solves P- g = e_j (row j of the inverse) and forms y_j = g . e and
//                    W_jj = g' D g, and lane i < 15 forms h_i(x^s), the row h_i and h_i P^s h_i'.  The per-node terms are float32;
//                    each lane keeps two float64 accumulators (Q component r, R row r) and the counts, summed in node order.
//                    The chunk's partial sums go to the workspace: [chunk][27][n] float64 and [chunk][16][n] int32 (rows 0-14
//                    nr, row 15 nq).
//   k_ekf_em_reduce  one lane per (row, instance): the chunks in chunk order, rounded to float32 once; the counts; Qn, Rn.
// No atomics, every sum in a fixed order: an instance's bits depend neither on n nor on where it sits in the batch.  They do
// depend on kEmChunk (where the float64 partial sums are cut), which is therefore part of the contract.
// The per-lane code is shared with the host build (tests/host_em, -DAC_HOST_CHECK), which runs the 16 lanes of a group one
// after the other, phase by phase: a phase reads from the mirrors only what an EARLIER phase wrote.
#pragma once
#include "ac_rts.hpp"

namespace ac {

constexpr int kEmChunk = 32;            // consecutive nodes per workgroup of k_ekf_em_nodes
constexpr int kEmGroups = kEkfGroups;   // instances per workgroup of k_ekf_em_nodes (four waves)
constexpr int kEmRows = kEkfN + kEkfZ;  // partial sums per chunk and instance: 12 of Q, then 15 of R
constexpr int kEmCounts = 16;           // counts per chunk and instance: nr of the 15 rows, then nq
constexpr int kEmBlock = 256;           // lanes per workgroup of k_ekf_em_reduce
constexpr float kEmFloorRel = 1.0e-4f;  // floor_rel == 0

// status values per node and instance
constexpr int AC_EM_NOT_PD = 1;     // a pivot of the Cholesky of P-_k was <= 0 or not finite: no Q term
constexpr int AC_EM_NONFINITE = 2;  // an operand of the node was not finite: no term at all

// What the launches read and write ([T][rows][n] arrays; Qn, Rn may be NULL).
struct EmIo {
    const float *Xpred, *Ppred, *Xs, *Ps, *Z;
    const int* used;          // [T][n]
    const float *Qd, *Rd;     // [12][n], [15][n]
    double* part;             // [chunks][27][n]
    int* cnt;                 // [chunks][16][n]
    float *Qsum, *Rsum;       // [12][n], [15][n]
    int *nq, *nr, *status;    // [n], [15][n], [T][n]
    float *Qn, *Rn;
    float mag[3], eps, floor_rel;
    long n, T;
};

constexpr long em_chunks(long T) { return (T + kEmChunk - 1) / kEmChunk; }

// The mirrors of one instance (LDS on the device).
struct EmShared {
    float m[3][kEkfLanes][kEkfLd];  // P-_k, then L below its diagonal | D = P-_k - P^s_k | P^s_k
    float xs[kEkfLanes];            // x^s_k
    float xm[kEkfLanes];            // x-_k
    float red[kEkfLanes];           // per-lane flags of a reduction
    float pad[16];                  // 688 dwords = 16 mod 32 banks: the two groups of a 32-lane half never share a bank
};
static_assert(sizeof(EmShared) / 4 % 32 == 16, "EmShared: neighbouring groups on disjoint LDS banks");
static_assert(kEmGroups * sizeof(EmShared) <= 48 * 1024, "EmShared: the smoother's LDS budget");

// What lane r reads of one node.
struct EmRow {
    float pm[12], ps[12];  // row r of P-_k and of P^s_k
    float xm, xs, z;       // element r of x-_k and of x^s_k (r < 13), of z_k (r < 15)
    int used;
};

// What lane r of a group keeps in registers.  l, inv, opsok, pivbad, nqc are the same in every lane of the group.
struct EmLane {
    EmRow cur, nxt;    // the node at work and the one after it (loaded ahead)
    float l[12];       // row r of L
    float inv[12];     // 1 / L_jj
    float q;           // Qd of component r
    double accq, accr; // the chunk's sums: Q component r, R row r
    int nqc, nrc;
    bool opsok, pivbad;
};

// The operands of node k for lane r of instance i.
AC_DI void em_load(const EmIo& io, long k, long i, int r, EmRow& o) {
    const long n = io.n;
    const int rr = r < kEkfN ? r : 0, rx = r < 13 ? r : 0, rz = r < kEkfZ ? r : 0;
    const float* const pm = io.Ppred + (size_t)k * 144 * n;
    const float* const ps = io.Ps + (size_t)k * 144 * n;
    o.xm = io.Xpred[((size_t)k * 13 + rx) * n + i];
    o.xs = io.Xs[((size_t)k * 13 + rx) * n + i];
    o.z = io.Z[((size_t)k * kEkfZ + rz) * n + i];
    o.used = io.used[(size_t)k * n + i];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        o.pm[j] = pm[(rr * 12 + j) * n + i];
        o.ps[j] = ps[(rr * 12 + j) * n + i];
    }
}

// The nodes of chunk c of instance i.  G: the group (device: one lane and a barrier after every phase; host: a loop over the
// lanes).  store false: a group past the end of the batch, which computes and stores nothing.
template <class G>
AC_DI void em_nodes_group(G& grp, EmShared& s, const EmIo& io, long i, long c, bool store) {
    AC_EKF_FP
    const long n = io.n;
    const long k0 = c * kEmChunk, k1 = k0 + kEmChunk < io.T ? k0 + kEmChunk : io.T;
    grp.each([&](EmLane& L, int r) AC_EKF_INLINE {
        L.q = io.Qd[(r < kEkfN ? r : 0) * n + i];
        L.accq = 0.0;
        L.accr = 0.0;
        L.nqc = 0;
        L.nrc = 0;
        em_load(io, k0, i, r, L.nxt);
    });
    for (long k = k0; k < k1; ++k) {
        // ---- the operands of this node into the mirrors; are they finite?; the loads of the next node ------------------------
        grp.each([&](EmLane& L, int r) AC_EKF_INLINE {
            L.cur = L.nxt;
            if (k + 1 < k1) em_load(io, k + 1, i, r, L.nxt);
            bool fin = ekf_finite(L.cur.xm) && ekf_finite(L.cur.xs) && ekf_finite(L.q);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                fin = fin && ekf_finite(L.cur.pm[j]) && ekf_finite(L.cur.ps[j]);
                const float ch = L.cur.pm[j];  // the matrix that is factored: P-_k
                s.m[0][r][j] = ch;
                s.m[1][r][j] = L.cur.pm[j] - L.cur.ps[j];
                s.m[2][r][j] = L.cur.ps[j];
            }
            s.red[r] = fin ? 0.f : 1.0f;
            s.xs[r] = L.cur.xs;
            s.xm[r] = L.cur.xm;
            L.pivbad = false;
        });
        // ---- L L' = P-_k, column by column (ac_group.hpp) ------------------------------------------------------------------------
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            grp.each([&](EmLane& L, int r) AC_EKF_INLINE {
                if (j == 0) {
                    bool ok = true;
#pragma unroll
                    for (int q = 0; q < kEkfLanes; ++q) ok = ok && s.red[q] == 0.f;
                    L.opsok = ok;
                }
                grp_chol_column(s.m[0], L.l, r, j, L.inv[j], L.pivbad);
            });
        }
        // ---- lane j: row j of (P-_k)^-1 by two triangular solves, y_j, W_jj, t_kj; lane i: h_i(x^s), h_i, h_i P^s h_i' ---------------
        grp.each([&](EmLane& L, int r) AC_EKF_INLINE {
            float y[12], g[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float t = r == j ? 1.0f : 0.f;
#pragma unroll
                for (int q = 0; q < j; ++q) t = fmaf(-s.m[0][j][q], y[q], t);
                y[j] = t * L.inv[j];
            }
#pragma unroll
            for (int j = 11; j >= 0; --j) {
                float t = y[j];
#pragma unroll
                for (int q = 11; q > j; --q) t = fmaf(-s.m[0][q][j], g[q], t);
                g[j] = t * L.inv[j];
            }
            float xs[13], xm[13], e[12];
#pragma unroll
            for (int q = 0; q < 13; ++q) {
                xs[q] = s.xs[q];
                xm[q] = s.xm[q];
            }
            rts_minus(xs, xm, e);
            float yj = 0.f, wjj = 0.f;
#pragma unroll
            for (int q = 0; q < 12; ++q) yj = fmaf(g[q], e[q], yj);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < 12; ++q) acc = fmaf(g[q], s.m[1][q][j], acc);  // (g' D)_j
                wjj = fmaf(acc, g[j], wjj);
            }
            const float q2 = L.q * L.q;
            const float tq = fmaf(q2, fmaf(yj, yj, -wjj), L.q);
            const int status = L.opsok ? (L.pivbad ? AC_EM_NOT_PD : 0) : AC_EM_NONFINITE;
            if (status == 0) {
                L.accq += (double)tq;
                L.nqc += 1;
            }
            // the sensor rows, relinearised at x^s_k
            EkfMeas m;
            ekf_measure<true>(io.eps, io.mag, xs, m);
            float hr[12], hv = 0.f;
#pragma unroll
            for (int j = 0; j < 12; ++j) hr[j] = 0.f;
#pragma unroll
            for (int z = 0; z < kEkfZ; ++z) {
                if (r == z) {
                    hv = m.h[z];
                    if (z < 6) hr[z] = 1.0f;
                    else if (z < 9) hr[z + 3] = 1.0f;
                    else if (z < 12) {
#pragma unroll
                        for (int q = 0; q < 6; ++q) hr[3 + q] = m.Ha[z >= 9 && z < 12 ? z - 9 : 0][q];
                    } else {
#pragma unroll
                        for (int q = 0; q < 3; ++q) hr[6 + q] = m.Hm[z >= 12 ? z - 12 : 0][q];
                    }
                }
            }
            float hph = 0.f;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < 12; ++q) acc = fmaf(hr[q], s.m[2][q][j], acc);  // (h_i P^s)_j
                hph = fmaf(acc, hr[j], hph);
            }
            const float res = L.cur.z - hv;
            const float tr = fmaf(res, res, hph);
            if (status != AC_EM_NONFINITE && r < kEkfZ && ((L.cur.used >> r) & 1) && ekf_finite(L.cur.z)) {
                L.accr += (double)tr;
                L.nrc += 1;
            }
            if (store && r == 0) io.status[(size_t)k * n + i] = status;
        });
    }
    // ---- the chunk's partial sums and counts --------------------------------------------------------------------------------------
    grp.each([&](EmLane& L, int r) AC_EKF_INLINE {
        if (!store) return;
        double* const part = io.part + (size_t)c * kEmRows * n;
        int* const cnt = io.cnt + (size_t)c * kEmCounts * n;
        if (r < kEkfN) part[r * n + i] = L.accq;
        if (r < kEkfZ) part[(kEkfN + r) * n + i] = L.accr;
        cnt[r * n + i] = r < kEkfZ ? L.nrc : L.nqc;
    });
}

// k_ekf_em_reduce's unit: row `row` (0-11 of Q, 12-26 of R) of instance i over the chunks, in chunk order.
AC_DI void em_reduce_unit(const EmIo& io, int row, long i) {
    AC_EKF_FP
    const long n = io.n, chunks = em_chunks(io.T);
    const bool isq = row < kEkfN;
    const int zr = row - kEkfN;
    double sum = 0.0;
    int count = 0;
    for (long c = 0; c < chunks; ++c) {
        sum += io.part[((size_t)c * kEmRows + row) * n + i];
        count += io.cnt[((size_t)c * kEmCounts + (isq ? kEmCounts - 1 : zr)) * n + i];
    }
    const float in = isq ? io.Qd[row * n + i] : io.Rd[zr * n + i];
    if (isq) {
        io.Qsum[row * n + i] = (float)sum;
        if (row == 0) io.nq[i] = count;
    } else {
        io.Rsum[zr * n + i] = (float)sum;
        io.nr[zr * n + i] = count;
    }
    float* const out = isq ? io.Qn : io.Rn;
    if (out) {
        float v = in;  // the input bit for bit where nothing was counted
        if (count > 0) {
            const float mean = (float)(sum / (double)count);
            const float fl = (io.floor_rel > 0.f ? io.floor_rel : kEmFloorRel) * in;
            v = mean > fl ? mean : fl;
        }
        out[(isq ? row : zr) * n + i] = v;
    }
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launcher (defined in em_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; it neither allocates
// nor synchronises.  `grid`, `lds` receive the launch dimension and the static LDS of k_ekf_em_nodes (ac_last_launch).
hipError_t em_launch(const EmIo& io, hipStream_t st, int* grid, int* lds);
}  // namespace ac
#endif
