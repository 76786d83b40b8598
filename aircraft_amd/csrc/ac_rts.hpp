// ac_rts.hpp — batched fixed-interval Rauch-Tung-Striebel smoother over the trace of the extended Kalman filter
// (ac_ekf_smooth_f32).  Reads what ac_ekf_filter_rec_f32 records and ac_ekf.hpp defines.
//
// Nodes k = 0 .. T-1 are the filter's steps: node k carries the filtered (x^_k, P_k), the prediction (x-_k, P-_k) and Abar_k,
// which maps the error state of node k-1 to node k; the optional node "-1" is the filter's initial (x0, P0).  Node T-1 is
// copied bit for bit.  Link k = T-1 .. 1 (and 0 with x0, P0) gives node k-1 from node k:
//     L L' = P-_k                                   plain Cholesky, column by column, every sum in index order
//     C_k  = P_{k-1} Abar_k' (P-_k)^-1              row r of C from row r of P_{k-1} Abar_k' by two triangular solves
//     e    = x^s_k [-] x-_k                         (dp, dv, 2 vec(r) / r_w with r = conj(q-) (x) q^s, dw): the inverse of [+]
//     x^s_{k-1} = x^_{k-1} [+] (C_k e)
//     P^s_{k-1} = 1/2 (X + X'),  X = P_{k-1} + (C_k (P^s_k - P-_k)) C_k'                       (symmetric bit for bit)
// As the filter applies no reset Jacobian, P_k is taken as the covariance about x^_k.
// Status of link k: AC_RTS_NONFINITE when an operand (x^_{k-1}, P_{k-1}, x-_k, P-_k, Abar_k, the carried x^s_k, P^s_k) is not
// finite; else AC_RTS_NOT_PD when a pivot of the Cholesky is <= 0 or not finite.  Either way C_k = 0 and node k-1 is the
// filtered (x^_{k-1}, P_{k-1}) bit for bit (no [+] 0), and the recursion goes on from there.
//
// Kernel (rts_inst.hip): k_ekf_smooth, one launch for the whole backward sweep; one instance per 16-lane group, sixteen per
// workgroup (k_ekf_step's mapping); lane r owns row r of P_{k-1}, P-_k, Abar_k, C_k and P^s, and element r of x^_{k-1} and
// x-_k.  x^s (in every lane) and P^s (row r) stay in registers from link to link.  L and what every lane reads go through
// LDS mirrors of row stride 13.  The global loads of link k-1 are issued before the arithmetic of link k (RtsLane::nxt).  No
// atomics, every sum in a fixed order: an instance's bits depend neither on n nor on where it sits in the batch.
// The per-lane code is shared with the host build (tests/host_rts, -DAC_HOST_CHECK), which runs the 16 lanes of a group one
// after the other, phase by phase: a phase reads from the mirrors only what an EARLIER phase wrote.
#pragma once
#include "ac_ekf.hpp"

namespace ac {

constexpr int kRtsGroups = kEkfGroups;  // instances per workgroup of k_ekf_smooth (four waves)

// status bits per link and instance
constexpr int AC_RTS_NOT_PD = 1;     // a pivot of the Cholesky of P-_k was <= 0 or not finite
constexpr int AC_RTS_NONFINITE = 2;  // an operand of the link was not finite

// What the launch reads and writes ([T][rows][n] arrays; X0, P0, Xs0, Ps0 all given or all NULL; Cg may be NULL).
struct RtsIo {
    const float *X0, *P0;                       // [13][n], [12][12][n]: node -1
    const float *Xf, *Pf, *Xpred, *Ppred, *Abar;
    float *Xs, *Ps, *Xs0, *Ps0, *Cg;
    int* status;                                // [T][n]
    long n, T;
};

// The mirrors of one instance (LDS on the device).
struct RtsShared {
    float m[3][kEkfLanes][kEkfLd];  // P-_k, then L below its diagonal, then X | Abar_k, then C_k | P^s_k - P-_k
    float xh[kEkfLanes];            // x^_{k-1}
    float xm[kEkfLanes];            // x-_k
    float d[kEkfLanes];             // C_k e
    float red[kEkfLanes];           // per-lane flags of a reduction
};
// 688 dwords = 16 mod 32 banks: the two groups of a 32-lane half never share a bank
static_assert(sizeof(RtsShared) / 4 % 32 == 16, "RtsShared: neighbouring groups on disjoint LDS banks");

// What lane r reads of one link.
struct RtsRow {
    float p[12], pm[12], a[12];  // row r of P_{k-1}, of P-_k and of Abar_k
    float xh, xm;                // element r of x^_{k-1} and of x-_k (r < 13)
};

// What lane r of a group keeps in registers.  xs, inv, ok are the same in every lane of the group.
struct RtsLane {
    RtsRow cur, nxt;   // the link at work and the one after it (loaded ahead)
    float xs[13];      // x^s_k
    float ps[12];      // row r of P^s_k
    float l[12];       // row r of L
    float inv[12];     // 1 / L_jj
    float mr[12];      // row r of P_{k-1} Abar_k'
    float c[12];       // row r of C_k
    float x[12];       // row r of X
    bool opsok, pivbad, ok;
};

// x [-] xb: the d with xb [+] d = x
AC_DI void rts_minus(const float x[13], const float xb[13], float e[12]) {
    AC_EKF_FP
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        e[i] = x[i] - xb[i];
        e[3 + i] = x[3 + i] - xb[3 + i];
        e[9 + i] = x[10 + i] - xb[10 + i];
    }
    // conj(qb) (x) q: vector part bw a - w b - b x a, scalar part bw w + b . a
    const float bx = xb[6], by = xb[7], bz = xb[8], bw = xb[9];
    const float ax = x[6], ay = x[7], az = x[8], aw = x[9];
    const float rx = fmaf(bw, ax, -(aw * bx)) - fmaf(by, az, -(bz * ay));
    const float ry = fmaf(bw, ay, -(aw * by)) - fmaf(bz, ax, -(bx * az));
    const float rz = fmaf(bw, az, -(aw * bz)) - fmaf(bx, ay, -(by * ax));
    const float rw = fmaf(bw, aw, fmaf(bx, ax, fmaf(by, ay, bz * az)));
    const float two = 2.0f / rw;
    e[6] = two * rx;
    e[7] = two * ry;
    e[8] = two * rz;
}

// The operands of link k for lane r of instance i (link 0 reads node -1 from X0, P0).
AC_DI void rts_load(const RtsIo& io, long k, long i, int r, RtsRow& o) {
    const long n = io.n;
    const int rr = r < kEkfN ? r : 0, rx = r < 13 ? r : 0;
    const float* const xh = k > 0 ? io.Xf + (size_t)(k - 1) * 13 * n : io.X0;
    const float* const ph = k > 0 ? io.Pf + (size_t)(k - 1) * 144 * n : io.P0;
    const float* const xm = io.Xpred + (size_t)k * 13 * n;
    const float* const pm = io.Ppred + (size_t)k * 144 * n;
    const float* const ab = io.Abar + (size_t)k * 144 * n;
    o.xh = xh[rx * n + i];
    o.xm = xm[rx * n + i];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        o.p[j] = ph[(rr * 12 + j) * n + i];
        o.pm[j] = pm[(rr * 12 + j) * n + i];
        o.a[j] = ab[(rr * 12 + j) * n + i];
    }
}

// The backward sweep of instance i.  G: the group (device: one lane and a barrier after every phase; host: a loop over the
// lanes).  store false: a group past the end of the batch, which computes and stores nothing.
template <class G>
AC_DI void rts_sweep_group(G& grp, RtsShared& s, const RtsIo& io, long i, bool store) {
    AC_EKF_FP
    const long n = io.n, T = io.T;
    const long lo = io.X0 ? 0 : 1;  // the last link
    // ---- node T-1: the filtered one, bit for bit; the operands of link T-1 ----------------------------------------------------
    grp.each([&](RtsLane& L, int r) AC_EKF_INLINE {
        const int rr = r < kEkfN ? r : 0;
        const float* const xf = io.Xf + (size_t)(T - 1) * 13 * n;
        const float* const pf = io.Pf + (size_t)(T - 1) * 144 * n;
#pragma unroll
        for (int c = 0; c < 13; ++c) L.xs[c] = xf[c * n + i];
#pragma unroll
        for (int j = 0; j < 12; ++j) L.ps[j] = pf[(rr * 12 + j) * n + i];
        if (T - 1 >= lo) rts_load(io, T - 1, i, r, L.nxt);
        if (store) {
            float* const xo = io.Xs + (size_t)(T - 1) * 13 * n;
            float* const po = io.Ps + (size_t)(T - 1) * 144 * n;
#pragma unroll
            for (int c = 0; c < 13; ++c)
                if (r == c) xo[c * n + i] = L.xs[c];
            if (r < kEkfN) {
#pragma unroll
                for (int j = 0; j < 12; ++j) po[(r * 12 + j) * n + i] = L.ps[j];
            }
            if (!io.X0) {  // no link 0
                if (r == 0) io.status[i] = 0;
                if (io.Cg && r < kEkfN) {
#pragma unroll
                    for (int j = 0; j < 12; ++j) io.Cg[(r * 12 + j) * n + i] = 0.f;
                }
            }
        }
    });
    for (long k = T - 1; k >= lo; --k) {
        // ---- the operands of this link into the mirrors; are they finite?; the loads of the next link ------------------------
        grp.each([&](RtsLane& L, int r) AC_EKF_INLINE {
            L.cur = L.nxt;
            if (k - 1 >= lo) rts_load(io, k - 1, i, r, L.nxt);
            bool fin = ekf_finite(L.cur.xh) && ekf_finite(L.cur.xm);
#pragma unroll
            for (int c = 0; c < 13; ++c) fin = fin && ekf_finite(L.xs[c]);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                fin = fin && ekf_finite(L.cur.p[j]) && ekf_finite(L.cur.pm[j]) && ekf_finite(L.cur.a[j]) && ekf_finite(L.ps[j]);
                const float ch = L.cur.pm[j];  // the matrix that is factored: P-_k
                s.m[0][r][j] = ch;
                s.m[1][r][j] = L.cur.a[j];
                s.m[2][r][j] = L.ps[j] - L.cur.pm[j];
            }
            s.red[r] = fin ? 0.f : 1.0f;
            s.xh[r] = L.cur.xh;
            s.xm[r] = L.cur.xm;
            L.pivbad = false;
        });
        // ---- L L' = P-_k, column by column (ac_group.hpp); with column 0, row r of P_{k-1} Abar_k' -------------------------------------
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            grp.each([&](RtsLane& L, int r) AC_EKF_INLINE {
                if (j == 0) {
                    bool ok = true;
#pragma unroll
                    for (int c = 0; c < kEkfLanes; ++c) ok = ok && s.red[c] == 0.f;
                    L.opsok = ok;
#pragma unroll
                    for (int q = 0; q < 12; ++q) {
                        float acc = 0.f;
#pragma unroll
                        for (int c = 0; c < 12; ++c) acc = fmaf(L.cur.p[c], s.m[1][q][c], acc);  // Abar[q][c]: column q of Abar'
                        L.mr[q] = acc;
                    }
                }
                grp_chol_column(s.m[0], L.l, r, j, L.inv[j], L.pivbad);
            });
        }
        // ---- row r of C_k by two triangular solves; e = x^s_k [-] x-_k; element r of C_k e -----------------------------------------
        grp.each([&](RtsLane& L, int r) AC_EKF_INLINE {
            float y[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float t = L.mr[j];
#pragma unroll
                for (int c = 0; c < j; ++c) t = fmaf(-s.m[0][j][c], y[c], t);
                y[j] = t * L.inv[j];
            }
#pragma unroll
            for (int j = 11; j >= 0; --j) {
                float t = y[j];
#pragma unroll
                for (int c = 11; c > j; --c) t = fmaf(-s.m[0][c][j], L.c[c], t);
                L.c[j] = t * L.inv[j];
            }
            L.ok = L.opsok && !L.pivbad;
            float xm[13], e[12];
#pragma unroll
            for (int c = 0; c < 13; ++c) xm[c] = s.xm[c];
            rts_minus(L.xs, xm, e);
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (!L.ok) L.c[j] = 0.f;
                s.m[1][r][j] = L.c[j];
                acc = fmaf(L.c[j], e[j], acc);
            }
            s.d[r] = acc;
        });
        // ---- row r of X = P_{k-1} + (C_k (P^s_k - P-_k)) C_k'; x^s_{k-1} = x^_{k-1} [+] C_k e -----------------------------------------
        grp.each([&](RtsLane& L, int r) AC_EKF_INLINE {
            float w[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) w[j] = 0.f;
#pragma unroll
            for (int c = 0; c < 12; ++c)
#pragma unroll
                for (int j = 0; j < 12; ++j) w[j] = fmaf(L.c[c], s.m[2][c][j], w[j]);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 12; ++c) acc = fmaf(w[c], s.m[1][j][c], acc);  // C[j][c]: column j of C'
                L.x[j] = L.cur.p[j] + acc;
                s.m[0][r][j] = L.x[j];
            }
            float xh[13], d[12], xo[13];
#pragma unroll
            for (int c = 0; c < 13; ++c) xh[c] = s.xh[c];
#pragma unroll
            for (int j = 0; j < 12; ++j) d[j] = s.d[j];
            ekf_inject(xh, d, xo);
#pragma unroll
            for (int c = 0; c < 13; ++c) L.xs[c] = L.ok ? xo[c] : xh[c];
        });
        // ---- P^s_{k-1} = 1/2 (X + X'); node k-1, C_k and the status of link k ----------------------------------------------------
        grp.each([&](RtsLane& L, int r) AC_EKF_INLINE {
            const int rc = r < kEkfN ? r : 0;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                const float v = 0.5f * (L.x[j] + s.m[0][j][rc]);
                L.ps[j] = L.ok ? v : L.cur.p[j];
            }
            if (store) {
                float* const xo = k > 0 ? io.Xs + (size_t)(k - 1) * 13 * n : io.Xs0;
                float* const po = k > 0 ? io.Ps + (size_t)(k - 1) * 144 * n : io.Ps0;
#pragma unroll
                for (int c = 0; c < 13; ++c)
                    if (r == c) xo[c * n + i] = L.xs[c];
                if (r < kEkfN) {
#pragma unroll
                    for (int j = 0; j < 12; ++j) po[(r * 12 + j) * n + i] = L.ps[j];
                    if (io.Cg) {
                        float* const cg = io.Cg + (size_t)k * 144 * n;
#pragma unroll
                        for (int j = 0; j < 12; ++j) cg[(r * 12 + j) * n + i] = L.c[j];
                    }
                }
                if (r == 0) io.status[(size_t)k * n + i] = L.opsok ? (L.pivbad ? AC_RTS_NOT_PD : 0) : AC_RTS_NONFINITE;
            }
        });
    }
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launcher (defined in rts_inst.hip, which holds the kernel).  Arguments are checked by the ABI unit; it neither allocates
// nor synchronises.  `grid`, `lds` receive the launch dimension and the static LDS (ac_last_launch).
hipError_t rts_launch_smooth(const RtsIo& io, hipStream_t st, int* grid, int* lds);
}  // namespace ac
#endif
