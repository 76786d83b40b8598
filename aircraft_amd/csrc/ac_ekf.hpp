// ac_ekf.hpp — batched extended Kalman filter over the step sensitivities (ac_ekf_step_f32, ac_ekf_filter_f32,
// ac_ekf_measure_f32).
//
// Error state about an estimate x: d = (dp NED, dv NED, dtheta body-frame rotation vector, dw) in R^12, and
//     x [+] d = ( p + dp,  v + dv,  (q (x) (dtheta/2, 1)) / |.|,  w + dw )                    (Hamilton, xyzw)
// the multiplicative chart: no heading singularity and none of the |v|-sized cancelling terms of the steady-flight chart
// (ac_lqr.hpp).  With q = (a, w):
//     G(x) = d(x [+] d)/dd at 0   [13][12]: identity on p, v, w; quaternion rows 1/2 [w I + [a]x ; -a']
//     E(x) = dd/dx                [12][13]: identity on p, v, w; attitude rows 2 [w I - [a]x | -a] / |q|^2
// (E G = I, E annihilates the quaternion-norm direction for any |q|).  Time update from the handle's own step sensitivities
// x- = F(x, u, dt), A = dF/dx:   Abar = E(x-) A G(x),   P- = Abar P Abar' + diag(Qd)   (symmetrised: 1/2 (X + X') bit for bit).
// Measurements h(x) in R^15: 0-2 GPS position p, 3-5 GPS velocity v (NED), 6-8 gyro w, 9-11 air data (V, alpha, beta) exactly
// as aero_pre forms them, 12-14 magnetometer R(q/|q|)' m_ned.  H [15][12] analytic, with R(q dq)' v = v_b + [v_b]x dtheta:
// identity blocks for rows 0-8 (the gyro on columns 9-11), air rows J_air [R' | [v_b]x] on columns 3-8 (J_air = d(V, alpha,
// beta)/d v_r), magnetometer rows [R' m]x on columns 6-8.  nu = z - h(x-) and H are evaluated once, at x-; R = diag(Rd).
// The update is 15 scalar updates in row order over the used rows (mask bit set and z finite):
//     s = h P h' + r,   rho = nu_i - h d,   d += (P h') rho / s,   P -= (P h')(P h')' / s
// (the outer product is rounded before the division: P stays symmetric bit for bit); a used row with s <= 0 or a
// non-finite s is skipped and reported.  Then x+ = x- [+] d (x- itself, bit for bit, when no row was applied).  No reset
// Jacobian is applied to P.
//
// Kernels (ekf_inst.hip):
//   k_ekf_step     one instance per 16-lane group, four per wave (k_lqr_dare's mapping), sixteen per workgroup (a wave alone
//                  uses 16 B of every 64-B sector of the [rows][n] arrays: measured 3.9 x the operand bytes fetched): lane r
//                  owns row r of Abar and P; what every lane reads (P, Abar, P h') goes through LDS mirrors of row stride
//                  13.  No atomics, every sum in a fixed order: an instance's bits depend neither on n nor on where it
//                  sits in the batch.
//   k_ekf_measure  one lane per instance: h(x) -> [15][n]
// The per-lane code is shared with the host build (tests/host_ekf, -DAC_HOST_CHECK), which runs the 16 lanes of a group one
// after the other, phase by phase: a phase reads from the mirrors only what an EARLIER phase wrote.
#pragma once
#include "ac_dynamics.hpp"
#include "ac_group.hpp"  // the group, AC_EKF_FP (it opens every function body of this header), kEkfFltMax

namespace ac {

constexpr int kEkfN = 12;               // error-state coordinates
constexpr int kEkfZ = 15;               // measurement rows
constexpr int kEkfLanes = kGrpLanes;    // lanes of one instance's group (rows 12-15 idle)
constexpr int kEkfLd = kGrpLd;          // row stride of the LDS mirrors
constexpr int kEkfGroups = 16;          // instances per workgroup of k_ekf_step (four waves)
constexpr int kEkfBlock = 256;          // lanes per workgroup of k_ekf_measure
constexpr float kEkfLog2Pi = 1.8378770664093453f;
constexpr long kEkfSensFloats = 13 + 169 + 91;      // x- | A | B per instance (the sensitivity launch's outputs)
constexpr long kEkfChainFloats = 2 * (13 + 144);    // two (x, P) pairs per instance: ac_ekf_filter_f32's ping-pong

// status bits per instance
constexpr int AC_EKF_REJECTED = 1;   // a used row had s <= 0 or a non-finite s and was skipped
constexpr int AC_EKF_NONFINITE = 2;  // the prediction is not finite: the outputs are the prediction, no row was applied

AC_DI bool ekf_finite(float v) { return fabsf(v) <= kEkfFltMax; }  // (false for NaN)

// only epsilon is read (aero_pre)
AC_DI DevParams ekf_params(float eps) {
    DevParams P{};
    P.p.epsilon = eps;
    return P;
}

AC_DI void ekf_skew(const float v[3], float S[3][3]) {
    S[0][0] = 0.f; S[0][1] = -v[2]; S[0][2] = v[1];
    S[1][0] = v[2]; S[1][1] = 0.f; S[1][2] = -v[0];
    S[2][0] = -v[1]; S[2][1] = v[0]; S[2][2] = 0.f;
}

// h(x) and, with JAC, the blocks of H that are not identity: Ha = air rows on columns 3-8, Hm = magnetometer rows on 6-8
struct EkfMeas {
    float h[kEkfZ];
    float Ha[3][6], Hm[3][3];
};

// R(q/|q|)' for any |q| != 0 (NED -> body)
AC_DI void ekf_rot_t(const float x[13], float M[3][3]) {
    AC_EKF_FP
    const float qx = x[6], qy = x[7], qz = x[8], qw = x[9];
    const float s = 2.0f / fmaf(qx, qx, fmaf(qy, qy, fmaf(qz, qz, qw * qw)));
    M[0][0] = 1.0f - s * fmaf(qy, qy, qz * qz); M[0][1] = s * fmaf(qx, qy, qw * qz); M[0][2] = s * fmaf(qx, qz, -(qw * qy));
    M[1][0] = s * fmaf(qx, qy, -(qw * qz)); M[1][1] = 1.0f - s * fmaf(qx, qx, qz * qz); M[1][2] = s * fmaf(qy, qz, qw * qx);
    M[2][0] = s * fmaf(qx, qz, qw * qy); M[2][1] = s * fmaf(qy, qz, -(qw * qx)); M[2][2] = 1.0f - s * fmaf(qx, qx, qy * qy);
}

// The air rows are aero_pre's expressions (ac_dynamics.hpp) with every rounding written out; k_ekf_measure stores aero_pre's own
// values in their place (ekf_measure_unit).
template <bool JAC>
AC_DI void ekf_measure(float eps, const float mag[3], const float x[13], EkfMeas& m) {
    AC_EKF_FP
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        m.h[i] = x[i];
        m.h[3 + i] = x[3 + i];
        m.h[6 + i] = x[10 + i];
    }
    float M[3][3], vb[3], vr[3];
    ekf_rot_t(x, M);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        vb[i] = fmaf(M[i][0], x[3], fmaf(M[i][1], x[4], M[i][2] * x[5]));
        vr[i] = vb[i] + eps;
        m.h[12 + i] = fmaf(M[i][0], mag[0], fmaf(M[i][1], mag[1], M[i][2] * mag[2]));
    }
    // V = sqrt(|v_r|^2 + eps), alpha = atan2(v_r2, v_r0 + eps), beta = asin(v_r1 / V)
    const float cx = vr[0] + eps, cy = vr[1], cz = vr[2];
    const float V = sqrtf(fmaf(vr[0], vr[0], fmaf(vr[1], vr[1], vr[2] * vr[2])) + eps);
    m.h[9] = V;
    m.h[10] = atan2f(cz, cx);
    m.h[11] = asinf(cy / V);
    if (JAC) {
        float Sv[3][3];
        ekf_skew(vb, Sv);
        ekf_skew(m.h + 12, m.Hm);
        // J_air = d(V, alpha, beta)/d v_r
        const float ixz = 1.0f / fmaf(cx, cx, cz * cz);
        const float V2 = V * V;
        const float iV = 1.0f / V;
        const float ib = 1.0f / (V2 * sqrtf(fmaf(-cy, cy, V2)));
        float J[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            J[0][k] = vr[k] * iV;
            J[2][k] = fmaf(-cy, vr[k], k == 1 ? V2 : 0.f) * ib;
        }
        J[1][0] = -(cz * ixz);
        J[1][1] = 0.f;
        J[1][2] = cx * ixz;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                m.Ha[k][c] = fmaf(J[k][0], M[0][c], fmaf(J[k][1], M[1][c], J[k][2] * M[2][c]));
                m.Ha[k][3 + c] = fmaf(J[k][0], Sv[0][c], fmaf(J[k][1], Sv[1][c], J[k][2] * Sv[2][c]));
            }
    }
}

// quaternion rows of G(x): 1/2 [w I + [a]x ; -a']  [4][3]
AC_DI void ekf_Gq(const float x[13], float Gq[4][3]) {
    AC_EKF_FP
    float S[3][3];
    ekf_skew(x + 6, S);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Gq[i][j] = 0.5f * ((i == j ? x[9] : 0.f) + S[i][j]);
        Gq[3][i] = -(0.5f * x[6 + i]);
    }
}

// attitude rows of E(x): 2 [w I - [a]x | -a] / |q|^2  [3][4]
AC_DI void ekf_Eq(const float x[13], float Eq[3][4]) {
    AC_EKF_FP
    float S[3][3];
    ekf_skew(x + 6, S);
    const float n2 = fmaf(x[6], x[6], fmaf(x[7], x[7], fmaf(x[8], x[8], x[9] * x[9])));
    const float two = 2.0f / n2;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Eq[i][j] = two * ((i == j ? x[9] : 0.f) - S[i][j]);
        Eq[i][3] = -(two * x[6 + i]);
    }
}

// x [+] d
AC_DI void ekf_inject(const float x[13], const float d[12], float o[13]) {
    AC_EKF_FP
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[i] = x[i] + d[i];
        o[3 + i] = x[3 + i] + d[3 + i];
        o[10 + i] = x[10 + i] + d[9 + i];
    }
    // q (x) (dtheta/2, 1): vector part w e + a + a x e, scalar part w - a . e
    const float ax = x[6], ay = x[7], az = x[8], aw = x[9];
    const float ex = 0.5f * d[6], ey = 0.5f * d[7], ez = 0.5f * d[8];
    struct { float x, y, z, w; } r;
    r.x = fmaf(aw, ex, ax) + fmaf(ay, ez, -(az * ey));
    r.y = fmaf(aw, ey, ay) + fmaf(az, ex, -(ax * ez));
    r.z = fmaf(aw, ez, az) + fmaf(ax, ey, -(ay * ex));
    r.w = aw - fmaf(ax, ex, fmaf(ay, ey, az * ez));
    const float inv = 1.0f / sqrtf(fmaf(r.x, r.x, fmaf(r.y, r.y, fmaf(r.z, r.z, r.w * r.w))));
    o[6] = r.x * inv;
    o[7] = r.y * inv;
    o[8] = r.z * inv;
    o[9] = r.w * inv;
}

// What one launch reads and writes ([rows][n] arrays; optional pointers may be NULL).
struct EkfIo {
    const float *X, *P;      // [13][n], [12][12][n]: the estimate
    const float *Xp, *A;     // [13][n], [13][13][n]: the sensitivity launch's x- and A (prediction only)
    const float *Z, *Qd, *Rd;
    const int* mask;         // [n] or NULL (all rows)
    const float* ll_in;      // [n] or NULL: added to this step's log-likelihood
    float *Xo, *Po;
    float *nu, *S, *nis, *ll;
    int *used, *status;
    float *Xpred, *Ppred, *Abar;
    long n;
};

// The mirrors of one instance (LDS on the device).
struct EkfShared {
    float m[3][kEkfLanes][kEkfLd];  // P | Abar | the unsymmetrised P-
    float c[2][kEkfLanes];          // P h' of the current row (two in flight)
    float red[kEkfLanes];           // per-lane flags of a reduction
    float pad[16];                  // 688 dwords = 16 mod 32 banks: the two groups of a 32-lane half never share a bank
};
static_assert(sizeof(EkfShared) / 4 % 32 == 16, "EkfShared: neighbouring groups on disjoint LDS banks");

// What lane r of a group keeps in registers.  Everything but p, a, ph is the same in every lane of the group.
struct EkfLane {
    float p[12], a[12];   // row r of P and of Abar
    float d[12];          // the error-state correction so far
    float xm[13];         // x-
    float nu[kEkfZ], rd[kEkfZ];
    float Ha[3][6], Hm[3][3];
    float ph, nis, ll;
    int usedbits, applied;
    bool xfin, predok, rejected;
};

// row i of H times a 12-vector
AC_DI float ekf_hdot(const EkfLane& L, const float v[12], int i) {
    AC_EKF_FP
    if (i < 6) return v[i];
    if (i < 9) return v[i + 3];
    if (i < 12) {
        const float* h = L.Ha[i - 9];
        return fmaf(h[0], v[3], fmaf(h[1], v[4], fmaf(h[2], v[5], fmaf(h[3], v[6], fmaf(h[4], v[7], h[5] * v[8])))));
    }
    const float* h = L.Hm[i - 12];
    return fmaf(h[0], v[6], fmaf(h[1], v[7], h[2] * v[8]));
}

// One filter step of instance i.  G: the group (device: one lane and a barrier after every phase; host: a loop over the
// lanes).  PREDICT false: the measurement update alone (Abar = I, Qd not read, x- = x).
template <bool PREDICT, class G>
AC_DI void ekf_step_group(G& grp, EkfShared& s, const ac_ekf_opts& o, float eps, const EkfIo& io, long i, bool store) {
    AC_EKF_FP
    const long n = io.n;
    // ---- x-, nu, H, row r of P and of Abar = E(x-) A G(x) ---------------------------------------------------------------------
    grp.each([&](EkfLane& L, int r) AC_EKF_INLINE {
        const int rr = r < kEkfN ? r : 0;
        float xh[13];
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 13; ++k) {
            xh[k] = io.X[k * n + i];
            L.xm[k] = PREDICT ? io.Xp[k * n + i] : xh[k];
            fin = fin && ekf_finite(L.xm[k]);
        }
        L.xfin = fin;
        EkfMeas m;
        ekf_measure<true>(eps, o.mag_ned, L.xm, m);
        int zf = 0;
#pragma unroll
        for (int k = 0; k < kEkfZ; ++k) {
            const float z = io.Z[k * n + i];
            zf |= ekf_finite(z) ? (1 << k) : 0;
            L.nu[k] = z - m.h[k];
            L.rd[k] = io.Rd[k * n + i];
        }
        L.usedbits = zf & (io.mask ? io.mask[i] : 0x7fff) & 0x7fff;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int c = 0; c < 6; ++c) L.Ha[k][c] = m.Ha[k][c];
#pragma unroll
            for (int c = 0; c < 3; ++c) L.Hm[k][c] = m.Hm[k][c];
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            L.p[j] = io.P[(rr * 12 + j) * n + i];
            L.d[j] = 0.f;
        }
        L.nis = 0.f;
        L.ll = 0.f;
        L.applied = 0;
        L.rejected = false;
        if (PREDICT) {
            float t[13], Gq[4][3];
            const float* A = io.A + i;
            if (r >= 6 && r < 9) {  // an attitude row of E(x-): four rows of A
                float Eq[3][4], e[4];
                ekf_Eq(L.xm, Eq);
#pragma unroll
                for (int c = 0; c < 4; ++c) e[c] = r == 6 ? Eq[0][c] : r == 7 ? Eq[1][c] : Eq[2][c];
#pragma unroll
                for (int c = 0; c < 13; ++c)
                    t[c] = fmaf(e[0], A[(6 * 13 + c) * n], fmaf(e[1], A[(7 * 13 + c) * n], fmaf(e[2], A[(8 * 13 + c) * n], e[3] * A[(9 * 13 + c) * n])));
            } else {
                const int row = r < 6 ? r : r < kEkfN ? r + 1 : 0;
#pragma unroll
                for (int c = 0; c < 13; ++c) t[c] = A[(row * 13 + c) * n];
            }
            ekf_Gq(xh, Gq);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (j < 6) L.a[j] = t[j];
                else if (j < 9) L.a[j] = fmaf(t[6], Gq[0][j - 6], fmaf(t[7], Gq[1][j - 6], fmaf(t[8], Gq[2][j - 6], t[9] * Gq[3][j - 6])));
                else L.a[j] = t[j + 1];
                s.m[0][r][j] = L.p[j];
                s.m[1][r][j] = L.a[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 12; ++j) s.m[2][r][j] = L.p[j];
        }
    });
    // ---- M = Abar P, X = M Abar' ---------------------------------------------------------------------------------------------
    if (PREDICT) {
        grp.each([&](EkfLane& L, int r) AC_EKF_INLINE {
            float mr[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) mr[j] = 0.f;
#pragma unroll
            for (int k = 0; k < 12; ++k)
#pragma unroll
                for (int j = 0; j < 12; ++j) mr[j] = fmaf(L.a[k], s.m[0][k][j], mr[j]);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 12; ++k) acc = fmaf(mr[k], s.m[1][j][k], acc);  // Abar[j][k]: column j of Abar'
                L.p[j] = acc;
                s.m[2][r][j] = acc;
            }
        });
    }
    // ---- P- = 1/2 (X + X') + diag(Qd); is the prediction finite?; P h' of row 0 ------------------------------------------------
    grp.each([&](EkfLane& L, int r) AC_EKF_INLINE {
        const int rc = r < kEkfN ? r : 0;
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            float v = 0.5f * (L.p[j] + s.m[2][j][rc]);
            if (PREDICT && j == r) v += io.Qd[j * n + i];
            L.p[j] = v;
            fin = fin && ekf_finite(v);
        }
        s.red[r] = (r < kEkfN && !fin) ? 1.0f : 0.f;
        if (store && r < kEkfN) {
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (io.Ppred) io.Ppred[(r * 12 + j) * n + i] = L.p[j];
                if (io.Abar) io.Abar[(r * 12 + j) * n + i] = PREDICT ? L.a[j] : (j == r ? 1.0f : 0.f);
            }
        }
        if (store && r == 0 && io.Xpred) {
#pragma unroll
            for (int k = 0; k < 13; ++k) io.Xpred[k * n + i] = L.xm[k];
        }
        L.ph = ekf_hdot(L, L.p, 0);
        s.c[0][r] = L.ph;
    });
    // ---- the fifteen scalar updates, in row order --------------------------------------------------------------------------------
#pragma unroll
    for (int z = 0; z < kEkfZ; ++z) {
        grp.each([&](EkfLane& L, int r) AC_EKF_INLINE {
            if (z == 0) {
                bool ok = L.xfin;
#pragma unroll
                for (int k = 0; k < kEkfN; ++k) ok = ok && s.red[k] == 0.f;
                L.predok = ok;
            }
            float ph[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) ph[j] = s.c[z & 1][j];
            const float sz = L.rd[z] + ekf_hdot(L, ph, z);
            const float rho = L.nu[z] - ekf_hdot(L, L.d, z);
            const bool used = L.predok && ((L.usedbits >> z) & 1);
            const bool ok = used && sz > 0.f && sz <= kEkfFltMax;
            if (used && !ok) L.rejected = true;
            if (ok) {
                const float w = 1.0f / sz;
                const float g = rho * w;
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    L.d[j] = fmaf(ph[j], g, L.d[j]);
                    L.p[j] = fmaf(-(L.ph * ph[j]), w, L.p[j]);
                }
                const float e = (rho * rho) * w;
                L.nis += e;
                L.ll += logf(sz) + kEkfLog2Pi + e;
                L.applied += 1;
            }
            if (store && r == 0) {
                if (io.nu) io.nu[z * n + i] = used ? rho : 0.f;
                if (io.S) io.S[z * n + i] = used ? sz : 0.f;
            }
            if (z + 1 < kEkfZ) {
                L.ph = ekf_hdot(L, L.p, z + 1);
                s.c[(z + 1) & 1][r] = L.ph;
            } else {
                // ---- x+ = x- [+] d and the by-products ------------------------------------------------------------------------
                float xo[13];
                ekf_inject(L.xm, L.d, xo);
                const bool moved = L.applied > 0;
                if (store && r < kEkfN) {
#pragma unroll
                    for (int j = 0; j < 12; ++j) io.Po[(r * 12 + j) * n + i] = L.p[j];
                }
                if (store) {
#pragma unroll
                    for (int k = 0; k < 13; ++k)
                        if (r == k) io.Xo[k * n + i] = moved ? xo[k] : L.xm[k];
                }
                if (store && r == 0) {
                    if (io.nis) io.nis[i] = L.nis;
                    const float ll = moved ? -0.5f * L.ll : 0.f;
                    if (io.ll) io.ll[i] = io.ll_in ? io.ll_in[i] + ll : ll;
                    if (io.used) io.used[i] = L.predok ? L.usedbits : 0;
                    if (io.status) io.status[i] = (L.rejected ? AC_EKF_REJECTED : 0) | (L.predok ? 0 : AC_EKF_NONFINITE);
                }
            }
        });
    }
}

// k_ekf_measure's unit
AC_DI void ekf_measure_unit(const ac_ekf_opts& o, float eps, const float* X, long n, long i, float* Z) {
    const DevParams P = ekf_params(eps);
    float x[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) x[k] = X[k * n + i];
    EkfMeas m;
    ekf_measure<false>(eps, o.mag_ned, x, m);
    AeroPre<float> a;
    aero_pre(P, x, a);  // the forward kernels' own expressions: rows 9-11 are ac_aero_f32's rows 3-5 bit for bit
    m.h[9] = a.V;
    m.h[10] = a.alpha;
    m.h[11] = a.beta;
#pragma unroll
    for (int k = 0; k < kEkfZ; ++k) Z[k * n + i] = m.h[k];
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launchers (defined in ekf_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; none allocates or
// synchronises.  `grid` receives the launch dimension (ac_last_launch).
hipError_t ekf_launch_step(const ac_ekf_opts& o, float eps, const EkfIo& io, hipStream_t st, int* grid, int* lds);
hipError_t ekf_launch_measure(const ac_ekf_opts& o, float eps, const float* X, long n, float* Z, hipStream_t st, int* grid);
}  // namespace ac
#endif
