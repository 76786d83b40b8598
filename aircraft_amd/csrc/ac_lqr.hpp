// ac_lqr.hpp — batched LQR stabiliser about steady-flight trims (ac_lqr_f32, ac_lqr_gains_f32, ac_steady_error_f32;
// DESIGN.md §4.13).
//
// The steady-flight chart.  For a state x and a nominal xb, with psi_b the yaw of q_b and Z = R_z(psi_b):
//     xi = ( Z' (p - p_b),  R(q)' v - R(q_b)' v_b,  Z' 2 vec(q (x) q_b^-1),  w - w_b )            (12 coordinates)
// R(q) rotates body to NED (quaternions normalised, Hamilton xyzw), the sign of q (x) q_b^-1 makes its scalar part >= 0.
// Coordinates: 0 along-track, 1 cross-track, 2 down (heading frame), 3-5 body velocity, 6-7 tilt about the heading frame's
// forward and right axes, 8 heading, 9-11 body rates.  The dynamics are invariant under translation and under rotation
// about NED down, so with x+ = F(x_b, u_b, dt)
//     A_xi = E(x+) A T(x_b)  [12][12],     B_xi = E(x+) B  [12][7]
// (T = dx/dxi at xi = 0, E = dxi/dx; E annihilates the quaternion-norm direction) are the same at every point of the
// trim helix: steady flight is a fixed point of the chart, and 0, 1, 2, 8 feed none of the other eight coordinates.
//
// Kernels (lqr_inst.hip):
//   k_lqr_project    one lane per instance: analytic T and E, A_xi and B_xi from the handle's own step sensitivities
//   k_lqr_dare       one instance per 16-lane group (lane r owns row r of the 12x12 matrices, operands that every lane
//                    reads are mirrored in LDS): the structured doubling algorithm
//                        W = I + G H,   A+ = A W^-1 A,   G+ = G + A W^-1 G A',   H+ = H + A' H W^-1 A
//                    from A0 = A_xi, G0 = B R^-1 B', H0 = Q, G and H symmetrised each step, H_k -> P; W X = [A | G] is solved by
//                    elimination with partial pivoting across the group and back substitution.  A fixed number of
//                    iterations; an instance whose H moved by less than tol (relative, max norm) is frozen.  Then K = (R + B'PB)^-1 B'PA and the relative
//                    residual of the Riccati equation at the returned P.  The rows are float32; the elimination and the
//                    sums of the products run in float64.
//   k_lqr_gains      one lane per (node, instance): K_x,k = -K E(x_k), the layout ac_rollout_policy_f32 reads
//   k_steady_error   one lane per instance: the nonlinear chart
// The per-lane code is shared with the host build (tests/host_lqr, -DAC_HOST_CHECK), which runs the 16 lanes of a group one
// after the other, phase by phase: a phase reads from the mirrors only what an EARLIER phase wrote.
#pragma once
#include "ac_group.hpp"
#include "../../include/aircraft_hip.h"

#ifdef AC_HOST_CHECK
#define AC_LQR_INLINE
#else
#define AC_LQR_INLINE __attribute__((always_inline))
#endif

namespace ac {

constexpr int kLqrN = 12;       // chart coordinates
constexpr int kLqrM = 7;        // controls
constexpr int kLqrLanes = kGrpLanes;  // lanes of one instance's group (rows 12-15 idle)
constexpr int kLqrLd = 13;      // row stride of the LDS mirrors
constexpr int kLqrGroups = 4;   // instances per workgroup of k_lqr_dare (one wave)
constexpr int kLqrBlock = 256;  // lanes per workgroup of the one-lane-per-instance kernels
constexpr float kLqrFltMax = 3.0e38f;
constexpr long kLqrWsFloats = 13 + 169 + 91;  // x+ | A | B per instance

// status per instance (ac_lqr_f32's `status`)
constexpr int AC_LQR_CONVERGED = 0;
constexpr int AC_LQR_MAXITER = 1;
constexpr int AC_LQR_BREAKDOWN = 2;
constexpr int AC_LQR_NONFINITE = 3;

// a*b - c*d with both products rounded (never contracted into one FMA): exactly 0 when the two products are equal
AC_DI float lqr_det2(float a, float b, float c, float d) {
    const float p = a * b;
    const float q = c * d;
    return p - q;
}

// ---- the chart -----------------------------------------------------------------------------------------------------------------
// Frame of a nominal state: unit attitude, its norm before normalising, R(q) (body -> NED) and Z = R_z(yaw(q)).
struct LqrFrame {
    float q[4], nq;    // unit quaternion xyzw, |q| of the input
    float R[3][3];     // body -> NED
    float Z[3][3];     // heading frame -> NED
};

AC_DI LqrFrame lqr_frame(const float x[13]) {
    LqrFrame f;
    const float n2 = fmaf(x[6], x[6], fmaf(x[7], x[7], fmaf(x[8], x[8], x[9] * x[9])));
    f.nq = sqrtf(n2);
    const float inv = 1.0f / f.nq;
#pragma unroll
    for (int i = 0; i < 4; ++i) f.q[i] = x[6 + i] * inv;
    const float qx = f.q[0], qy = f.q[1], qz = f.q[2], qw = f.q[3];
    f.R[0][0] = 1.0f - 2.0f * (qy * qy + qz * qz); f.R[0][1] = 2.0f * lqr_det2(qx, qy, qz, qw); f.R[0][2] = 2.0f * (qx * qz + qy * qw);
    f.R[1][0] = 2.0f * (qx * qy + qz * qw); f.R[1][1] = 1.0f - 2.0f * (qx * qx + qz * qz); f.R[1][2] = 2.0f * lqr_det2(qy, qz, qx, qw);
    f.R[2][0] = 2.0f * lqr_det2(qx, qz, qy, qw); f.R[2][1] = 2.0f * (qy * qz + qx * qw); f.R[2][2] = 1.0f - 2.0f * (qx * qx + qy * qy);
    // cos, sin of the yaw atan2(R10, R00) without the angle (straight up or down: heading 0)
    const float hyp = sqrtf(fmaf(f.R[0][0], f.R[0][0], f.R[1][0] * f.R[1][0]));
    const float c = hyp > 0.f ? f.R[0][0] / hyp : 1.0f, s = hyp > 0.f ? f.R[1][0] / hyp : 0.0f;
    f.Z[0][0] = c; f.Z[0][1] = -s; f.Z[0][2] = 0.f;
    f.Z[1][0] = s; f.Z[1][1] = c; f.Z[1][2] = 0.f;
    f.Z[2][0] = 0.f; f.Z[2][1] = 0.f; f.Z[2][2] = 1.0f;
    return f;
}

// M' v for a 3x3 M
AC_DI void lqr_mtv(const float M[3][3], const float v[3], float o[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = fmaf(M[0][i], v[0], fmaf(M[1][i], v[1], M[2][i] * v[2]));
}

// xi = chart(x; xb)
AC_DI void lqr_chart(const float x[13], const float xb[13], float xi[12]) {
    const LqrFrame fb = lqr_frame(xb), fx = lqr_frame(x);
    const float dp[3] = {x[0] - xb[0], x[1] - xb[1], x[2] - xb[2]};
    lqr_mtv(fb.Z, dp, xi);
    float vx[3], vb[3];
    lqr_mtv(fx.R, x + 3, vx);
    lqr_mtv(fb.R, xb + 3, vb);
#pragma unroll
    for (int i = 0; i < 3; ++i) xi[3 + i] = vx[i] - vb[i];
    // d = q (x) conj(q_b): vec d = b_w a_v - a_w b_v - a_v x b_v, d_w = a_w b_w + a_v . b_v
    const float* a = fx.q;
    const float* b = fb.q;
    const float dw = fmaf(a[3], b[3], fmaf(a[0], b[0], fmaf(a[1], b[1], a[2] * b[2])));
    float d[3];
    d[0] = lqr_det2(b[3], a[0], a[3], b[0]) - lqr_det2(a[1], b[2], a[2], b[1]);
    d[1] = lqr_det2(b[3], a[1], a[3], b[1]) - lqr_det2(a[2], b[0], a[0], b[2]);
    d[2] = lqr_det2(b[3], a[2], a[3], b[2]) - lqr_det2(a[0], b[1], a[1], b[0]);
    const float sg = dw < 0.f ? -2.0f : 2.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] *= sg;
    lqr_mtv(fb.Z, d, xi + 6);
#pragma unroll
    for (int i = 0; i < 3; ++i) xi[9 + i] = x[10 + i] - xb[10 + i];
}

AC_DI void lqr_skew(const float v[3], float S[3][3]) {
    S[0][0] = 0.f; S[0][1] = -v[2]; S[0][2] = v[1];
    S[1][0] = v[2]; S[1][1] = 0.f; S[1][2] = -v[0];
    S[2][0] = -v[1]; S[2][1] = v[0]; S[2][2] = 0.f;
}

// T = dx/dxi at xi = 0 about xb, dense [13][12] (the zeros are literal: the unrolled users drop them)
AC_DI void lqr_T(const float xb[13], float T[13][12]) {
    const LqrFrame f = lqr_frame(xb);
#pragma unroll
    for (int i = 0; i < 13; ++i)
#pragma unroll
        for (int j = 0; j < 12; ++j) T[i][j] = 0.f;
    float S[3][3], M[4][3];
    lqr_skew(xb + 3, S);
    // d (x) q_b with q_b as it is, not normalised: xi = 0 is xb itself.  (The yaw column of T cancels terms of size |v| in
    // A T: a norm error of 1e-7 in the tangent would leave 1e-7 |v| of heading in the other coordinates.)
    float Sq[3][3];
    lqr_skew(xb + 6, Sq);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = (i == j ? xb[9] : 0.f) - Sq[i][j];
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3][j] = -xb[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            T[i][j] = f.Z[i][j];
            T[3 + i][3 + j] = f.R[i][j];
            T[3 + i][6 + j] = -fmaf(S[i][0], f.Z[0][j], fmaf(S[i][1], f.Z[1][j], S[i][2] * f.Z[2][j]));
            T[10 + i][9 + j] = i == j ? 1.0f : 0.f;
        }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[6 + i][6 + j] = 0.5f * fmaf(M[i][0], f.Z[0][j], fmaf(M[i][1], f.Z[1][j], M[i][2] * f.Z[2][j]));
}

// E = dxi/dx at x = xb, dense [12][13]
AC_DI void lqr_E(const float xb[13], float E[12][13]) {
    const LqrFrame f = lqr_frame(xb);
#pragma unroll
    for (int i = 0; i < 12; ++i)
#pragma unroll
        for (int j = 0; j < 13; ++j) E[i][j] = 0.f;
    float S[3][3], Sq[3][3], N2[3][4], SN[3][4];
    lqr_skew(xb + 3, S);
    lqr_skew(f.q, Sq);
    const float two = 2.0f / f.nq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) N2[i][j] = two * ((i == j ? f.q[3] : 0.f) + Sq[i][j]);
        N2[i][3] = -(two * f.q[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) SN[i][j] = fmaf(S[i][0], N2[0][j], fmaf(S[i][1], N2[1][j], S[i][2] * N2[2][j]));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            E[i][j] = f.Z[j][i];
            E[3 + i][3 + j] = f.R[j][i];
            E[9 + i][10 + j] = i == j ? 1.0f : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            E[3 + i][6 + j] = fmaf(f.R[0][i], SN[0][j], fmaf(f.R[1][i], SN[1][j], f.R[2][i] * SN[2][j]));
            E[6 + i][6 + j] = fmaf(f.Z[0][i], N2[0][j], fmaf(f.Z[1][i], N2[1][j], f.Z[2][i] * N2[2][j]));
        }
    }
}

// One instance's column of a [rows][n] array (element w at b[w * s]).
struct LqrCol {
    float* b;
    long s;
    AC_DI float& operator[](int w) const { return b[(long)w * s]; }
};
struct LqrCCol {
    const float* b;
    long s;
    AC_DI float operator[](int w) const { return b[(long)w * s]; }
};

AC_DI bool lqr_finite(float v) { return fabsf(v) <= kLqrFltMax; }  // (false for NaN)

// k_lqr_project's unit: A_xi = E(x+) A T(x), B_xi = E(x+) B.  A non-finite x or u makes every output NaN (the Riccati kernel
// reports it as AC_LQR_NONFINITE).
AC_DI void lqr_project_unit(const LqrCCol& X, const LqrCCol& U, const LqrCCol& Xp, const LqrCCol& A, const LqrCCol& B,
                            const LqrCol& Axi, const LqrCol& Bxi) {
    float x[13], xp[13];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        x[i] = X[i];
        xp[i] = Xp[i];
        ok = ok && lqr_finite(x[i]) && lqr_finite(xp[i]);
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) ok = ok && lqr_finite(U[i]);
    const float poison = ok ? 0.f : __builtin_nanf("");
    float T[13][12], E[12][13];
    lqr_T(x, T);
    lqr_E(xp, E);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        float col[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < 13; ++c)
                if ((c < 3 && j < 3) || (c >= 3 && c < 6 && j >= 3 && j < 9) || (c >= 6 && c < 10 && j >= 6 && j < 9) ||
                    (c >= 10 && j >= 9))  // the blocks of T that are not identically zero
                    acc = fmaf(A[i * 13 + c], T[c][j], acc);
            col[i] = acc;
        }
#pragma unroll
        for (int r = 0; r < 12; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < 13; ++i)
                if ((r < 3 && i < 3) || (r >= 3 && r < 6 && i >= 3 && i < 10) || (r >= 6 && r < 9 && i >= 6 && i < 10) ||
                    (r >= 9 && i >= 10))  // the blocks of E that are not identically zero
                    acc = fmaf(E[r][i], col[i], acc);
            Axi[r * 12 + j] = acc + poison;
        }
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        float col[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) col[i] = B[i * 7 + c];
#pragma unroll
        for (int r = 0; r < 12; ++r) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < 13; ++i)
                if ((r < 3 && i < 3) || (r >= 3 && r < 6 && i >= 3 && i < 10) || (r >= 6 && r < 9 && i >= 6 && i < 10) ||
                    (r >= 9 && i >= 10))
                    acc = fmaf(E[r][i], col[i], acc);
            Bxi[r * 7 + c] = acc + poison;
        }
    }
}

// k_lqr_gains' unit: K_x = -K E(x_k)  [7][13]
AC_DI void lqr_gains_unit(const LqrCCol& Xk, const LqrCCol& K, const LqrCol& Kx) {
    float x[13], E[12][13];
#pragma unroll
    for (int i = 0; i < 13; ++i) x[i] = Xk[i];
    lqr_E(x, E);
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        float k[12];
#pragma unroll
        for (int r = 0; r < 12; ++r) k[r] = K[c * 12 + r];
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            float acc = 0.f;
#pragma unroll
            for (int r = 0; r < 12; ++r)
                if ((r < 3 && i < 3) || (r >= 3 && r < 6 && i >= 3 && i < 10) || (r >= 6 && r < 9 && i >= 6 && i < 10) ||
                    (r >= 9 && i >= 10))
                    acc = fmaf(k[r], E[r][i], acc);
            Kx[c * 13 + i] = -acc;
        }
    }
}

AC_DI void lqr_error_unit(const LqrCCol& X, const LqrCCol& Xb, const LqrCol& Xi) {
    float x[13], xb[13], xi[12];
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        x[i] = X[i];
        xb[i] = Xb[i];
    }
    lqr_chart(x, xb, xi);
#pragma unroll
    for (int i = 0; i < 12; ++i) Xi[i] = xi[i];
}

// ---- the Riccati solve: one instance on a group of 16 lanes ----------------------------------------------------------------------
// The mirrors of one instance (LDS on the device).
struct LqrShared {
    float m[4][kLqrLanes][kLqrLd];
    double row[2][36];    // the pivot / solution row of an elimination step (two in flight)
    float red[2][kLqrLanes];  // per-lane partial results of a reduction
    float c[kLqrLanes];   // pivot candidates | per-lane partial results
};

// What lane r of a group keeps in registers.
struct LqrLane {
    float a[12], g[12], h[12];    // row r of A_k, G_k, H_k
    double w[12], x[24];          // row r of the system being eliminated and of its right-hand sides (lqr_solve_rows)
    float t[12], u[12], an[12];   // row r of A X2 -> G+, of H X1 -> H+, of A+
    int piv, p;                   // the column this lane's row was the pivot of; the pivot lane of the current step
    bool used;                    // this lane's row has been a pivot
    bool done, bad, nonfinite;    // the instance: frozen, broken down, non-finite input (every lane holds the same values)
    int iters;
};

// the dropped coordinates as a bit mask: q[i] == 0 for i in {0, 1, 2, 8}
AC_DI int lqr_drop_mask(const ac_lqr_opts& o) {
    return (o.q[0] == 0.f ? 1 : 0) | (o.q[1] == 0.f ? 2 : 0) | (o.q[2] == 0.f ? 4 : 0) | (o.q[8] == 0.f ? 256 : 0);
}
// o.q[r] / o.r[c] for a lane-dependent index (a select chain: the options stay in scalar registers)
AC_DI float lqr_q_of(const ac_lqr_opts& o, int r) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) v = i == r ? o.q[i] : v;
    return v;
}
AC_DI float lqr_r_of(const ac_lqr_opts& o, int c) {
    float v = 1.0f;
#pragma unroll
    for (int i = 0; i < 7; ++i) v = i == c ? o.r[i] : v;
    return v;
}

// the lane with the largest pivot candidate (the lowest lane on ties; a NaN never wins against a number)
AC_DI int lqr_pivot_lane(const float c[kLqrLanes], float& best) {
    int p = 0;
    best = c[0];
#pragma unroll
    for (int i = 1; i < kLqrLanes; ++i) {
        const float v = c[i];
        if (v > best) {
            best = v;
            p = i;
        }
    }
    return p;
}

// Elimination with partial pivoting across the group, then back substitution (the arithmetic of an LU solve): lanes
// 0..NW-1 hold row r of W in L.w[0..NW) and of the right-hand sides in L.x[0..NR).  Forward: the unused row with the largest
// entry in column k becomes its pivot row, is scaled to a unit pivot and eliminated from the rows not yet used.  Backward:
// the finished solution rows are substituted into the earlier pivot rows.  Afterwards the lane whose row was the pivot of
// column k (L.piv == k) holds row k of W^-1 RHS in L.x.  A pivot at or below 0 (or NaN) marks the instance broken down;
// the arithmetic goes on (no lane leaves).
// The system and its solve are float64, like the 12-term sums of the products around it (lqr_row_times): cond(I + G H)
// reaches 2e5 on the trims of the test grid, and float32 there puts 1e-4 into K instead of 3e-5.  What is
// kept between phases (the lanes' rows of A_k, G_k, H_k and the mirrors) is float32.
template <int NW, int NR, class G>
AC_DI void lqr_solve_rows(G& grp, LqrShared& s) {
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
        L.used = r >= NW;
        L.piv = r < NW ? r : NW;
        s.c[r] = L.used ? -1.0f : (float)fabs(L.w[0]);
    });
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            float best;
            const int p = lqr_pivot_lane(s.c, best);  // partial pivoting: the largest candidate of column k
            if (!(best > 0.f) || !(best <= kLqrFltMax)) L.bad = true;
            L.p = L.used ? -1 : p;  // (-1: this row takes no part in the elimination of column k)
            if (r == p) {
                const double inv = 1.0 / L.w[k];
#pragma unroll
                for (int j = k + 1; j < NW; ++j) {
                    L.w[j] *= inv;
                    s.row[k & 1][j] = L.w[j];
                }
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    L.x[j] *= inv;
                    s.row[k & 1][12 + j] = L.x[j];
                }
                L.used = true;
                L.piv = k;
                L.p = -1;
            }
        });
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            if (L.p >= 0) {
                const double f = L.w[k];
#pragma unroll
                for (int j = k + 1; j < NW; ++j) L.w[j] = fma(-f, s.row[k & 1][j], L.w[j]);
#pragma unroll
                for (int j = 0; j < NR; ++j) L.x[j] = fma(-f, s.row[k & 1][12 + j], L.x[j]);
            }
            const int kn = k + 1 < NW ? k + 1 : k;  // (no candidates after the last column)
            s.c[r] = L.used ? -1.0f : (float)fabs(L.w[kn]);
        });
    }
    // (row[(NW - 1) & 1] still holds the last pivot row: a finished solution row)
#pragma unroll
    for (int k = NW - 1; k >= 1; --k) {
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            if (L.piv < k) {
                const double f = L.w[k];
#pragma unroll
                for (int j = 0; j < NR; ++j) L.x[j] = fma(-f, s.row[k & 1][12 + j], L.x[j]);
            }
            if (L.piv == k - 1) {
#pragma unroll
                for (int j = 0; j < NR; ++j) s.row[(k - 1) & 1][12 + j] = L.x[j];
            }
        });
    }
}

// row r of A_xi and B_xi with the dropped coordinates zeroed; returns false when an entry is not finite
AC_DI bool lqr_load_rows(const LqrCCol& Axi, const LqrCCol& Bxi, int r, int drop, float a[12], float b[7]) {
    bool ok = true;
    const bool live = r < kLqrN;
    const int rr = live ? r : 0;
    const bool zr = !live || ((drop >> rr) & 1);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const float v = Axi[rr * 12 + j];
        ok = ok && lqr_finite(v);
        a[j] = (zr || ((drop >> j) & 1)) ? 0.f : v;
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const float v = Bxi[rr * 7 + c];
        ok = ok && lqr_finite(v);
        b[c] = zr ? 0.f : v;
    }
    return ok;
}

// out[j] = sum_k v[k] M[k][j], j < NJ: a lane's row times a mirrored matrix (float64 sums, one rounding per entry)
template <int NJ>
AC_DI void lqr_row_times(const float v[12], const float (*M)[kLqrLd], float out[NJ]) {
    double acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = fma((double)v[k], (double)M[k][j], acc[j]);
#pragma unroll
    for (int j = 0; j < NJ; ++j) out[j] = (float)acc[j];
}

// The whole solve of one instance.  G: the group (device: one lane and a barrier after every phase; host: a loop over the lanes).
// Outputs P [12][12], K [7][12] (component-major columns), resid, status, used_iters of this instance, written when `store`.
template <class G>
AC_DI void lqr_dare_group(G& grp, LqrShared& s, const ac_lqr_opts& o, int iters, const LqrCCol& Axi, const LqrCCol& Bxi,
                          const LqrCol& P, const LqrCol& K, float* resid, int* status, int* used_iters, bool store) {
    const int drop = lqr_drop_mask(o);
    // A0, B -> registers and mirrors; G0 = B R^-1 B', H0 = Q
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
        float b[7];
        const bool ok = lqr_load_rows(Axi, Bxi, r, drop, L.a, b);
        s.c[r] = ok ? 0.f : 1.0f;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            s.m[2][r][c] = b[c];
            L.t[c] = b[c] / o.r[c];
        }
        L.done = false;
        L.bad = false;
        L.iters = 0;
    });
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
        bool nf = false;
#pragma unroll
        for (int i = 0; i < kLqrN; ++i) nf = nf || s.c[i] != 0.f;
        L.nonfinite = nf;
        const float qr = (r < kLqrN && !((drop >> r) & 1)) ? lqr_q_of(o, r) : 0.f;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < 7; ++c) acc = fmaf(L.t[c], s.m[2][j][c], acc);
            L.g[j] = acc;
            L.h[j] = j == r ? qr : 0.f;
            s.m[0][r][j] = L.h[j];
        }
    });
    for (int it = 0; it < iters; ++it) {
        // W = I + G H (H mirrored in m0); right-hand sides [A | G]
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                L.w[j] = j == r ? 1.0 : 0.0;
                L.x[j] = L.a[j];
                L.x[12 + j] = L.g[j];
            }
#pragma unroll
            for (int k = 0; k < 12; ++k)
#pragma unroll
                for (int j = 0; j < 12; ++j) L.w[j] = fma((double)L.g[k], (double)s.m[0][k][j], L.w[j]);
        });
        lqr_solve_rows<12, 24>(grp, s);
        // X1 = W^-1 A -> m1, X2 = W^-1 G -> m2, A -> m3
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            if (r < kLqrN) {
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    s.m[1][L.piv][j] = (float)L.x[j];
                    s.m[2][L.piv][j] = (float)L.x[12 + j];
                    s.m[3][r][j] = L.a[j];
                }
            }
        });
        // A+ = A X1, t = A X2, u = H X1 (-> m0)
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            lqr_row_times<12>(L.a, s.m[1], L.an);
            lqr_row_times<12>(L.a, s.m[2], L.t);
            lqr_row_times<12>(L.h, s.m[1], L.u);
#pragma unroll
            for (int j = 0; j < 12; ++j) s.m[0][r][j] = L.u[j];
        });
        // G+ = G + t A', H+ = H + A' u (-> m1, m2 for the symmetrisation)
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            const int rc = r < kLqrN ? r : 0;
            double hn[12], gn[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) hn[j] = L.h[j];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const double akr = s.m[3][k][rc];  // A_k[k][r]: row r of A_k' u
#pragma unroll
                for (int j = 0; j < 12; ++j) hn[j] = fma(akr, (double)s.m[0][k][j], hn[j]);
            }
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                double acc = L.g[j];
#pragma unroll
                for (int k = 0; k < 12; ++k) acc = fma((double)L.t[k], (double)s.m[3][j][k], acc);
                gn[j] = acc;
            }
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                L.t[j] = (float)gn[j];
                L.u[j] = (float)hn[j];
                s.m[1][r][j] = L.t[j];
                s.m[2][r][j] = L.u[j];
            }
        });
        // symmetrise; how far H moved
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            const int rc = r < kLqrN ? r : 0;
            float diff = 0.f, hm = 0.f;
            bool fin = true;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                L.t[j] = 0.5f * (L.t[j] + s.m[1][j][rc]);
                L.u[j] = 0.5f * (L.u[j] + s.m[2][j][rc]);
                diff = fmaxf(diff, fabsf(L.u[j] - L.h[j]));
                hm = fmaxf(hm, fabsf(L.u[j]));
                fin = fin && lqr_finite(L.an[j]) && lqr_finite(L.t[j]) && lqr_finite(L.u[j]);
            }
            const bool live = r < kLqrN;
            s.c[r] = live ? diff : 0.f;
            s.red[0][r] = live ? hm : 0.f;
            s.red[1][r] = (live && !fin) ? 1.0f : 0.f;
        });
        // commit (a frozen or broken instance keeps its state), H -> m0 for the next iteration
        grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
            float diff = 0.f, hm = 0.f;
            bool nf = false;
#pragma unroll
            for (int i = 0; i < kLqrN; ++i) {
                diff = fmaxf(diff, s.c[i]);
                hm = fmaxf(hm, s.red[0][i]);
                nf = nf || s.red[1][i] != 0.f;
            }
            if (!L.done && !L.bad && !L.nonfinite) {
                if (nf) {
                    L.bad = true;
                } else {
#pragma unroll
                    for (int j = 0; j < 12; ++j) {
                        L.a[j] = L.an[j];
                        L.g[j] = L.t[j];
                        L.h[j] = L.u[j];
                    }
                    L.iters = it + 1;
                    L.done = diff < o.tol * hm;
                }
            }
#pragma unroll
            for (int j = 0; j < 12; ++j) s.m[0][r][j] = L.h[j];
        });
    }
    // ---- K = (R + B'PB)^-1 B'PA and the residual, from the reduced A_xi, B_xi --------------------------------------------------
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
        float b[7];
        lqr_load_rows(Axi, Bxi, r, drop, L.a, b);
#pragma unroll
        for (int j = 0; j < 12; ++j) s.m[1][r][j] = L.a[j];
#pragma unroll
        for (int c = 0; c < 7; ++c) s.m[2][r][c] = b[c];
    });
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {  // P A -> m3, P B -> m0
        lqr_row_times<12>(L.h, s.m[1], L.t);
        lqr_row_times<7>(L.h, s.m[2], L.u);
#pragma unroll
        for (int j = 0; j < 12; ++j) s.m[3][r][j] = L.t[j];
#pragma unroll
        for (int c = 0; c < 7; ++c) s.m[0][r][c] = L.u[c];
    });
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {  // lane c < 7: row c of S = R + B'PB and of Y = B'PA
        const int c = r < kLqrM ? r : 0;
        const float rc = lqr_r_of(o, c);
#pragma unroll
        for (int d = 0; d < 7; ++d) L.w[d] = d == c ? (double)rc : 0.0;
#pragma unroll
        for (int j = 0; j < 12; ++j) L.x[j] = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const double bkc = s.m[2][k][c];
#pragma unroll
            for (int d = 0; d < 7; ++d) L.w[d] = fma(bkc, (double)s.m[0][k][d], L.w[d]);
#pragma unroll
            for (int j = 0; j < 12; ++j) L.x[j] = fma(bkc, (double)s.m[3][k][j], L.x[j]);
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) L.an[j] = (float)L.x[j];
    });
    lqr_solve_rows<7, 12>(grp, s);
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {  // K -> m2, Y -> m0
        if (r < kLqrM) {
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                s.m[2][L.piv][j] = (float)L.x[j];
                s.m[0][r][j] = L.an[j];
            }
        }
    });
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {  // row r of Q + A'(PA) - Y'K - P
        const int rc = r < kLqrN ? r : 0;
        const float qr = (r < kLqrN && !((drop >> r) & 1)) ? lqr_q_of(o, r) : 0.f;
        float res[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) res[j] = (j == r ? qr : 0.f) - L.h[j];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const float akr = s.m[1][k][rc];
#pragma unroll
            for (int j = 0; j < 12; ++j) res[j] = fmaf(akr, s.m[3][k][j], res[j]);
        }
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const float ycr = s.m[0][c][rc];
#pragma unroll
            for (int j = 0; j < 12; ++j) res[j] = fmaf(-ycr, s.m[2][c][j], res[j]);
        }
        float rm = 0.f, pm = 0.f;
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            rm = fmaxf(rm, fabsf(res[j]));
            pm = fmaxf(pm, fabsf(L.h[j]));
            fin = fin && lqr_finite(res[j]) && (r >= kLqrM || lqr_finite(s.m[2][rc][j]));
        }
        const bool live = r < kLqrN;
        s.c[r] = live ? rm : 0.f;
        s.red[0][r] = live ? pm : 0.f;
        s.red[1][r] = (live && !fin) ? 1.0f : 0.f;
    });
    grp.each([&](LqrLane& L, int r) AC_LQR_INLINE {
        float rm = 0.f, pm = 0.f;
        bool nf = false;
#pragma unroll
        for (int i = 0; i < kLqrN; ++i) {
            rm = fmaxf(rm, s.c[i]);
            pm = fmaxf(pm, s.red[0][i]);
            nf = nf || s.red[1][i] != 0.f;
        }
        const int st = L.nonfinite ? AC_LQR_NONFINITE : (L.bad || nf) ? AC_LQR_BREAKDOWN : L.done ? AC_LQR_CONVERGED : AC_LQR_MAXITER;
        const bool ok = st == AC_LQR_CONVERGED || st == AC_LQR_MAXITER;
        const float nan = __builtin_nanf("");
        if (store && r < kLqrN) {
#pragma unroll
            for (int j = 0; j < 12; ++j) P[r * 12 + j] = ok ? L.h[j] : nan;
        }
        if (store && r < kLqrM) {
#pragma unroll
            for (int j = 0; j < 12; ++j) K[r * 12 + j] = ok ? s.m[2][r][j] : nan;
        }
        if (store && r == 0) {
            *resid = ok ? rm / pm : nan;
            *status = st;
            *used_iters = L.iters;
        }
    });
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launchers (defined in lqr_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; none allocates or
// synchronises.  `grid` receives the launch dimension (ac_last_launch).
hipError_t lqr_launch_project(const float* X, const float* U, const float* Xp, const float* A, const float* B, long n, float* Axi,
                              float* Bxi, hipStream_t st, int* grid);
hipError_t lqr_launch_dare(const ac_lqr_opts& o, int iters, const float* Axi, const float* Bxi, long n, float* P, float* K,
                           float* resid, int* status, int* used_iters, hipStream_t st, int* grid, int* lds);
hipError_t lqr_launch_gains(const float* Xnom, const float* K, long n, long H, float* Kx, hipStream_t st, int* grid);
hipError_t lqr_launch_error(const float* X, const float* Xnom, long n, float* xi, hipStream_t st, int* grid);
}  // namespace ac
#endif
