// ac_trim.hpp — batched steady-flight trim of the fixed-wing models (ac_trim_f32).
//
// Per instance: given position p, airspeed V, heading psi, turn rate psid about NED down, the held control rows 3-6 and
// either the sideslip beta (lateral mode 0: the rudder is solved for) or the rudder (mode 1: beta is solved for), find
//     z = (alpha, theta, phi [rad], aileron, elevator [deg], rudder [deg] | beta [rad])
// with r(z) = 0, where from z
//     q    = quat_from_euler(phi, theta, psi)            (xyzw, body -> NED; euler_angles() in ac_dynamics.hpp inverts it)
//     v_b  = V (cos a cos b, sin b, sin a cos b),   v_ned = q v_b q^-1,   w_b = q^-1 (0, 0, psid) q
//     u    = (aileron, elevator, rudder, held rows 3-6)
//     r_v  = q^-1 f[3:6] q - w_b x v_b                    (body-axis rate of change of the velocity vector)
//     r_w  = f[10:13]                                     (f = state_derivative(x, u))
// r = 0 exactly when body velocity and body rates are constant.  Damped Gauss-Newton (Levenberg-Marquardt) with box
// projection, a fixed number of iterations, each one three launches (abi_flight.hip, ac_trim_f32):
//   k_trim_assemble     z -> X [13][n], U [7][n] in the workspace (one lane per instance)
//   derivative sens.    the handle's own ac_state_derivative_sens_f32 launch: Xdot, Fx [13][13][n], Fu [13][7][n]
//   k_trim_update       r and J_z = dr/dz (a Dual<6> seeded in z: f's tangent is Fx dx/dz + Fu du/dz, pushed through
//                       the rotation and the w_b x v_b term), accept / reject against the stored best, the next candidate
//                       from a 6x6 Cholesky solve in registers, projected onto the bounds
// Every coefficient model works, the MLP engines included, because f and its Jacobians come from the model's own kernel.
#pragma once
#include "ac_dynamics.hpp"

namespace ac {

// ---- the workspace: per instance, component-major like every other [rows][n] buffer ------------------------------------
//   X 13 | U 7 | Xdot 13 | Fx 169 | Fu 91 | LM state kTrimStateWords
constexpr int kTrimStateWords = 57;
constexpr long kTrimWsFloats = 13 + 7 + 13 + 169 + 91 + kTrimStateWords;
// words of the LM state column
constexpr int kTzc = 0;     // candidate z (the one the launches of this iteration evaluate)
constexpr int kTzb = 6;     // best z so far
constexpr int kTrb = 12;    // its residual
constexpr int kTJb = 18;    // its Jacobian, row-major [6][6]
constexpr int kTlam = 54;   // damping lambda
constexpr int kTcost = 55;  // its scaled |r|^2 (+inf before the first finite evaluation)
constexpr int kTflag = 56;  // kTrimActive, or the final status of a frozen instance (AC_TRIM_CONVERGED, AC_TRIM_NONFINITE)
constexpr float kTrimActive = -1.0f;
constexpr int kTrimBlock = 256;  // lanes per workgroup of both kernels (one instance per lane)
constexpr float kTrimLambda0 = 1e-3f, kTrimLambdaMin = 1e-8f, kTrimLambdaMax = 1e8f;

// status per instance (ac_trim_f32's `status`)
constexpr int AC_TRIM_CONVERGED = 0;
constexpr int AC_TRIM_MAXITER = 1;
constexpr int AC_TRIM_BOUND = 2;
constexpr int AC_TRIM_NONFINITE = 3;

// One instance's column of a [rows][n] array: element w at b[w * s] (s = n on the device, 1 in the host build).
struct TrimCol {
    float* b;
    long s;
    AC_DI float& operator[](int w) const { return b[(long)w * s]; }
};
// The derivative-sensitivity outputs of one instance: Xdot [13], Fx [13][13], Fu [13][7], stride s.
struct TrimSens {
    const float* xd;
    const float* fx;
    const float* fu;
    long s;
    AC_DI float f(int r) const { return xd[(long)r * s]; }
    AC_DI float dx(int r, int c) const { return fx[(long)(r * 13 + c) * s]; }
    AC_DI float du(int r, int c) const { return fu[(long)(r * 7 + c) * s]; }
};

// target [7][n]: p(3), V, psi, turn rate, beta (mode 0) | rudder (mode 1)
struct TrimTarget {
    float p[3], V, psi, psid, lat;
};
AC_DI TrimTarget trim_target(const float* T, long n, long i) {
    TrimTarget t;
    t.p[0] = T[i]; t.p[1] = T[n + i]; t.p[2] = T[2 * n + i];
    t.V = T[3 * n + i]; t.psi = T[4 * n + i]; t.psid = T[5 * n + i]; t.lat = T[6 * n + i];
    return t;
}

AC_DI void trim_sincos(float a, float& s, float& c) { s = sinf(a); c = cosf(a); }
template <int N> AC_DI void trim_sincos(const Dual<N>& a, Dual<N>& s, Dual<N>& c) {
    s.v = sinf(a.v); c.v = cosf(a.v);
#pragma unroll
    for (int i = 0; i < N; ++i) { s.d[i] = c.v * a.d[i]; c.d[i] = -(s.v * a.d[i]); }
}

// z -> attitude, body velocity, NED velocity and body rates.  T = float (the assembled state) or Dual<N> seeded in z.
template <class T>
AC_DI void trim_kinematics(const TrimTarget& t, int lateral, const T z[6], Q4<T>& q, T vb[3], T vn[3], T wb[3]) {
    T sa, ca, sb, cb, sr, cr, sp, cp;
    trim_sincos(z[0], sa, ca);
    const T be = lateral ? z[5] : T(t.lat);
    trim_sincos(be, sb, cb);
    trim_sincos(z[2] * 0.5f, sr, cr);
    trim_sincos(z[1] * 0.5f, sp, cp);
    const float sy = sinf(0.5f * t.psi), cy = cosf(0.5f * t.psi);
    // synthetic.quat_from_euler(roll = phi, pitch = theta, yaw = psi)
    q.x = (sr * cp) * cy - (cr * sp) * sy;
    q.y = (cr * sp) * cy + (sr * cp) * sy;
    q.z = (cr * cp) * sy - (sr * sp) * cy;
    q.w = (cr * cp) * cy + (sr * sp) * sy;
    vb[0] = t.V * (ca * cb);
    vb[1] = t.V * sb;
    vb[2] = t.V * (sa * cb);
    const Q4<T> qi = qinv(q);
    const Q4<T> a = qmul(qmul_vec(q, vb[0], vb[1], vb[2]), qi);
    vn[0] = a.x; vn[1] = a.y; vn[2] = a.z;
    const T zero(0.f);
    const Q4<T> w = qmul(qmul_vec(qi, zero, zero, T(t.psid)), q);
    wb[0] = w.x; wb[1] = w.y; wb[2] = w.z;
}

// z -> the state and control the derivative-sensitivity launch evaluates.  uh: held rows 3-6.
AC_DI void trim_assemble(const TrimTarget& t, int lateral, const float z[6], const float uh[4], float x[13], float u[7]) {
    Q4<float> q;
    float vb[3], vn[3], wb[3];
    trim_kinematics(t, lateral, z, q, vb, vn, wb);
    x[0] = t.p[0]; x[1] = t.p[1]; x[2] = t.p[2];
    x[3] = vn[0]; x[4] = vn[1]; x[5] = vn[2];
    x[6] = q.x; x[7] = q.y; x[8] = q.z; x[9] = q.w;
    x[10] = wb[0]; x[11] = wb[1]; x[12] = wb[2];
    u[0] = z[3]; u[1] = z[4]; u[2] = lateral ? t.lat : z[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[3 + k] = uh[k];
}

// r_v = q^-1 f_v q - w_b x v_b,  r_w = f_w
template <class T>
AC_DI void trim_residual(const Q4<T>& q, const T fv[3], const T fw[3], const T vb[3], const T wb[3], T r[6]) {
    const Q4<T> a = qmul(qmul_vec(qinv(q), fv[0], fv[1], fv[2]), q);
    r[0] = a.x - (wb[1] * vb[2] - wb[2] * vb[1]);
    r[1] = a.y - (wb[2] * vb[0] - wb[0] * vb[2]);
    r[2] = a.z - (wb[0] * vb[1] - wb[1] * vb[0]);
    r[3] = fw[0]; r[4] = fw[1]; r[5] = fw[2];
}

// r(z) and J_z = dr/dz [6][6] from f's value and Jacobians at the assembled (x(z), u(z)).  Only rows 3-5 and 10-12 of f
// enter r; p never enters f, so columns 0-2 of Fx do not either.
template <class S>
AC_DI void trim_residual_jacobian(const TrimTarget& t, int lateral, const float zv[6], const S& sens, float r[6], float J[36]) {
    typedef Dual<6> D;
    D z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        z[j] = D(zv[j]);
        z[j].d[j] = 1.f;
    }
    Q4<D> q;
    D vb[3], vn[3], wb[3];
    trim_kinematics(t, lateral, z, q, vb, vn, wb);
    const D xs[10] = {vn[0], vn[1], vn[2], q.x, q.y, q.z, q.w, wb[0], wb[1], wb[2]};  // rows 3..12 of x
    constexpr int kRows[6] = {3, 4, 5, 10, 11, 12};
    D f[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int rr = kRows[k];
        f[k].v = sens.f(rr);
#pragma unroll
        for (int j = 0; j < 6; ++j) f[k].d[j] = 0.f;
#pragma unroll
        for (int c = 0; c < 10; ++c) {
            const float a = sens.dx(rr, 3 + c);
#pragma unroll
            for (int j = 0; j < 6; ++j) f[k].d[j] = fmaf(a, xs[c].d[j], f[k].d[j]);
        }
        f[k].d[3] += sens.du(rr, 0);             // aileron
        f[k].d[4] += sens.du(rr, 1);             // elevator
        if (!lateral) f[k].d[5] += sens.du(rr, 2);  // rudder (mode 0)
    }
    D rd[6];
    trim_residual(q, f, f + 3, vb, wb, rd);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        r[i] = rd[i].v;
#pragma unroll
        for (int j = 0; j < 6; ++j) J[i * 6 + j] = rd[i].d[j];
    }
}

// residual rows scaled by the tolerances: the instance has converged when every scaled entry is <= 1 in magnitude
AC_DI float trim_row_weight(const ac_trim_opts& o, int i) { return i < 3 ? 1.0f / o.tol_v : 1.0f / o.tol_w; }
AC_DI bool trim_converged(const ac_trim_opts& o, const float r[6]) {
    return fabsf(r[0]) <= o.tol_v && fabsf(r[1]) <= o.tol_v && fabsf(r[2]) <= o.tol_v && fabsf(r[3]) <= o.tol_w &&
           fabsf(r[4]) <= o.tol_w && fabsf(r[5]) <= o.tol_w;  // (false for NaN)
}
AC_DI float trim_cost(const ac_trim_opts& o, const float r[6]) {
    float c = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float e = r[i] * trim_row_weight(o, i);
        c = fmaf(e, e, c);
    }
    return c;
}
// g = J' W^2 r: the gradient of half the scaled cost
AC_DI void trim_gradient(const ac_trim_opts& o, const float r[6], const float J[36], float g[6]) {
#pragma unroll
    for (int j = 0; j < 6; ++j) g[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float w = trim_row_weight(o, i);
        const float wr = w * w * r[i];
#pragma unroll
        for (int j = 0; j < 6; ++j) g[j] = fmaf(J[i * 6 + j], wr, g[j]);
    }
}

// The next candidate: (H + lam diag(H) + mu I) dz = -g with H = J' W^2 J, by a 6x6 Cholesky of the diagonally scaled
// system (unit diagonal), then z + dz projected onto [lo, hi].  A non-finite step leaves z where it is (its re-evaluation
// is then no improvement, and lambda grows).
AC_DI void trim_step(const ac_trim_opts& o, const float z[6], const float r[6], const float J[36], float lam, float zn[6]) {
    float g[6], H[6][6];
    trim_gradient(o, r, J, g);
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = 0; k <= j; ++k) H[j][k] = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float w = trim_row_weight(o, i);
        const float w2 = w * w;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float a = w2 * J[i * 6 + j];
#pragma unroll
            for (int k = 0; k <= j; ++k) H[j][k] = fmaf(a, J[i * 6 + k], H[j][k]);
        }
    }
    float hmax = 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j) hmax = fmaxf(hmax, H[j][j]);
    const float mu = 1e-7f * hmax + 1e-30f;  // keeps a column J does not depend on (the linear model's rudder) solvable
    float d[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) d[j] = 1.0f / sqrtf(fmaf(H[j][j], 1.0f + lam, mu));
    // L L' = D (H + lam diag(H) + mu I) D, unit diagonal before the factorisation
    float L[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float s = 1.0f;
#pragma unroll
        for (int k = 0; k < j; ++k) s = fmaf(-L[j][k], L[j][k], s);
        s = sqrtf(fmaxf(s, 1e-12f));
        L[j][j] = s;
        const float inv = 1.0f / s;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float a = H[i][j] * (d[i] * d[j]);
#pragma unroll
            for (int k = 0; k < j; ++k) a = fmaf(-L[i][k], L[j][k], a);
            L[i][j] = a * inv;
        }
    }
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float a = -(d[i] * g[i]);
#pragma unroll
        for (int k = 0; k < i; ++k) a = fmaf(-L[i][k], y[k], a);
        y[i] = a / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        float a = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) a = fmaf(-L[k][i], y[k], a);
        y[i] = a / L[i][i];
    }
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) finite = finite && (fabsf(y[j] * d[j]) <= 3.0e38f);
#pragma unroll
    for (int j = 0; j < 6; ++j) zn[j] = finite ? fminf(fmaxf(z[j] + d[j] * y[j], o.lo[j]), o.hi[j]) : z[j];
}

// Status of an instance that is still active after the last iteration: AC_TRIM_BOUND when some z_j sits on a bound and
// the descent direction -g points out of the box there, else AC_TRIM_MAXITER.
AC_DI int trim_final_status(const ac_trim_opts& o, const float z[6], const float r[6], const float J[36]) {
    float g[6];
    trim_gradient(o, r, J, g);
    bool stuck = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) stuck = stuck || (z[j] >= o.hi[j] && g[j] < 0.f) || (z[j] <= o.lo[j] && g[j] > 0.f);
    return stuck ? AC_TRIM_BOUND : AC_TRIM_MAXITER;
}

// The inputs of one instance are usable: V > 0, everything finite.
AC_DI bool trim_inputs_ok(const TrimTarget& t, const float uh[4], const float z0[6]) {
    bool ok = t.V > 0.f && t.V <= 3.0e38f;
    const float v[6] = {t.p[0], t.p[1], t.p[2], t.psi, t.psid, t.lat};
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && fabsf(v[k]) <= 3.0e38f;
#pragma unroll
    for (int k = 0; k < 4; ++k) ok = ok && fabsf(uh[k]) <= 3.0e38f;
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && fabsf(z0[k]) <= 3.0e38f;
    return ok;
}

// First launch of a call: the LM state from the guess (projected onto the bounds) and the validity of the inputs.
AC_DI void trim_init_unit(const ac_trim_opts& o, const TrimTarget& t, const float uh[4], const float z0[6], const TrimCol& c) {
    const bool ok = trim_inputs_ok(t, uh, z0);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float z = ok ? fminf(fmaxf(z0[j], o.lo[j]), o.hi[j]) : z0[j];
        c[kTzc + j] = z;
        c[kTzb + j] = z;
        c[kTrb + j] = __builtin_nanf("");
    }
    c[kTlam] = kTrimLambda0;
    c[kTcost] = __builtin_inff();
    c[kTflag] = ok ? kTrimActive : (float)AC_TRIM_NONFINITE;
}

// k_trim_assemble's unit: the candidate of an active instance -> x, u.  Returns false (writes nothing) for a frozen one.
// An instance whose inputs are unusable gets a benign level-flight state once (init), so that no NaN enters the model.
AC_DI bool trim_assemble_unit(const ac_trim_opts& o, const TrimTarget& t, const float uh[4], const TrimCol& c, bool init,
                              float x[13], float u[7]) {
    const float flag = c[kTflag];
    if (flag != kTrimActive) {
        if (!init) return false;
#pragma unroll
        for (int k = 0; k < 13; ++k) x[k] = 0.f;
        x[3] = 30.f; x[9] = 1.f;
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = 0.f;
        return true;
    }
    float z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) z[j] = c[kTzc + j];
    trim_assemble(t, o.lateral, z, uh, x, u);
    return true;
}

// k_trim_update's unit.  An active instance: evaluate the candidate, accept (store z, r, J; lambda / 3) or reject
// (restore them; lambda x 4), freeze on convergence, else form the next candidate (not after the last iteration).
// On the last iteration (`last`) it returns the best z, its r and the status; the caller writes them out.
template <class S>
AC_DI void trim_update_unit(const ac_trim_opts& o, const TrimTarget& t, const S& sens, const TrimCol& c, bool last,
                            float zo[6], float ro[6], int& status) {
    float flag = c[kTflag];
    if (flag == kTrimActive) {
        float zb[6], rb[6], Jb[36];
#pragma unroll
        for (int j = 0; j < 6; ++j) zb[j] = c[kTzc + j];
        trim_residual_jacobian(t, o.lateral, zb, sens, rb, Jb);
        const float cost = trim_cost(o, rb);
        const float best = c[kTcost];
        float lam = c[kTlam];
        if (cost < best) {  // (false for NaN)
#pragma unroll
            for (int j = 0; j < 6; ++j) { c[kTzb + j] = zb[j]; c[kTrb + j] = rb[j]; }
#pragma unroll
            for (int k = 0; k < 36; ++k) c[kTJb + k] = Jb[k];
            c[kTcost] = cost;
            lam = fmaxf(lam * (1.0f / 3.0f), kTrimLambdaMin);
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) { zb[j] = c[kTzb + j]; rb[j] = c[kTrb + j]; }
#pragma unroll
            for (int k = 0; k < 36; ++k) Jb[k] = c[kTJb + k];
            lam = fminf(lam * 4.0f, kTrimLambdaMax);
            if (!(best <= 3.0e38f)) flag = (float)AC_TRIM_NONFINITE;  // not one finite evaluation: nothing to step from
        }
        if (flag == kTrimActive && trim_converged(o, rb)) flag = (float)AC_TRIM_CONVERGED;
        if (flag == kTrimActive) {
            if (last) {
                status = trim_final_status(o, zb, rb, Jb);
            } else {
                float zn[6];
                trim_step(o, zb, rb, Jb, lam, zn);
#pragma unroll
                for (int j = 0; j < 6; ++j) c[kTzc + j] = zn[j];
            }
        } else {
            c[kTflag] = flag;
            status = (int)flag;
        }
        c[kTlam] = lam;
#pragma unroll
        for (int j = 0; j < 6; ++j) { zo[j] = zb[j]; ro[j] = rb[j]; }
        return;
    }
    status = (int)flag;
    if (last) {
#pragma unroll
        for (int j = 0; j < 6; ++j) { zo[j] = c[kTzb + j]; ro[j] = c[kTrb + j]; }
    }
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// (defined in an_inst_trim.hip only; declared for the ABI unit)
__global__ void k_trim_assemble(const ac_trim_opts o, const float* __restrict__ target, const float* __restrict__ Uhold,
                                const float* __restrict__ Z0, long n, int init, float* __restrict__ X, float* __restrict__ U,
                                float* __restrict__ St);
__global__ void k_trim_update(const ac_trim_opts o, const float* __restrict__ target, const float* __restrict__ Uhold,
                              const float* __restrict__ Xd, const float* __restrict__ Fx, const float* __restrict__ Fu, long n,
                              int last, float* __restrict__ St, float* __restrict__ Xo, float* __restrict__ Uo,
                              float* __restrict__ Zo, float* __restrict__ Ro, int* __restrict__ status);
#ifdef AC_TRIM_INSTANTIATE
__global__ __launch_bounds__(kTrimBlock) void k_trim_assemble(const ac_trim_opts o, const float* __restrict__ target,
                                                              const float* __restrict__ Uhold, const float* __restrict__ Z0,
                                                              long n, int init, float* __restrict__ X, float* __restrict__ U,
                                                              float* __restrict__ St) {
    const long i = (long)blockIdx.x * kTrimBlock + threadIdx.x;
    if (i >= n) return;
    const TrimTarget t = trim_target(target, n, i);
    const TrimCol c{St + i, n};
    float uh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) uh[k] = Uhold[(3 + k) * n + i];
    if (init) {
        float z0[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) z0[j] = Z0[j * n + i];
        trim_init_unit(o, t, uh, z0, c);
    }
    float x[13], u[7];
    if (!trim_assemble_unit(o, t, uh, c, init != 0, x, u)) return;
#pragma unroll
    for (int k = 0; k < 13; ++k) X[k * n + i] = x[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) U[k * n + i] = u[k];
}

__global__ __launch_bounds__(kTrimBlock) void k_trim_update(const ac_trim_opts o, const float* __restrict__ target,
                                                            const float* __restrict__ Uhold, const float* __restrict__ Xd,
                                                            const float* __restrict__ Fx, const float* __restrict__ Fu, long n,
                                                            int last, float* __restrict__ St, float* __restrict__ Xo,
                                                            float* __restrict__ Uo, float* __restrict__ Zo,
                                                            float* __restrict__ Ro, int* __restrict__ status) {
    const long i = (long)blockIdx.x * kTrimBlock + threadIdx.x;
    if (i >= n) return;
    const TrimTarget t = trim_target(target, n, i);
    const TrimCol c{St + i, n};
    const TrimSens s{Xd + i, Fx + i, Fu + i, n};
    float z[6], r[6];
    int st = AC_TRIM_MAXITER;
    trim_update_unit(o, t, s, c, last != 0, z, r, st);
    if (!last) return;
    float uh[4], x[13], u[7];
#pragma unroll
    for (int k = 0; k < 4; ++k) uh[k] = Uhold[(3 + k) * n + i];
    trim_assemble(t, o.lateral, z, uh, x, u);
#pragma unroll
    for (int k = 0; k < 13; ++k) Xo[k * n + i] = x[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) Uo[k * n + i] = u[k];
#pragma unroll
    for (int j = 0; j < 6; ++j) { Zo[j * n + i] = z[j]; Ro[j * n + i] = r[j]; }
    status[i] = st;
}
#endif  // AC_TRIM_INSTANTIATE
}  // namespace ac
#endif  // AC_HOST_CHECK
