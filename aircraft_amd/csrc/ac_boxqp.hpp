// ac_boxqp.hpp — the 7-variable box-constrained QP of the control-limited Riccati pass (Tassa, Mansard, Todorov,
// "Control-limited differential dynamic programming", ICRA 2014), by projected Newton:
//
//     min_x  1/2 x'Q x + q'x     subject to   lo <= x <= hi          (Q symmetric positive definite, fp32 throughout)
//
//   x <- clip(0, lo, hi);  then per iteration, with g = q + Q x:
//     clamped set  c = { i : pinned_i  or  (x_i == lo_i and g_i > 0)  or  (x_i == hi_i and g_i < 0) },  pinned_i = lo_i >= hi_i
//     stop         when c repeats after a FULL step (alpha = 1 and nothing was clipped: x is the minimiser of its face, and the
//                  signs of g on c are the KKT conditions)
//     direction    d_f = -Q_ff^-1 g_f on the free block, d_c = 0: clamped rows and columns of Q are replaced by unit ones and the
//                  clamped right-hand-side entries by zeros, so the ordinary 7 x 7 Cholesky and its two triangular solves serve
//     line search  x(alpha) = clip(x + alpha d), alpha = 1, 1/2, ..: accepted when the decrease  g's + 1/2 s'Q s  (s = x(alpha) - x,
//                  evaluated from s, not as a difference of two objective values) is <= kBoxQpArmijo g's   (projected Armijo)
//   Caps: kBoxQpIters Newton iterations, kBoxQpHalvings halvings.  When one is hit the last iterate stays — it is feasible and
//   no worse than the start — and `capped` says so.
//
// Everything is statically indexed (registers on the device, no scratch); the routine runs redundantly on every lane of the
// instance's wave, as the Cholesky of k_ilqr_backward does.  With -DAC_HOST_CHECK the header is plain host C++
// (tests/host_boxqp).
#pragma once
#include "ac_math.hpp"

namespace ac {

constexpr int kBoxQpIters = 16;      // Newton iterations (factorisations) at most
constexpr int kBoxQpHalvings = 12;   // halvings of alpha at most: 13 trial points per iteration
constexpr float kBoxQpArmijo = 0.1f;

// reciprocal square root: the hardware estimate plus one Newton step (full fp32 accuracy)
AC_DI float boxqp_rsqrt(float d) {
    float r = AC_RSQ(d);
    return r * fmaf(-0.5f * d * r, r, 1.5f);
}

// Q = L L' (lower triangle of L, reciprocal diagonal in rinv); pivots clamped at 1e-12
AC_DI void chol7(const float (&Q)[7][7], float (&L)[7][7], float (&rinv)[7]) {
#pragma unroll
    for (int m = 0; m < 7; ++m) {
        float d = Q[m][m];
#pragma unroll
        for (int p = 0; p < m; ++p) d = fmaf(-L[m][p], L[m][p], d);
        d = fmaxf(d, 1e-12f);
        rinv[m] = boxqp_rsqrt(d);
        L[m][m] = d * rinv[m];
#pragma unroll
        for (int i = m + 1; i < 7; ++i) {
            float s = Q[i][m];
#pragma unroll
            for (int p = 0; p < m; ++p) s = fmaf(-L[i][p], L[m][p], s);
            L[i][m] = s * rinv[m];
        }
    }
}

// in place: rhs <- (L L')^-1 rhs
AC_DI void chol7_solve(const float (&L)[7][7], const float (&rinv)[7], float (&rhs)[7]) {
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        float s = rhs[i];
#pragma unroll
        for (int p = 0; p < i; ++p) s = fmaf(-L[i][p], rhs[p], s);
        rhs[i] = s * rinv[i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        float s = rhs[i];
#pragma unroll
        for (int p = i + 1; p < 7; ++p) s = fmaf(-L[p][i], rhs[p], s);
        rhs[i] = s * rinv[i];
    }
}

// Q with the rows and columns of the set `c` (bit i = row i) replaced by unit ones
AC_DI void boxqp_mask(const float (&Q)[7][7], unsigned c, float (&Qm)[7][7]) {
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int m = 0; m < 7; ++m) Qm[i][m] = (((c >> i) | (c >> m)) & 1u) ? (i == m ? 1.f : 0.f) : Q[i][m];
}

struct BoxQp {
    float x[7];        // the solution; exactly lo_i or hi_i on a clamped row
    unsigned clamped;  // bit i: row i is clamped (pinned rows included)
    unsigned pinned;   // bit i: lo_i >= hi_i
    unsigned upper;    // bit i: x_i == hi_i (what a clamped, not pinned row sits on: the lower bound otherwise)
    int iters;         // Newton iterations taken
    int capped;        // 1: a cap ended the iteration
    // 0 free, -1 clamped at the lower bound, +1 at the upper bound, 2 pinned
    AC_DI int act(int i) const {
        return ((pinned >> i) & 1u) ? 2 : (((clamped >> i) & 1u) ? (((upper >> i) & 1u) ? 1 : -1) : 0);
    }
};

AC_DI void boxqp7(const float (&Q)[7][7], const float (&q)[7], const float (&lo)[7], const float (&hi)[7], BoxQp& r) {
    float x[7];
    unsigned pinned = 0u;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        x[i] = fminf(fmaxf(0.f, lo[i]), hi[i]);
        if (lo[i] >= hi[i]) pinned |= 1u << i;
    }
    unsigned prev = 0u, c = 0u;
    bool full = false;
    int it = 0, capped = 0;
    for (;;) {
        float g[7];
        c = pinned;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            float s = q[i];
#pragma unroll
            for (int m = 0; m < 7; ++m) s = fmaf(Q[i][m], x[m], s);
            g[i] = s;
            if ((x[i] == lo[i] && s > 0.f) || (x[i] == hi[i] && s < 0.f)) c |= 1u << i;
        }
        if (full && c == prev) break;
        if (it == kBoxQpIters) { capped = 1; break; }
        ++it;
        float d[7];
        {
            float Qm[7][7], L[7][7], rinv[7];
            boxqp_mask(Q, c, Qm);
            chol7(Qm, L, rinv);
#pragma unroll
            for (int i = 0; i < 7; ++i) d[i] = ((c >> i) & 1u) ? 0.f : g[i];
            chol7_solve(L, rinv, d);
#pragma unroll
            for (int i = 0; i < 7; ++i) d[i] = ((c >> i) & 1u) ? 0.f : -d[i];
        }
        float alpha = 1.f, xc[7];
        bool ok = false;
        for (int h = 0; h <= kBoxQpHalvings; ++h) {
            float s[7], gs = 0.f, sqs = 0.f;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                xc[i] = fminf(fmaxf(fmaf(alpha, d[i], x[i]), lo[i]), hi[i]);
                s[i] = xc[i] - x[i];
                gs = fmaf(g[i], s[i], gs);
            }
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                float t = 0.f;
#pragma unroll
                for (int m = 0; m < 7; ++m) t = fmaf(Q[i][m], s[m], t);
                sqs = fmaf(s[i], t, sqs);
            }
            if (fmaf(0.5f, sqs, gs) <= kBoxQpArmijo * gs) { ok = true; break; }
            alpha *= 0.5f;
        }
        if (!ok) { capped = 1; break; }
        full = alpha == 1.f;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            full = full && (xc[i] == x[i] + d[i]);
            x[i] = xc[i];
        }
        prev = c;
    }
    unsigned upper = 0u;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        r.x[i] = x[i];
        if (x[i] == hi[i]) upper |= 1u << i;
    }
    r.clamped = c; r.pinned = pinned; r.upper = upper; r.iters = it; r.capped = capped;
}

}  // namespace ac
