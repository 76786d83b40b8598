// ac_eig.hpp — batched eigenvalues of small real matrices and the flight modes of the trim linearisation (ac_eig_f32,
// ac_modes_f32).
//
// One instance: a real m x m matrix, 1 <= m <= 13.  Inputs and outputs are float32; the arithmetic between them is float64:
// the eigenvalue condition numbers of the flight blocks reach 28 .. 412, and a float32 chain (LAPACK's sgeev as much as this
// one) leaves 1e-6 .. 8e-5 in the eigenvalues where float64 leaves the rounding of the output, 6e-8.  The
// classic chain:
//   eig_balance   LAPACK gebal, both halves.  Permutation: a row whose off-diagonal part inside the window is exactly zero is
//                 exchanged to the bottom of the window, then a column to its top, repeatedly; their eigenvalues are read
//                 off the diagonal and the window [lo, hi] shrinks.  Scaling: row i / f, column i * f inside the window with f
//                 a power of two (exact), sweeps until no row/column pair improves (c + r) / f < 0.95 (c + r).
//   eig_hessenberg  Householder reflectors (EISPACK orthes) on the window; the reflector of a column is kept in that column
//                 below the subdiagonal while it is applied and zeroed afterwards.
//   eig_hqr       Francis implicit double-shift QR (EISPACK hqr) on the window: deflation |h(k,k-1)| <= eps (|h(k-1,k-1)| +
//                 |h(k,k)|) with eps = 2^-52 (the norm of the window where both diagonals are 0), the two-consecutive-small-
//                 subdiagonals start, exceptional shifts at the 10th and 20th iteration of an eigenvalue, at most max_iters
//                 iterations per eigenvalue; the closing 2 x 2 in the standard stable form: a real pair, or a conjugate
//                 pair whose real parts are the same bits and whose imaginary parts are +z, -z.
//   eig_sort      wr, wi are rounded to float32, then put in the canonical order: descending |lambda|^2 = wr^2 + wi^2 (float32,
//                 both products rounded), then descending imaginary
//                 part (the + member of a pair first), then descending real part.  The stored order is part of the contract.
// Status per instance: AC_EIG_OK; AC_EIG_MAXITER, the cap was reached: every output of the instance is NaN; AC_EIG_NONFINITE,
// an entry is not finite: outputs NaN, no iteration.  iters: QR iterations over all eigenvalues.
//
// Storage.  The routines index the matrix with run-time indices, so it must not be a private array (that would be scratch
// memory on the device).  They take a memory `S` of float64 words with operator[](int word): on the device word w of a
// lane's instance is the LDS word w * L + lane, L the instances of the workgroup (consecutive lanes on consecutive words), on
// the host a plain array.  Words [0, m*m): the matrix, row-major; then wr [m] and wi [m].  eig_words(m) = m*m + 2m.  L = 64
// while that fits 64 KiB (m <= 10: 40 KiB at m = 8, 60 KiB at m = 10), 32 beyond (48.75 KiB at m = 13).
//
// Kernels (modes_inst.hip), one instance per lane, one wave (or half a wave) per workgroup, no barrier and no cross-lane traffic: the code a
// lane runs is the host build's (tests/host_modes, -DAC_HOST_CHECK -ffp-contract=off), so an instance's bits depend neither
// on n nor on where it sits in the batch.  Lanes whose instance has finished wait, masked, for the wave's slowest.
//   k_eig        M [m][m][n] -> wr, wi [m][n], status, iters
//   k_modes_eig  A_xi (and B_xi, K) -> a copy of A_xi with the entries [flight rows][columns 0, 1, 2, 8] set to exactly 0 (they
//                are 0 by the translation and yaw invariance of the dynamics; the float32 projection leaves 1e-6 there, and
//                the permutation step needs the exact zeros), minus B_xi K, the rows and columns of `coords` -> eigenvalues
//                (float32 out) and from those s = log(lambda) / dt in float32 as sigma = log1p((wr - 1)(wr + 1) + wi^2) / (2 dt), omega = atan2(wi, wr) / dt.
// AC_EIG_FP opens every function body: no contraction beyond the fmaf calls that are written out (ac_ekf.hpp).
#pragma once
#include "ac_math.hpp"
#include "../../include/aircraft_hip.h"

#ifdef AC_HOST_CHECK
#define AC_EIG_FP
#else
#define AC_EIG_FP _Pragma("clang fp contract(off)")
#endif

namespace ac {

constexpr int kEigMaxM = 13;
constexpr int kEigLanes = 64;            // lanes of a workgroup of k_eig and k_modes_eig: one wave
constexpr int kEigDefaultIters = 30;
constexpr double kEigEps = 2.220446049250313e-16;  // 2^-52
constexpr float kEigFltMax = 3.0e38f;
constexpr unsigned kModesFlight = 0xEF8u;  // chart coordinates 3-7, 9-11
constexpr long kModesWsFloats = 13 + 169 + 91 + 144 + 84;  // x+ | A | B | A_xi | B_xi per instance

constexpr int AC_EIG_OK = 0;
constexpr int AC_EIG_MAXITER = 1;
constexpr int AC_EIG_NONFINITE = 3;

constexpr int eig_words(int m) { return m * m + 2 * m; }  // per instance
// instances per workgroup: a full wave while its words fit 64 KiB of LDS (m <= 10), half a wave beyond
constexpr int eig_lanes(int m) { return m <= 10 ? kEigLanes : kEigLanes / 2; }
constexpr int eig_lds_bytes(int m) { return eig_words(m) * eig_lanes(m) * (int)sizeof(double); }  // per workgroup

// One instance's column of a [rows][n] array (element w at b[w * s]).
struct EigCol {
    float* b;
    long s;
    AC_DI float& operator[](int w) const { return b[(long)w * s]; }
};
struct EigCCol {
    const float* b;
    long s;
    AC_DI float operator[](int w) const { return b[(long)w * s]; }
};

AC_DI double eig_sign(double a, double b) { return b < 0.0 ? -fabs(a) : fabs(a); }

// exchange rows j and k and columns j and k (a permutation similarity)
template <class S>
AC_DI void eig_exchange(S& a, int m, int j, int k) {
    AC_EIG_FP
    if (j == k) return;
    for (int c = 0; c < m; ++c) {
        const double t = a[j * m + c];
        a[j * m + c] = a[k * m + c];
        a[k * m + c] = t;
    }
    for (int r = 0; r < m; ++r) {
        const double t = a[r * m + j];
        a[r * m + j] = a[r * m + k];
        a[r * m + k] = t;
    }
}

// gebal: afterwards rows hi+1 .. m-1 and columns 0 .. lo-1 are isolated (their eigenvalues stand on the diagonal) and the
// window [lo, hi] is scaled.  lo > hi never happens: the last isolated row leaves lo == hi == 0.0
template <class S>
AC_DI void eig_balance(S& a, int m, int& lo, int& hi) {
    AC_EIG_FP
    int k = 0, l = m - 1;
    // rows that isolate an eigenvalue go to the bottom of the window
    for (bool again = true; again && l > 0;) {
        again = false;
        for (int j = l; j >= 0; --j) {
            bool zero = true;
            for (int c = 0; c <= l; ++c) zero = zero && (c == j || a[j * m + c] == 0.0);
            if (zero) {
                eig_exchange(a, m, j, l);
                --l;
                again = true;
                break;
            }
        }
    }
    // columns that isolate an eigenvalue go to its top
    for (bool again = true; again && k < l;) {
        again = false;
        for (int j = k; j <= l; ++j) {
            bool zero = true;
            for (int r = k; r <= l; ++r) zero = zero && (r == j || a[r * m + j] == 0.0);
            if (zero) {
                eig_exchange(a, m, j, k);
                ++k;
                again = true;
                break;
            }
        }
    }
    lo = k;
    hi = l;
    // scaling by powers of two (at most 32 sweeps; f stays inside 2^+-62)
    bool noconv = true;
    for (int sweep = 0; noconv && sweep < 32; ++sweep) {
        noconv = false;
        for (int i = k; i <= l; ++i) {
            double c = 0.0, r = 0.0;
            for (int j = k; j <= l; ++j)
                if (j != i) {
                    c += fabs(a[j * m + i]);
                    r += fabs(a[i * m + j]);
                }
            if (c == 0.0 || r == 0.0) continue;
            double g = r * 0.5, f = 1.0;
            const double s = c + r;
            while (c < g && f < 4.0e18) {
                f *= 2.0;
                c *= 4.0;
            }
            g = r * 2.0;
            while (c >= g && f > 2.5e-19) {
                f *= 0.5;
                c *= 0.25;
            }
            if ((c + r) / f < 0.95 * s) {
                g = 1.0 / f;
                noconv = true;
                for (int j = 0; j < m; ++j) a[i * m + j] *= g;
                for (int j = 0; j < m; ++j) a[j * m + i] *= f;
            }
        }
    }
}

// orthes on the window: Householder reflectors, column by column
template <class S>
AC_DI void eig_hessenberg(S& a, int m, int lo, int hi) {
    AC_EIG_FP
    for (int c = lo + 1; c < hi; ++c) {
        double scale = 0.0;
        for (int i = c; i <= hi; ++i) scale += fabs(a[i * m + c - 1]);
        if (scale == 0.0) continue;
        double h = 0.0;
        for (int i = hi; i >= c; --i) {
            const double u = a[i * m + c - 1] / scale;
            a[i * m + c - 1] = u;
            h = fma(u, u, h);
        }
        const double uc = a[c * m + c - 1];
        const double g = -eig_sign(sqrt(h), uc);
        h -= uc * g;
        a[c * m + c - 1] = uc - g;
        // (I - u u' / h) A, columns c .. hi
        for (int j = c; j <= hi; ++j) {
            double f = 0.0;
            for (int i = hi; i >= c; --i) f = fma(a[i * m + c - 1], a[i * m + j], f);
            f /= h;
            for (int i = c; i <= hi; ++i) a[i * m + j] = fma(-f, a[i * m + c - 1], a[i * m + j]);
        }
        // A (I - u u' / h), rows lo .. hi
        for (int i = lo; i <= hi; ++i) {
            double f = 0.0;
            for (int j = hi; j >= c; --j) f = fma(a[j * m + c - 1], a[i * m + j], f);
            f /= h;
            for (int j = c; j <= hi; ++j) a[i * m + j] = fma(-f, a[j * m + c - 1], a[i * m + j]);
        }
        a[c * m + c - 1] = scale * g;
        for (int i = c + 1; i <= hi; ++i) a[i * m + c - 1] = 0.0;
    }
}

// hqr on the window [lo, hi] of an upper Hessenberg matrix -> wr, wi at words m*m + k, m*m + m + k; returns false when an
// eigenvalue took more than max_iters iterations.  `iters` receives the iterations used.
template <class S>
AC_DI bool eig_hqr(S& a, int m, int lo, int hi, int max_iters, int& iters) {
    AC_EIG_FP
    const int WR = m * m, WI = m * m + m;
    double norm = 0.0;
    for (int i = lo; i <= hi; ++i)
        for (int j = (i > lo ? i - 1 : lo); j <= hi; ++j) norm += fabs(a[i * m + j]);
    int en = hi;
    double t = 0.0;
    iters = 0;
    while (en >= lo) {
        int its = 0;
        for (;;) {
            // a single small subdiagonal entry
            int l = en;
            for (; l > lo; --l) {
                double s = fabs(a[(l - 1) * m + l - 1]) + fabs(a[l * m + l]);
                if (s == 0.0) s = norm;
                if (fabs(a[l * m + l - 1]) <= kEigEps * s) break;
            }
            double x = a[en * m + en];
            if (l == en) {  // one root
                a[WR + en] = x + t;
                a[WI + en] = 0.0;
                en -= 1;
                break;
            }
            double y = a[(en - 1) * m + en - 1];
            double w = a[en * m + en - 1] * a[(en - 1) * m + en];
            if (l == en - 1) {  // two roots
                const double p = 0.5 * (y - x);
                const double q = fma(p, p, w);
                double z = sqrt(fabs(q));
                x += t;
                if (q >= 0.0) {  // a real pair
                    z = p + eig_sign(z, p);
                    a[WR + en - 1] = x + z;
                    a[WR + en] = z != 0.0 ? x - w / z : x + z;
                    a[WI + en - 1] = 0.0;
                    a[WI + en] = 0.0;
                } else {  // a conjugate pair
                    a[WR + en - 1] = x + p;
                    a[WR + en] = x + p;
                    a[WI + en - 1] = z;
                    a[WI + en] = -z;
                }
                en -= 2;
                break;
            }
            if (its >= max_iters) return false;
            if (its == 10 || its == 20) {  // an exceptional shift
                t += x;
                for (int i = lo; i <= en; ++i) a[i * m + i] -= x;
                const double s = fabs(a[en * m + en - 1]) + fabs(a[(en - 1) * m + en - 2]);
                x = 0.75 * s;
                y = x;
                w = -0.4375 * s * s;
            }
            ++its;
            ++iters;
            // two consecutive small subdiagonal entries
            double p = 0.0, q = 0.0, r = 0.0, z;
            int k0 = en - 2;
            for (; k0 >= l; --k0) {
                z = a[k0 * m + k0];
                r = x - z;
                double s = y - z;
                p = (r * s - w) / a[(k0 + 1) * m + k0] + a[k0 * m + k0 + 1];
                q = a[(k0 + 1) * m + k0 + 1] - z - r - s;
                r = a[(k0 + 2) * m + k0 + 1];
                s = fabs(p) + fabs(q) + fabs(r);
                p /= s;
                q /= s;
                r /= s;
                if (k0 == l) break;
                const double u = fabs(a[k0 * m + k0 - 1]) * (fabs(q) + fabs(r));
                const double v = fabs(p) * (fabs(a[(k0 - 1) * m + k0 - 1]) + fabs(z) + fabs(a[(k0 + 1) * m + k0 + 1]));
                if (u <= kEigEps * v) break;
            }
            for (int i = k0 + 2; i <= en; ++i) {
                a[i * m + i - 2] = 0.0;
                if (i != k0 + 2) a[i * m + i - 3] = 0.0;
            }
            // the double QR step on rows l .. en and columns k0 .. en
            for (int k = k0; k <= en - 1; ++k) {
                const bool notlast = k != en - 1;
                if (k != k0) {
                    p = a[k * m + k - 1];
                    q = a[(k + 1) * m + k - 1];
                    r = notlast ? a[(k + 2) * m + k - 1] : 0.0;
                    x = fabs(p) + fabs(q) + fabs(r);
                    if (x == 0.0) continue;
                    p /= x;
                    q /= x;
                    r /= x;
                }
                const double s = eig_sign(sqrt(fma(p, p, fma(q, q, r * r))), p);
                if (k == k0) {
                    if (l != k0) a[k * m + k - 1] = -a[k * m + k - 1];
                } else {
                    a[k * m + k - 1] = -s * x;
                }
                p += s;
                x = p / s;
                y = q / s;
                z = r / s;
                q /= p;
                r /= p;
                for (int j = k; j <= en; ++j) {  // rows
                    double pp = fma(q, a[(k + 1) * m + j], a[k * m + j]);
                    if (notlast) {
                        pp = fma(r, a[(k + 2) * m + j], pp);
                        a[(k + 2) * m + j] = fma(-pp, z, a[(k + 2) * m + j]);
                    }
                    a[(k + 1) * m + j] = fma(-pp, y, a[(k + 1) * m + j]);
                    a[k * m + j] = fma(-pp, x, a[k * m + j]);
                }
                const int last = en < k + 3 ? en : k + 3;
                for (int i = l; i <= last; ++i) {  // columns
                    double pp = fma(y, a[i * m + k + 1], x * a[i * m + k]);
                    if (notlast) {
                        pp = fma(z, a[i * m + k + 2], pp);
                        a[i * m + k + 2] = fma(-pp, r, a[i * m + k + 2]);
                    }
                    a[i * m + k + 1] = fma(-pp, q, a[i * m + k + 1]);
                    a[i * m + k] -= pp;
                }
            }
        }
    }
    return true;
}

// true when (ar, ai) stands before (br, bi) in the canonical order
AC_DI bool eig_before(float ar, float ai, float br, float bi) {
    AC_EIG_FP
    const float a1 = ar * ar, a2 = ai * ai, b1 = br * br, b2 = bi * bi;
    const float ma = a1 + a2, mb = b1 + b2;
    if (ma != mb) return ma > mb;
    if (ai != bi) return ai > bi;
    return ar > br;
}

template <class S>
AC_DI void eig_sort(S& a, int m) {
    AC_EIG_FP
    const int WR = m * m, WI = m * m + m;
    for (int i = 1; i < m; ++i) {
        const float vr = (float)a[WR + i], vi = (float)a[WI + i];
        int j = i - 1;
        for (; j >= 0 && eig_before(vr, vi, (float)a[WR + j], (float)a[WI + j]); --j) {
            a[WR + j + 1] = a[WR + j];
            a[WI + j + 1] = a[WI + j];
        }
        a[WR + j + 1] = vr;
        a[WI + j + 1] = vi;
    }
}

// The eigenvalues of the matrix in words [0, m*m) of `a` (destroyed) -> wr, wi in words m*m .. in the canonical order.
// Returns the status; on AC_EIG_MAXITER and AC_EIG_NONFINITE wr and wi are NaN.
template <class S>
AC_DI int eig_solve(S& a, int m, int max_iters, int& iters) {
    AC_EIG_FP
    const int WR = m * m, WI = m * m + m;
    iters = 0;
    bool finite = true;
    for (int e = 0; e < m * m; ++e) finite = finite && fabs(a[e]) <= (double)kEigFltMax;
    int status = finite ? AC_EIG_OK : AC_EIG_NONFINITE;
    if (finite) {
        int lo, hi;
        eig_balance(a, m, lo, hi);
        for (int i = 0; i < m; ++i)
            if (i < lo || i > hi) {
                a[WR + i] = a[i * m + i];
                a[WI + i] = 0.0;
            }
        eig_hessenberg(a, m, lo, hi);
        if (!eig_hqr(a, m, lo, hi, max_iters, iters)) status = AC_EIG_MAXITER;
    }
    if (status == AC_EIG_OK) {
        // the outputs are float32: round, then order what is stored
        for (int i = 0; i < m; ++i) {
            a[WR + i] = (double)(float)a[WR + i];
            a[WI + i] = (double)(float)a[WI + i];
        }
        eig_sort(a, m);
    } else {
        const double nan = __builtin_nan("");
        for (int i = 0; i < m; ++i) {
            a[WR + i] = nan;
            a[WI + i] = nan;
        }
    }
    return status;
}

// k_eig's unit: one instance of M [m][m][n]
template <class S>
AC_DI void eig_unit(S& a, const EigCCol& M, int m, int max_iters, const EigCol& wr, const EigCol& wi, int* status, int* iters) {
    AC_EIG_FP
    for (int e = 0; e < m * m; ++e) a[e] = (double)M[e];
    int it;
    const int st = eig_solve(a, m, max_iters, it);
    for (int i = 0; i < m; ++i) {
        wr[i] = (float)a[m * m + i];
        wi[i] = (float)a[m * m + m + i];
    }
    *status = st;
    if (iters) *iters = it;
}

// s = log(lambda) / dt: sigma from log1p of |lambda|^2 - 1 = (wr - 1)(wr + 1) + wi^2 (|lambda| - 1 is about 1e-4 for the phugoid
// at dt = 0.01: log(hypot) would lose it), omega from atan2
AC_DI void modes_continuous(float wr, float wi, float dt, float& sigma, float& omega) {
    AC_EIG_FP
    const float d = fmaf(wr - 1.0f, wr + 1.0f, wi * wi);
    sigma = 0.5f * log1pf(d) / dt;
    omega = atan2f(wi, wr) / dt;
}

// k_modes_eig's unit: A_xi [12][12], B_xi [12][7], K [7][12] (NULL base: open loop) of one instance, `coords` the kept
// coordinates (m of them) -> wr, wi, sigma, omega [12] (rows >= m are 0), status, iters
template <class S>
AC_DI void modes_unit(S& a, const EigCCol& Axi, const EigCCol& Bxi, const EigCCol& K, unsigned coords, int m, int max_iters,
                      float dt, const EigCol& wr, const EigCol& wi, const EigCol& sigma, const EigCol& omega, int* status,
                      int* iters) {
    AC_EIG_FP
    constexpr unsigned kIgnorable = 0x107u;  // coordinates 0, 1, 2, 8
    int rr = 0;
    for (int r = 0; r < 12; ++r) {
        if (!((coords >> r) & 1u)) continue;
        int cc = 0;
        for (int c = 0; c < 12; ++c) {
            if (!((coords >> c) & 1u)) continue;
            double v = (double)Axi[r * 12 + c];
            // the flight rows do not depend on position and heading: exactly 0 (a NaN stays: the instance is non-finite)
            if (!((kIgnorable >> r) & 1u) && ((kIgnorable >> c) & 1u) && fabs(v) <= (double)kEigFltMax) v = 0.0;
            if (K.b) {
                double acc = 0.0;
                for (int j = 0; j < 7; ++j) acc = fma((double)Bxi[r * 7 + j], (double)K[j * 12 + c], acc);
                v -= acc;
            }
            a[rr * m + cc] = v;
            ++cc;
        }
        ++rr;
    }
    int it;
    const int st = eig_solve(a, m, max_iters, it);
    for (int i = 0; i < 12; ++i) {
        float r = 0.f, im = 0.f, sg = 0.f, om = 0.f;
        if (i < m) {
            r = (float)a[m * m + i];
            im = (float)a[m * m + m + i];
            modes_continuous(r, im, dt, sg, om);
        }
        wr[i] = r;
        wi[i] = im;
        sigma[i] = sg;
        omega[i] = om;
    }
    *status = st;
    if (iters) *iters = it;
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launchers (defined in modes_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; none allocates or
// synchronises.  `grid` and `lds` receive the launch dimension and the dynamic LDS request (ac_last_launch).
hipError_t eig_launch(const float* M, int m, int max_iters, long n, float* wr, float* wi, int* status, int* iters, hipStream_t st,
                      int* grid, int* lds);
hipError_t modes_launch_eig(const float* Axi, const float* Bxi, const float* K, unsigned coords, int m, int max_iters, float dt,
                            long n, float* wr, float* wi, float* sigma, float* omega, int* status, int* iters, hipStream_t st,
                            int* grid, int* lds);
}  // namespace ac
#endif
