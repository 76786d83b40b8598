// ac_ukf.hpp — batched unscented Kalman filter beside the EKF bank (ac_ukf_step_f32, ac_ukf_filter_f32).
// The EKF's error state, chart ([+] ekf_inject, [-] rts_minus), measurement rows (ekf_measure<false>), diagonal Qd, Rd and
// mask / NaN rule (ac_ekf.hpp, ac_rts.hpp); no Jacobian is read.
//
// kappa >= 0:  gamma = sqrt(12 + kappa),  w0 = kappa / (12 + kappa),  w1 = 1 / (2 (12 + kappa)) for the 24 other points.
// Points are numbered 0 (centre), 1 + j (+gamma L.j), 13 + j (-gamma L.j), j = 0 .. 11.
// Time update:    L L' = P (plain Cholesky);  chi_j = x [+] (+-gamma L.j), stored with the position rows RELATIVE to p^ (p
//                 never enters f, ac_step_vjp_f32: the images then carry the position increments at full precision);
//                 the handle's forward step over the 25 n units;  e_j = F(chi_j) [-] F(chi_0) (e_0 = 0),  dbar = sum w_j e_j,
//                 x- = F(chi_0) [+] dbar with p^ added back,  d_j = e_j - dbar,  P- = sum w_j d_j d_j' + diag(Qd);
//                 Abar = D L^-1 with D.j = (e_+j - e_-j) / (2 gamma): the statistical linearisation Cov(d+, d) P^-1.
// Measurement:    L- L-' = P-;  z_j = h(x- [+] (+-gamma L-.j)),  zbar = sum w_j z_j,  Pzz = sum w_j (z_j - zbar)(z_j - zbar)' +
//                 diag(Rd) with an unused row replaced by a unit row,  Pzx = Y L-' with Y.j = (z_+j - z_-j) / (2 gamma);
//                 L_S L_S' = Pzz column by column, the innovation z - zbar carried as a sixteenth row: that row of the factor
//                 is w = L_S^-1 (z - zbar);  Yx' = L_S^-1 Pzx,  d = Yx w,  P = P- - Yx Yx',  x+ = x- [+] d (x- itself, bit for
//                 bit, when no row was applied).
// Outputs as the EKF's: S_i = the pivot of row i (the innovation variance given the rows before it), nu_i = the residual
// of row i before it is divided by L_S,ii (= L_S,ii w_i), nis = sum w_i^2, ll = -1/2 sum (log 2 pi S_i + w_i^2).
// Every product that enters P- , Pzz and P is commutative and every sum runs in a fixed order: the three are symmetric bit
// for bit, and an instance's bits depend neither on n nor on where it sits in the batch.  No atomics.
//
// Kernels (ukf_inst.hip), both with k_ekf_step's mapping (one instance per 16-lane group, sixteen per workgroup, lane r owns
// row r):
//   k_ukf_sigma            factor P, the 25 points and the replicated controls into the workspace, L and a flag beside them
//   k_ukf_update<PREDICT>  everything after the forward step; the measurement points live in registers, their images in LDS
// The per-lane code is shared with the host build (tests/host_ukf, -DAC_HOST_CHECK), which runs the 16 lanes of a group one
// after the other, phase by phase: a phase reads from the mirrors only what an EARLIER phase wrote (or the lane itself).
#pragma once
#include "ac_rts.hpp"

namespace ac {

constexpr int kUkfPts = 25;       // sigma points per instance
constexpr int kUkfGroups = kEkfGroups;
constexpr int kUkfZs = 17;        // row stride of the z and Pzz mirrors (odd: the lanes of a group on distinct banks)
constexpr long kUkfUnitFloats = 13 + 7 + 13;                     // point | controls | image, per step unit
constexpr long kUkfInstFloats = kUkfPts * kUkfUnitFloats + 145;  // ... and L [12][12], flag per instance

constexpr int AC_UKF_NOT_PD = 4;  // a pivot of the factor of P or of P- was <= 0 or not finite

struct UkfWeights {
    float gamma, w0, w1, i2g;  // i2g = 1 / (2 gamma)
};

// formed once on the host (IEEE sqrt and division), passed to the kernels by value
inline UkfWeights ukf_weights(float kappa) {
    UkfWeights w;
    const float c = 12.0f + kappa;
    w.gamma = sqrtf(c);
    w.w0 = kappa / c;
    w.w1 = 1.0f / (2.0f * c);
    w.i2g = 1.0f / (2.0f * w.gamma);
    return w;
}

// ---- k_ukf_sigma ------------------------------------------------------------------------------------------------------------------
struct UkfSigIo {
    const float *X, *P, *U;  // [13][n], [12][12][n], [7][n]
    float *Xw, *Uw;          // [13][25 n], [7][25 n]: unit j n + i is point j of instance i
    float* Lw;               // [12][12][n]: L, zero above the diagonal
    int* flag;               // [n]: 1 when a pivot of P's factor failed (the 25 units are then all x^)
    long n;
};

struct UkfSigShared {
    float m[kEkfLanes][kEkfLd];  // P, then L below its diagonal
    float pad[32];               // 240 dwords = 16 mod 32 banks
};
static_assert(sizeof(UkfSigShared) / 4 % 32 == 16, "UkfSigShared: neighbouring groups on disjoint LDS banks");

struct UkfSigLane {
    float l[12];  // row r of L
    bool pivbad;
};

// gamma times column c of the factor whose strict lower triangle is in m and whose diagonal entry of row c is dg (c < 12)
AC_DI void ukf_column(const float (&m)[kEkfLanes][kEkfLd], float dg, float gamma, int c, float dl[12]) {
    AC_EKF_FP
#pragma unroll
    for (int k = 0; k < 12; ++k) dl[k] = k < c ? 0.f : gamma * (k == c ? dg : m[k][c]);
}

template <class G>
AC_DI void ukf_sigma_group(G& grp, UkfSigShared& s, const UkfWeights& w, const UkfSigIo& io, long i, bool store) {
    AC_EKF_FP
    const long n = io.n, n25 = kUkfPts * io.n;
    grp.each([&](UkfSigLane& L, int r) AC_EKF_INLINE {
        const int rr = r < kEkfN ? r : 0;
#pragma unroll
        for (int j = 0; j < 12; ++j) s.m[r][j] = io.P[(rr * 12 + j) * n + i];
        L.pivbad = false;
    });
    // ---- L L' = P, column by column (ac_group.hpp; 1 / L_jj is not kept) ----------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        grp.each([&](UkfSigLane& L, int r) AC_EKF_INLINE {
            float iv;
            grp_chol_column(s.m, L.l, r, j, iv, L.pivbad);
        });
    }
    grp.each([&](UkfSigLane& L, int r) AC_EKF_INLINE {
        if (store && r < kEkfN) {
#pragma unroll
            for (int j = 0; j < 12; ++j) io.Lw[(r * 12 + j) * n + i] = j <= r ? L.l[j] : 0.f;
        }
        if (store && r == 0) io.flag[i] = L.pivbad ? 1 : 0;
        if (r > kEkfN) return;  // lanes 0-11: the points +-r; lane 12: the centre
        float xh[13], u[7], dl[12], dg = 0.f;
#pragma unroll
        for (int k = 0; k < 13; ++k) xh[k] = io.X[k * n + i];
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = io.U[k * n + i];
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j == r) dg = L.l[j];
        ukf_column(s.m, dg, w.gamma, r < kEkfN ? r : 0, dl);
        const bool centre = r == kEkfN || L.pivbad;
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
            if (sg == 1 && r == kEkfN) break;
            float xo[13];
            ekf_inject(xh, dl, xo);
#pragma unroll
            for (int k = 0; k < 13; ++k) xo[k] = k < 3 ? (centre ? 0.f : dl[k]) : (centre ? xh[k] : xo[k]);
            const long col = (r == kEkfN ? 0 : sg ? 13 + r : 1 + r) * n + i;
            if (store) {
#pragma unroll
                for (int k = 0; k < 13; ++k) io.Xw[k * n25 + col] = xo[k];
#pragma unroll
                for (int k = 0; k < 7; ++k) io.Uw[k * n25 + col] = u[k];
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) dl[k] = -dl[k];
        }
    });
}

// ---- k_ukf_update -----------------------------------------------------------------------------------------------------------------
struct UkfIo {
    const float *X, *P;      // [13][n], [12][12][n]: the estimate
    const float *Fw, *Lw;    // [13][25 n], [12][12][n]: the images of the points and P's factor (prediction only)
    const int* flag;         // [n] (prediction only)
    const float *Z, *Qd, *Rd;
    const int* mask;         // [n] or NULL (all rows)
    const float* ll_in;      // [n] or NULL: added to this step's log-likelihood
    float *Xo, *Po;
    float *nu, *S, *nis, *ll;
    int *used, *status;
    float *Xpred, *Ppred, *Abar;
    long n;
};

struct UkfShared {
    union {
        float e[kUkfPts][kEkfLd];      // e_j, then d_j (time update)
        float z[kUkfPts][kUkfZs];      // z_j, then z_j - zbar
        float ms[kEkfLanes][kUkfZs];   // Pzz over the innovation row, then L_S below its diagonal over w
    } a;
    union {
        float m[kEkfLanes][kEkfLd];    // L | P-, then L- below its diagonal | Pzx
        float yx[kEkfN][kUkfZs];       // Yx
    } b;
    float v[kEkfLanes];    // dbar | zbar | d
    float dg[kEkfLanes];   // the diagonal of L-
    float red[kEkfLanes];  // per-lane flags of a reduction
    float pad[7];          // 688 dwords = 16 mod 32 banks: the two groups of a 32-lane half never share a bank
};
static_assert(sizeof(UkfShared) / 4 % 32 == 16, "UkfShared: neighbouring groups on disjoint LDS banks");

// What lane r of a group keeps in registers.  xm, inv, the flags and the bit sets are the same in every lane of the group.
struct UkfLane {
    float pm[12];    // row r of P-
    float l[12];     // row r of L, then of L-
    float base[13];  // F(chi_0)
    float xm[13];    // x-
    float s[15];     // row r of Pzz (lane 15: z - zbar), column by column row r of L_S (lane 15: w)
    float inv[15];   // 1 / L_S,cc
    float pzx[12];   // row r of Pzx
    float yx[15];    // row r of Yx
    float rd;        // Rd of row r
    float nis, ll;
    int usedbits, okbits;
    bool sigbad, xfin, go, pmbad, predok, rejected;
};

// One filter step of instance i.  G: the group (device: one lane and a barrier after every phase; host: a loop over the
// lanes).  PREDICT false: the measurement update alone at (x, P) (Abar = I; Fw, Lw, flag, Qd are not read).
template <bool PREDICT, class G>
AC_DI void ukf_update_group(G& grp, UkfShared& s, const ac_ukf_opts& o, const UkfWeights& w, float eps, const UkfIo& io, long i,
                            bool store) {
    AC_EKF_FP
    const long n = io.n, n25 = kUkfPts * io.n;
    // ---- e_j = F(chi_j) [-] F(chi_0): lane r the points 1 + r and 17 + r; row r of L ----------------------------------------------
    if (PREDICT) {
        grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
            const int rr = r < kEkfN ? r : 0;
#pragma unroll
            for (int k = 0; k < 13; ++k) L.base[k] = io.Fw[k * n25 + i];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = 1 + r + 16 * q;
                if (j < kUkfPts) {
                    float f[13], e[12];
#pragma unroll
                    for (int k = 0; k < 13; ++k) f[k] = io.Fw[k * n25 + j * n + i];
                    rts_minus(f, L.base, e);
#pragma unroll
                    for (int k = 0; k < 12; ++k) s.a.e[j][k] = e[k];
                }
            }
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                L.l[j] = io.Lw[(rr * 12 + j) * n + i];
                s.b.m[r][j] = L.l[j];
            }
            L.sigbad = io.flag[i] != 0;
        });
        // ---- dbar_r, d_j[r] = e_j[r] - dbar_r, row r of D and of Abar = D L^-1 ---------------------------------------------------------
        grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
            if (r >= kEkfN) return;
            float D[12], ab[12], sum = 0.f;
#pragma unroll
            for (int j = 1; j < kUkfPts; ++j) sum += s.a.e[j][r];
            const float db = w.w1 * sum;
#pragma unroll
            for (int j = 0; j < 12; ++j) D[j] = (s.a.e[1 + j][r] - s.a.e[13 + j][r]) * w.i2g;
            s.a.e[0][r] = -db;
#pragma unroll
            for (int j = 1; j < kUkfPts; ++j) s.a.e[j][r] = s.a.e[j][r] - db;
            s.v[r] = db;
            // a L = D, from the last column back
#pragma unroll
            for (int j = 11; j >= 0; --j) {
                float t = D[j];
#pragma unroll
                for (int c = 11; c > j; --c) t = fmaf(-ab[c], s.b.m[c][j], t);
                ab[j] = t / s.b.m[j][j];
            }
            if (store && io.Abar) {
#pragma unroll
                for (int j = 0; j < 12; ++j) io.Abar[(r * 12 + j) * n + i] = L.sigbad ? (j == r ? 1.0f : 0.f) : ab[j];
            }
        });
    }
    // ---- x- = F(chi_0) [+] dbar (p^ added back), row r of P- = sum w_j d_j d_j' + diag(Qd); are they finite? ------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
        const int rr = r < kEkfN ? r : 0;
        float xh[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) xh[k] = io.X[k * n + i];
        bool direct = !PREDICT;
        if (PREDICT) {
            direct = L.sigbad;
            float db[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) db[k] = s.v[k];
            ekf_inject(L.base, db, L.xm);
#pragma unroll
            for (int k = 0; k < 3; ++k) L.xm[k] += xh[k];
            const float d0r = s.a.e[0][rr];
#pragma unroll
            for (int c = 0; c < 12; ++c) {
                float acc = 0.f;
#pragma unroll
                for (int j = 1; j < kUkfPts; ++j) acc = fmaf(s.a.e[j][rr], s.a.e[j][c], acc);
                float v = fmaf(w.w0, d0r * s.a.e[0][c], w.w1 * acc);
                if (c == r) v += io.Qd[c * n + i];
                L.pm[c] = v;
            }
        }
        if (direct) {
#pragma unroll
            for (int k = 0; k < 13; ++k) L.xm[k] = xh[k];
#pragma unroll
            for (int c = 0; c < 12; ++c) L.pm[c] = io.P[(rr * 12 + c) * n + i];
        }
        bool xf = true, pf = true;
#pragma unroll
        for (int k = 0; k < 13; ++k) xf = xf && ekf_finite(L.xm[k]);
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            pf = pf && ekf_finite(L.pm[c]);
            s.b.m[r][c] = L.pm[c];
        }
        L.xfin = xf;
        s.red[r] = (r < kEkfN && !pf) ? 1.0f : 0.f;
        if (!PREDICT) L.sigbad = false;
        if (store && r < kEkfN) {
#pragma unroll
            for (int c = 0; c < 12; ++c) {
                if (io.Ppred) io.Ppred[(r * 12 + c) * n + i] = L.pm[c];
                if (!PREDICT && io.Abar) io.Abar[(r * 12 + c) * n + i] = c == r ? 1.0f : 0.f;
            }
        }
        if (store && r == 0 && io.Xpred) {
#pragma unroll
            for (int k = 0; k < 13; ++k) io.Xpred[k * n + i] = L.xm[k];
        }
        L.pmbad = false;
        L.rd = io.Rd[(r < kEkfZ ? r : 0) * n + i];
    });
    // ---- L- L-' = P-, column by column (ac_group.hpp) ---------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
            if (j == 0) {
                bool ok = L.xfin;
#pragma unroll
                for (int k = 0; k < kEkfN; ++k) ok = ok && s.red[k] == 0.f;
                L.predok = ok;
            }
            float iv;
            grp_chol_column(s.b.m, L.l, r, j, iv, L.pmbad);
            if (r == j) s.dg[j] = L.l[j];
        });
    }
    // ---- z_j = h(x- [+] (+-gamma L-.j)): lanes 0-11 the points +-r, lane 12 the centre ---------------------------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
        L.go = L.predok && !L.sigbad && !L.pmbad;
        int zf = 0;
#pragma unroll
        for (int k = 0; k < kEkfZ; ++k) zf |= ekf_finite(io.Z[k * n + i]) ? (1 << k) : 0;
        L.usedbits = L.go ? (zf & (io.mask ? io.mask[i] : 0x7fff) & 0x7fff) : 0;
        if (r > kEkfN) return;
        float dl[12];
        ukf_column(s.b.m, s.dg[r < kEkfN ? r : 0], w.gamma, r < kEkfN ? r : 0, dl);
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
            if (sg == 1 && r == kEkfN) break;
            float xo[13];
            EkfMeas m;
            ekf_inject(L.xm, dl, xo);
            if (r == kEkfN) {
#pragma unroll
                for (int k = 0; k < 13; ++k) xo[k] = L.xm[k];
            }
            ekf_measure<false>(eps, o.mag_ned, xo, m);
            const int j = r == kEkfN ? 0 : sg ? 13 + r : 1 + r;
#pragma unroll
            for (int k = 0; k < kEkfZ; ++k) s.a.z[j][k] = m.h[k];
#pragma unroll
            for (int k = 0; k < 12; ++k) dl[k] = -dl[k];
        }
    });
    // ---- zbar_r, z_j[r] - zbar_r, row r of Y and of Pzx = Y L-' -------------------------------------------------------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
        if (r >= kEkfZ) return;
        float Y[12], sum = 0.f;
        const float z0 = s.a.z[0][r];  // the weights sum to 1: zbar = z_0 + w1 sum (z_j - z_0), exact for a row the points do not move
#pragma unroll
        for (int j = 1; j < kUkfPts; ++j) sum += s.a.z[j][r] - z0;
        const float zb = z0 + w.w1 * sum;
#pragma unroll
        for (int j = 0; j < 12; ++j) Y[j] = (s.a.z[1 + j][r] - s.a.z[13 + j][r]) * w.i2g;
#pragma unroll
        for (int j = 0; j < kUkfPts; ++j) s.a.z[j][r] = s.a.z[j][r] - zb;
        s.v[r] = zb;
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            float acc = Y[q] * s.dg[q];
#pragma unroll
            for (int j = q - 1; j >= 0; --j) acc = fmaf(Y[j], s.b.m[q][j], acc);
            L.pzx[q] = acc;
        }
    });
    // ---- row r of Pzz (an unused row is a unit row); lane 15: the innovation z - zbar ----------------------------------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
        if (r < kEkfZ) {
            const float z0r = s.a.z[0][r];
            const bool ur = (L.usedbits >> r) & 1;
#pragma unroll
            for (int c = 0; c < kEkfZ; ++c) {
                float acc = 0.f;
#pragma unroll
                for (int j = 1; j < kUkfPts; ++j) acc = fmaf(s.a.z[j][r], s.a.z[j][c], acc);
                float v = fmaf(w.w0, z0r * s.a.z[0][c], w.w1 * acc);
                if (c == r) v += L.rd;
                const bool uc = (L.usedbits >> c) & 1;
                L.s[c] = (ur && uc) ? v : (c == r ? 1.0f : 0.f);
            }
        } else {
#pragma unroll
            for (int c = 0; c < kEkfZ; ++c) L.s[c] = ((L.usedbits >> c) & 1) ? io.Z[c * n + i] - s.v[c] : 0.f;
        }
    });
    // ---- the rows into their mirrors (the z mirror is no longer read) ------------------------------------------------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
#pragma unroll
        for (int c = 0; c < kEkfZ; ++c) s.a.ms[r][c] = L.s[c];
        if (r < kEkfZ) {
#pragma unroll
            for (int q = 0; q < 12; ++q) s.b.m[r][q] = L.pzx[q];
        }
        L.okbits = 0;
        L.rejected = false;
        L.nis = 0.f;
        L.ll = 0.f;
    });
    // ---- L_S L_S' = Pzz in row order; the sixteenth row becomes w; nu, S, nis, ll (lane 15) -----------------------------------------------
#pragma unroll
    for (int c = 0; c < kEkfZ; ++c) {
        grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
            float t = L.s[c], d = s.a.ms[c][c];
#pragma unroll
            for (int k = 0; k < c; ++k) {
                const float lk = s.a.ms[c][k];
                t = fmaf(-L.s[k], lk, t);
                d = fmaf(-lk, lk, d);
            }
            const bool used = (L.usedbits >> c) & 1;
            const bool ok = used && d > 0.f && d <= kEkfFltMax;
            if (used && !ok) L.rejected = true;
            const float iv = ok ? 1.0f / sqrtf(d) : 0.f;
            const float lc = ok ? t * iv : 0.f;
            L.inv[c] = iv;
            L.s[c] = lc;
            if (r > c) s.a.ms[r][c] = lc;
            if (ok) L.okbits |= 1 << c;
            if (r == 15) {
                if (ok) {
                    const float e = lc * lc;
                    L.nis += e;
                    L.ll += logf(d) + kEkfLog2Pi + e;
                }
                if (store) {
                    if (io.nu) io.nu[c * n + i] = used ? t : 0.f;
                    if (io.S) io.S[c * n + i] = used ? d : 0.f;
                }
            }
        });
    }
    // ---- row r of Yx: column r of Yx' = L_S^-1 Pzx by a forward solve ------------------------------------------------------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
        const int rr = r < kEkfN ? r : 0;
#pragma unroll
        for (int q = 0; q < kEkfZ; ++q) {
            float t = s.b.m[q][rr];
#pragma unroll
            for (int k = 0; k < q; ++k) t = fmaf(-s.a.ms[q][k], L.yx[k], t);
            L.yx[q] = ((L.okbits >> q) & 1) ? t * L.inv[q] : 0.f;
        }
    });
    // ---- Yx into its mirror; element r of d = Yx w --------------------------------------------------------------------------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < kEkfZ; ++q) acc = fmaf(L.yx[q], s.a.ms[15][q], acc);
        s.v[r] = acc;
        if (r < kEkfN) {
#pragma unroll
            for (int q = 0; q < kEkfZ; ++q) s.b.yx[r][q] = L.yx[q];
        }
    });
    // ---- P = P- - Yx Yx', x+ = x- [+] d and the by-products ---------------------------------------------------------------------------------
    grp.each([&](UkfLane& L, int r) AC_EKF_INLINE {
        const bool moved = L.okbits != 0;
        float dl[12], xo[13];
#pragma unroll
        for (int k = 0; k < 12; ++k) dl[k] = s.v[k];
        ekf_inject(L.xm, dl, xo);
        if (store && r < kEkfN) {
#pragma unroll
            for (int c = 0; c < 12; ++c) {
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < kEkfZ; ++q) acc = fmaf(L.yx[q], s.b.yx[c][q], acc);
                io.Po[(r * 12 + c) * n + i] = moved ? L.pm[c] - acc : L.pm[c];
            }
        }
        if (store) {
#pragma unroll
            for (int k = 0; k < 13; ++k)
                if (r == k) io.Xo[k * n + i] = moved ? xo[k] : L.xm[k];
        }
        if (store && r == 15) {
            if (io.nis) io.nis[i] = L.nis;
            const float ll = moved ? -0.5f * L.ll : 0.f;
            if (io.ll) io.ll[i] = io.ll_in ? io.ll_in[i] + ll : ll;
            if (io.used) io.used[i] = L.usedbits;
            if (io.status)
                io.status[i] = (L.rejected ? AC_EKF_REJECTED : 0) | (L.predok ? 0 : AC_EKF_NONFINITE) |
                               ((L.sigbad || (L.predok && L.pmbad)) ? AC_UKF_NOT_PD : 0);
        }
    });
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launchers (defined in ukf_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; none allocates or
// synchronises.  `grid`, `lds` receive the launch dimension and the static LDS (ac_last_launch).
hipError_t ukf_launch_sigma(const UkfWeights& w, const UkfSigIo& io, hipStream_t st, int* grid, int* lds);
hipError_t ukf_launch_update(const ac_ukf_opts& o, const UkfWeights& w, float eps, const UkfIo& io, hipStream_t st, int* grid, int* lds);
}  // namespace ac
#endif
