// Gauss-Newton multiple shooting: k_shoot_direction, k_shoot_merit_weight, k_shoot_candidates, k_shoot_merit and their launchers
// (ac_shoot.hpp; the k_ilqr_backward_shoot kernels are in ilqr_backward_inst.hip).
#include "ac_shoot.hpp"

namespace ac {

// ---- direction: one wave per instance, sequential in k -------------------------------------------------------------------------
//   dx_0 = 0,  du_k = kff_k + K_k dx_k,  dx_{k+1} = A_k dx_k + B_k du_k + (F_k - x_{k+1}),  lam_k = Vx[k] + Vxx[k] dx_{k+1}
// with `clip`:  du_k = clip(U_k + kff_k + K_k dx_k, u_min, u_max) - U_k, so that (X + alpha dX, U + alpha dU) stays consistent to
// first order when the box binds (for a feasible U the candidates' clip then only trims roundings).
// Lane (j, g) = (t & 15, t >> 4) owns row j and the columns m = g, g + 4, g + 8, g + 12 of the row's products: a lane reads ~20
// floats per node (a lane per instance reads ~550 and is bound by issuing them: 25.6 ms at B = 64, H = 400 — DESIGN.md §4), all of
// them independent of dx, so node k + 1's are loaded before node k's arithmetic.  The partial products are summed across the four
// groups with two cross-lane adds; dx and du travel as each group's own four (two) entries, fetched from the owning lanes.
struct ShootNode {
    float kq[4], aq[4], bq[2], vq[4], kf, d, vx, u;
};

__global__ __launch_bounds__(64) void k_shoot_direction(const IlqrCost C, const float* __restrict__ X, const float* __restrict__ U,
                                                        const float* __restrict__ F, const float* __restrict__ A,
                                                        const float* __restrict__ Bm, const float* __restrict__ K,
                                                        const float* __restrict__ kff, const float* __restrict__ Vx,
                                                        const float* __restrict__ Vxx, int clip, long B, long H,
                                                        float* __restrict__ dX, float* __restrict__ dU, float* __restrict__ Lam) {
    const int t = threadIdx.x, j = t & 15, g = t >> 4;
    const long b = blockIdx.x;  // grid = B
    const bool row_x = j < 13, row_u = j < 7;
    float lo = C.u_min[0], hi = C.u_max[0];
#pragma unroll
    for (int q = 1; q < 7; ++q) { lo = (j == q) ? C.u_min[q] : lo; hi = (j == q) ? C.u_max[q] : hi; }
    auto load = [&](long k, ShootNode& n) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m = g + 4 * c;
            const bool on = m < 13;
            const int mm = on ? m : 12;
            n.kq[c] = (row_u && on) ? K[((k * 7 + j) * 13 + mm) * B + b] : 0.f;
            n.aq[c] = (row_x && on) ? A[((k * 13 + j) * 13 + mm) * B + b] : 0.f;
            n.vq[c] = (row_x && on && Lam != nullptr) ? Vxx[((k * 13 + j) * 13 + mm) * B + b] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int i = g + 4 * c;
            const bool on = i < 7;
            n.bq[c] = (row_x && on) ? Bm[((k * 13 + j) * 7 + (on ? i : 6)) * B + b] : 0.f;
        }
        n.kf = row_u ? kff[(k * 7 + j) * B + b] : 0.f;
        n.u = (row_u && clip) ? U[(k * 7 + j) * B + b] : 0.f;
        n.d = row_x ? F[(k * 13 + j) * B + b] - X[((k + 1) * 13 + j) * B + b] : 0.f;
        n.vx = (row_x && Lam != nullptr) ? Vx[(k * 13 + j) * B + b] : 0.f;
    };
    auto groups = [](float s) {  // the sum over the four lane groups, in every lane
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        return s;
    };
    if (row_x && g == 0) dX[(long)j * B + b] = 0.f;
    float dxg[4] = {0.f, 0.f, 0.f, 0.f};  // dx[g + 4 c]
    ShootNode cur, nxt;
    load(0, cur);
    nxt = cur;
    for (long k = 0; k < H; ++k) {
        if (k + 1 < H) load(k + 1, nxt);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) s = fmaf(cur.kq[c], dxg[c], s);
        s = groups(s);  // (every lane takes part in the cross-lane adds: never inside a select)
        float du = row_u ? cur.kf + s : 0.f;
        if (clip) du = row_u ? fminf(fmaxf(cur.u + du, lo), hi) - cur.u : 0.f;
        if (row_u && g == 0) dU[(k * 7 + j) * B + b] = du;
        float dug[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) dug[c] = __shfl(du, (t & 48) | ((g + 4 * c) & 15), 64);  // (row 7 holds 0)
        s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) s = fmaf(cur.aq[c], dxg[c], s);
#pragma unroll
        for (int c = 0; c < 2; ++c) s = fmaf(cur.bq[c], dug[c], s);
        s = groups(s);
        const float dxn = row_x ? cur.d + s : 0.f;
        if (row_x && g == 0) dX[((k + 1) * 13 + j) * B + b] = dxn;
#pragma unroll
        for (int c = 0; c < 4; ++c) dxg[c] = __shfl(dxn, (t & 48) | ((g + 4 * c) & 15), 64);  // (rows 13-15 hold 0)
        if (Lam != nullptr) {
            s = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) s = fmaf(cur.vq[c], dxg[c], s);
            s = groups(s);
            if (row_x && g == 0) Lam[(k * 13 + j) * B + b] = cur.vx + s;
        }
        cur = nxt;
    }
}

// ---- merit weight: mu[b] = max(mu[b], factor max |Lam[:, :, b]|) — never decreases ---------------------------------------------
__global__ __launch_bounds__(kBlock) void k_shoot_merit_weight(const float* __restrict__ Lam, float factor, long B, long H,
                                                               float* __restrict__ mu) {
    const long b = (long)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    float m = 0.f;
    for (long r = 0; r < H * 13; ++r) m = fmaxf(m, fabsf(Lam[r * B + b]));
    mu[b] = fmaxf(mu[b], factor * m);
}

// ---- candidates: column c = a B + b of Xc [H+1][13][na B], Uc [H][7][na B] -----------------------------------------------------
//   Xc = X + alpha_a dX (row block 0: X[0] itself),  Uc = clip(U + alpha_a dU, u_min, u_max);  blockIdx.y strides over the rows
__global__ __launch_bounds__(kBlock) void k_shoot_candidates(const IlqrCost C, const float* __restrict__ X,
                                                             const float* __restrict__ U, const float* __restrict__ dX,
                                                             const float* __restrict__ dU, const AlphaSet al, long B, long H,
                                                             float* __restrict__ Xc, float* __restrict__ Uc) {
    const long c = (long)blockIdx.x * kBlock + threadIdx.x;
    const long Bc = (long)al.n * B;
    if (c >= Bc) return;
    const long b = c % B;
    const int ai = (int)(c / B);
    float alpha = al.a[0];  // (selects, not an indexed read of the argument block)
#pragma unroll
    for (int q = 1; q < 8; ++q) alpha = (ai == q) ? al.a[q] : alpha;
    const long nx = (H + 1) * 13, nrows = nx + H * 7;
    for (long r = blockIdx.y; r < nrows; r += gridDim.y) {
        if (r < 13) {
            Xc[r * Bc + c] = X[r * B + b];
        } else if (r < nx) {
            Xc[r * Bc + c] = fmaf(alpha, dX[r * B + b], X[r * B + b]);
        } else {
            const long ru = r - nx;
            const int i = (int)(ru % 7);
            float lo = C.u_min[0], hi = C.u_max[0];
#pragma unroll
            for (int q = 1; q < 7; ++q) { lo = (i == q) ? C.u_min[q] : lo; hi = (i == q) ? C.u_max[q] : hi; }
            Uc[ru * Bc + c] = fminf(fmaxf(fmaf(alpha, dU[ru * B + b], U[ru * B + b]), lo), hi);
        }
    }
}

// ---- merit: phi[c] = J[c] + mu[c % Bn] sum_k sum_i |R[k][i][c]|, defect_inf[c] = max |R| -----------------------------------------
// One lane per column, rows in their order (a fixed summation order, no atomics).  R == nullptr: R = X[k + 1] - F[k] of an iterate.
__global__ __launch_bounds__(kBlock) void k_shoot_merit(const float* __restrict__ J, const float* __restrict__ mu, long Bn,
                                                        const float* __restrict__ R, const float* __restrict__ F,
                                                        const float* __restrict__ X, long B, long H, float* __restrict__ phi,
                                                        float* __restrict__ defect_inf) {
    const long c = (long)blockIdx.x * kBlock + threadIdx.x;
    if (c >= B) return;
    float sum = 0.f, mx = 0.f;
    for (long r = 0; r < H * 13; ++r) {
        const float v = fabsf(R != nullptr ? R[r * B + c] : X[(r + 13) * B + c] - F[r * B + c]);
        sum += v;
        mx = fmaxf(mx, v);
    }
    phi[c] = fmaf(mu[c % Bn], sum, J[c]);
    defect_inf[c] = mx;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
hipError_t shoot_launch_direction(const IlqrCost& C, bool clip, const float* X, const float* U, const float* F, const float* A,
                                  const float* Bm, const float* K, const float* kff, const float* Vx, const float* Vxx, long B, long H,
                                  float* dX, float* dU, float* Lam, hipStream_t st, int* grid) {
    *grid = (int)B;  // one wave per instance
    hipLaunchKernelGGL(k_shoot_direction, *grid, 64, 0, st, C, X, U, F, A, Bm, K, kff, Vx, Vxx, clip ? 1 : 0, B, H, dX, dU, Lam);
    return hipGetLastError();
}

hipError_t shoot_launch_merit_weight(const float* Lam, float factor, long B, long H, float* mu, hipStream_t st, int* grid) {
    *grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_shoot_merit_weight, *grid, kBlock, 0, st, Lam, factor, B, H, mu);
    return hipGetLastError();
}

hipError_t shoot_launch_candidates(const IlqrCost& C, const float* X, const float* U, const float* dX, const float* dU,
                                   const AlphaSet& al, long B, long H, float* Xc, float* Uc, hipStream_t st, int* grid) {
    const long nrows = (H + 1) * 13 + H * 7;
    *grid = (int)(((long)al.n * B + kBlock - 1) / kBlock);
    const dim3 g((unsigned)*grid, (unsigned)(nrows < 4096 ? nrows : 4096));
    hipLaunchKernelGGL(k_shoot_candidates, g, kBlock, 0, st, C, X, U, dX, dU, al, B, H, Xc, Uc);
    return hipGetLastError();
}

hipError_t shoot_launch_merit(const float* J, const float* mu, long Bn, const float* R, const float* F, const float* X, long B, long H,
                              float* phi, float* defect_inf, hipStream_t st, int* grid) {
    *grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_shoot_merit, *grid, kBlock, 0, st, J, mu, Bn, R, F, X, B, H, phi, defect_inf);
    return hipGetLastError();
}

}  // namespace ac
