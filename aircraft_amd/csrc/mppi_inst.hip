// MPPI: k_mppi_sample, k_mppi_weights, k_mppi_blend and their launchers (see ac_mppi.hpp).
#include "ac_mppi.hpp"

namespace ac {

// ---- sampler -----------------------------------------------------------------------------------------------------------------
// Lane = kMppiCols consecutive candidate columns o .. o + 3 (N = K B columns) of one node; blockIdx.y strides the nodes.
// VEC: N % 4 == 0 and 16-byte aligned outputs -> one dwordx4 store per row (a wave writes 1 KiB contiguous per row).
template <bool VEC>
__global__ __launch_bounds__(kMppiBlock) void k_mppi_sample(const ac_mppi_opts o, const unsigned* __restrict__ it_dev,
                                                            const float* __restrict__ Unom, const float* __restrict__ X0, int K,
                                                            long B, long H, float* __restrict__ Uc, float* __restrict__ X0c) {
    const long N = (long)K * B;
    const long o0 = ((long)blockIdx.x * kMppiBlock + threadIdx.x) * kMppiCols;
    if (o0 >= N) return;
    const unsigned it = it_dev ? *it_dev : 0u;
    long kc[kMppiCols], bc[kMppiCols];
    kc[0] = o0 / B;
    bc[0] = o0 - kc[0] * B;
#pragma unroll
    for (int c = 1; c < kMppiCols; ++c) {
        const bool wrap = bc[c - 1] + 1 == B;
        kc[c] = kc[c - 1] + (wrap ? 1 : 0);
        bc[c] = wrap ? 0 : bc[c - 1] + 1;
    }
    const int ncol = VEC ? kMppiCols : (int)((N - o0) < (long)kMppiCols ? (N - o0) : (long)kMppiCols);
    if (X0 && blockIdx.y == 0) {
        for (int i = 0; i < 13; ++i) {
            float v[kMppiCols];
#pragma unroll
            for (int c = 0; c < kMppiCols; ++c) v[c] = c < ncol ? X0[i * B + bc[c]] : 0.f;
            float* dst = X0c + i * N + o0;
            if (VEC) {
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int c = 0; c < kMppiCols; ++c)
                    if (c < ncol) dst[c] = v[c];
            }
        }
    }
    for (long t = blockIdx.y; t < H; t += gridDim.y) {
        float u[7][kMppiCols];
#pragma unroll
        for (int c = 0; c < kMppiCols; ++c) {
            float unom[7], out[7];
            if (c < ncol) {
#pragma unroll
                for (int r = 0; r < 7; ++r) unom[r] = Unom[(t * 7 + r) * B + bc[c]];
                mppi_sample_column(o, (unsigned)kc[c], o.instance_offset + (unsigned)bc[c], (unsigned)t, it,
                                   o.keep_nominal && kc[c] == 0, unom, out);
            } else {
#pragma unroll
                for (int r = 0; r < 7; ++r) out[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < 7; ++r) u[r][c] = out[r];
        }
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            float* dst = Uc + (t * 7 + r) * N + o0;
            if (VEC) {
                *reinterpret_cast<float4*>(dst) = make_float4(u[r][0], u[r][1], u[r][2], u[r][3]);
            } else {
#pragma unroll
                for (int c = 0; c < kMppiCols; ++c)
                    if (c < ncol) dst[c] = u[r][c];
            }
        }
    }
}

// ---- weights -------------------------------------------------------------------------------------------------------------------
// Workgroup = KL x BL lanes, lane (kl, bl) = threadIdx.x / BL, threadIdx.x % BL: instance b = blockIdx.x BL + bl, samples
// k = kl, kl + KL, ...  Every reduction over kl is a tree in LDS in a fixed order.
template <int BL>
__global__ __launch_bounds__(kMppiBlock) void k_mppi_weights(const float* __restrict__ J, int K, long B, float lambda,
                                                             float* __restrict__ w, float* __restrict__ stats) {
    constexpr int KL = kMppiBlock / BL;
    __shared__ float sa[kMppiBlock];
    __shared__ float sb[kMppiBlock];
    __shared__ int si[kMppiBlock];
    __shared__ int sc[kMppiBlock];
    const int tid = threadIdx.x, kl = tid / BL, bl = tid % BL;
    const long b = (long)blockIdx.x * BL + bl;
    const bool live = b < B;
    // 1. the cheapest finite cost, its index, the number of finite costs
    float jmin = __builtin_inff();
    int kmin = -1, cnt = 0;
    if (live)
        for (int k = kl; k < K; k += KL) {
            const float j = J[(long)k * B + b];
            if (mppi_finite(j)) {
                ++cnt;
                if (kmin < 0 || j < jmin) { jmin = j; kmin = k; }  // (k ascends: the first of equal costs stays)
            }
        }
    if (KL > 1) {
        sa[tid] = jmin; si[tid] = kmin; sc[tid] = cnt;
        __syncthreads();
        for (int s = KL / 2; s > 0; s >>= 1) {
            if (kl < s) {
                const int p = tid + s * BL;
                const float jo = sa[p];
                const int ko = si[p];
                if (ko >= 0 && (si[tid] < 0 || mppi_better(jo, ko, sa[tid], si[tid]))) { sa[tid] = jo; si[tid] = ko; }
                sc[tid] += sc[p];
            }
            __syncthreads();
        }
        jmin = sa[bl]; kmin = si[bl]; cnt = sc[bl];
        __syncthreads();
    }
    // 2. eta = sum w, sum w^2
    float s1 = 0.f, s2 = 0.f;
    if (live && kmin >= 0)
        for (int k = kl; k < K; k += KL) {
            const float wk = mppi_weight(J[(long)k * B + b], jmin, lambda);
            s1 += wk;
            s2 = fmaf(wk, wk, s2);
        }
    if (KL > 1) {
        sa[tid] = s1; sb[tid] = s2;
        __syncthreads();
        for (int s = KL / 2; s > 0; s >>= 1) {
            if (kl < s) { sa[tid] += sa[tid + s * BL]; sb[tid] += sb[tid + s * BL]; }
            __syncthreads();
        }
        s1 = sa[bl]; s2 = sb[bl];
    }
    if (!live) return;
    // 3. the normalised weights (zero for an instance without a finite cost: the blend then keeps the nominal)
    for (int k = kl; k < K; k += KL)
        w[(long)k * B + b] = kmin >= 0 ? mppi_weight(J[(long)k * B + b], jmin, lambda) / s1 : 0.f;
    if (kl == 0) {
        stats[b] = jmin;                                  // +inf when no cost is finite
        stats[B + b] = kmin >= 0 ? (s1 * s1) / s2 : 0.f;  // effective sample size (the best sample has w = 1: s2 >= 1)
        stats[2 * B + b] = (float)cnt;
        stats[3 * B + b] = (float)kmin;
    }
}

// ---- blend ---------------------------------------------------------------------------------------------------------------------
// Workgroup = KL x BL lanes as above; a lane owns V consecutive instances of one row (t, r) = blockIdx.y and sums its samples
// in ascending k; the KL partial sums meet in an LDS tree.  V = 4: B % 4 == 0 and 16-byte aligned buffers (dwordx4 loads).
template <int BL, int V>
__global__ __launch_bounds__(kMppiBlock) void k_mppi_blend(const ac_mppi_opts o, unsigned* __restrict__ it_dev,
                                                           const float* __restrict__ w, const float* __restrict__ stats,
                                                           const float* __restrict__ Uc, const float* Unom, int K, long B,
                                                           long H, float* Unew) {
    constexpr int KL = kMppiBlock / BL;
    __shared__ float sm[KL > 1 ? kMppiBlock * V : 1];
    const int tid = threadIdx.x, kl = tid / BL, bl = tid % BL;
    const long b = ((long)blockIdx.x * BL + bl) * V;
    const bool live = b < B;
    const long N = (long)K * B;
    for (long row = blockIdx.y; row < H * 7; row += gridDim.y) {
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.f;
        if (live) {
            const float* up = Uc + row * N + b;
            const float* wp = w + b;
            for (int k = kl; k < K; k += KL) {
                if (V == 4) {
                    const float4 a = *reinterpret_cast<const float4*>(up + (long)k * B);
                    const float4 c = *reinterpret_cast<const float4*>(wp + (long)k * B);
                    acc[0] = fmaf(c.x, a.x, acc[0]); acc[1 % V] = fmaf(c.y, a.y, acc[1 % V]);
                    acc[2 % V] = fmaf(c.z, a.z, acc[2 % V]); acc[3 % V] = fmaf(c.w, a.w, acc[3 % V]);
                } else {
                    acc[0] = fmaf(wp[(long)k * B], up[(long)k * B], acc[0]);
                }
            }
        }
        if (KL > 1) {
#pragma unroll
            for (int v = 0; v < V; ++v) sm[v * kMppiBlock + tid] = acc[v];
            __syncthreads();
            for (int s = KL / 2; s > 0; s >>= 1) {
                if (kl < s) {
#pragma unroll
                    for (int v = 0; v < V; ++v) sm[v * kMppiBlock + tid] += sm[v * kMppiBlock + tid + s * BL];
                }
                __syncthreads();
            }
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = sm[v * kMppiBlock + bl];
            __syncthreads();
        }
        if (live && kl == 0) {
            const int r = (int)(row % 7);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const long i = row * B + b + v;
                const bool any = stats[2 * B + b + v] > 0.f;  // |F| > 0
                const float keep = Unom[i];                    // (read before the store: Unew may be Unom)
                Unew[i] = any ? mppi_clip(acc[v], o.u_min[r], o.u_max[r]) : keep;
            }
        }
    }
    // the last action of the update: the iteration counter, one plain store by one lane
    if (it_dev && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *it_dev = *it_dev + 1u;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
namespace {
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
int lanes_along_b(long n) {  // the power of four (1 .. 256) that covers n instances-per-lane groups, capped at the workgroup
    int bl = 1;
    while (bl < kMppiBlock && bl < n) bl *= 4;
    return bl;
}
}  // namespace

hipError_t mppi_launch_sample(const ac_mppi_opts& o, const unsigned* it_dev, const float* Unom, const float* X0, int K, long B,
                              long H, float* Uc, float* X0c, hipStream_t st, int* grid) {
    const long N = (long)K * B;
    const long groups = (N + kMppiCols - 1) / kMppiCols;
    const dim3 g((unsigned)((groups + kMppiBlock - 1) / kMppiBlock), (unsigned)(H < 65535 ? H : 65535));
    const bool vec = N % kMppiCols == 0 && aligned16(Uc) && (!X0c || aligned16(X0c));
    if (vec)
        hipLaunchKernelGGL(k_mppi_sample<true>, g, kMppiBlock, 0, st, o, it_dev, Unom, X0, K, B, H, Uc, X0c);
    else
        hipLaunchKernelGGL(k_mppi_sample<false>, g, kMppiBlock, 0, st, o, it_dev, Unom, X0, K, B, H, Uc, X0c);
    *grid = (int)g.x;
    return hipGetLastError();
}

hipError_t mppi_launch_update(const ac_mppi_opts& o, unsigned* it_dev, const float* J, const float* Uc, const float* Unom, int K,
                              long B, long H, float* Unew, float* stats, float* w, hipStream_t st, int* grid) {
    {
        const int bl = lanes_along_b(B);
        const unsigned g = (unsigned)((B + bl - 1) / bl);
#define AC_MPPI_W(BL_) \
    case BL_: hipLaunchKernelGGL(k_mppi_weights<BL_>, g, kMppiBlock, 0, st, J, K, B, o.lambda, w, stats); break;
        switch (bl) { AC_MPPI_W(1) AC_MPPI_W(4) AC_MPPI_W(16) AC_MPPI_W(64) default: AC_MPPI_W(256) }
#undef AC_MPPI_W
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const bool vec = B % 4 == 0 && aligned16(Uc) && aligned16(w) && aligned16(Unom) && aligned16(Unew);
    const long per = vec ? B / 4 : B;
    const int bl = lanes_along_b(per);
    const long rows = H * 7;
    const dim3 g((unsigned)((per + bl - 1) / bl), (unsigned)(rows < 65535 ? rows : 65535));
#define AC_MPPI_B(BL_)                                                                                                        \
    case BL_:                                                                                                                 \
        if (vec) hipLaunchKernelGGL((k_mppi_blend<BL_, 4>), g, kMppiBlock, 0, st, o, it_dev, w, stats, Uc, Unom, K, B, H, Unew); \
        else hipLaunchKernelGGL((k_mppi_blend<BL_, 1>), g, kMppiBlock, 0, st, o, it_dev, w, stats, Uc, Unom, K, B, H, Unew);     \
        break;
    switch (bl) { AC_MPPI_B(1) AC_MPPI_B(4) AC_MPPI_B(16) AC_MPPI_B(64) default: AC_MPPI_B(256) }
#undef AC_MPPI_B
    *grid = (int)g.x;
    return hipGetLastError();
}

}  // namespace ac
