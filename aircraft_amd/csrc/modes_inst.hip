// Batched eigenvalues and flight modes: k_eig, k_modes_eig and their launchers (ac_eig.hpp).
#include "ac_eig.hpp"

namespace ac {
namespace {

// Word w of this lane's instance: LDS word w * (instances of the workgroup) + lane.
struct EigLds {
    double* b;
    int stride;
    __device__ __forceinline__ double& operator[](int w) const { return b[w * stride]; }
};

int eig_grid(long n, int m) { return (int)((n + eig_lanes(m) - 1) / eig_lanes(m)); }

}  // namespace

// No barrier anywhere: a lane past the end of the batch leaves at once.
__global__ __launch_bounds__(kEigLanes) void k_eig(const float* __restrict__ M, int m, int max_iters, long n, float* __restrict__ wr,
                                                   float* __restrict__ wi, int* __restrict__ status, int* __restrict__ iters) {
    extern __shared__ double eig_mem[];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    EigLds a{eig_mem + threadIdx.x, (int)blockDim.x};
    eig_unit(a, EigCCol{M + i, n}, m, max_iters, EigCol{wr + i, n}, EigCol{wi + i, n}, status + i, iters ? iters + i : nullptr);
}

__global__ __launch_bounds__(kEigLanes) void k_modes_eig(const float* __restrict__ Axi, const float* __restrict__ Bxi,
                                                         const float* __restrict__ K, unsigned coords, int m, int max_iters, float dt,
                                                         long n, float* __restrict__ wr, float* __restrict__ wi,
                                                         float* __restrict__ sigma, float* __restrict__ omega,
                                                         int* __restrict__ status, int* __restrict__ iters) {
    extern __shared__ double eig_mem[];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    EigLds a{eig_mem + threadIdx.x, (int)blockDim.x};
    modes_unit(a, EigCCol{Axi + i, n}, EigCCol{Bxi + i, n}, EigCCol{K ? K + i : nullptr, n}, coords, m, max_iters, dt,
               EigCol{wr + i, n}, EigCol{wi + i, n}, EigCol{sigma + i, n}, EigCol{omega + i, n}, status + i,
               iters ? iters + i : nullptr);
}

hipError_t eig_launch(const float* M, int m, int max_iters, long n, float* wr, float* wi, int* status, int* iters, hipStream_t st,
                      int* grid, int* lds) {
    *grid = eig_grid(n, m);
    *lds = eig_lds_bytes(m);
    hipLaunchKernelGGL(k_eig, *grid, eig_lanes(m), *lds, st, M, m, max_iters, n, wr, wi, status, iters);
    return hipGetLastError();
}

hipError_t modes_launch_eig(const float* Axi, const float* Bxi, const float* K, unsigned coords, int m, int max_iters, float dt,
                            long n, float* wr, float* wi, float* sigma, float* omega, int* status, int* iters, hipStream_t st,
                            int* grid, int* lds) {
    *grid = eig_grid(n, m);
    *lds = eig_lds_bytes(m);
    hipLaunchKernelGGL(k_modes_eig, *grid, eig_lanes(m), *lds, st, Axi, Bxi, K, coords, m, max_iters, dt, n, wr, wi, sigma, omega,
                       status, iters);
    return hipGetLastError();
}

}  // namespace ac
