// Iterated extended Kalman smoother: k_ieks_filter, k_ieks_candidates, k_ieks_cost_nodes, k_ieks_cost_reduce, k_ieks_accept and
// their launchers (ac_ieks.hpp).
#include "ac_ieks.hpp"

namespace ac {

// (T is the same for every group of the workgroup: AC_GROUP_SLOT's rule holds.)  waves_per_eu: the 48 KiB of mirrors would let
// three workgroups share a CU, and the register budget the compiler derives from that (168) spills the lane state; with the whole
// file the kernel keeps it in registers (0 B scratch) at one wave per SIMD, k_ekf_smooth's occupancy.
__global__ __launch_bounds__(kIeksGroups* kEkfLanes) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_ieks_filter(const ac_ekf_opts o, float eps, const IeksIo io) {
    __shared__ IeksShared sh[kIeksGroups];
    AC_GROUP_SLOT(kEkfLanes, kIeksGroups, blockIdx.x, io.n);
    GroupDev<IeksLane> grp;
    grp.r = r;
    ieks_filter_group(grp, sh[g], o, eps, io, i, store);
}

// row-major over [T+1][C][n]: neighbouring lanes, neighbouring columns
__global__ __launch_bounds__(kIeksBlock) void k_ieks_candidates(const IeksCandIo io) {
    const long cols = io.n * io.lad.count;
    const long t = (long)blockIdx.x * kIeksBlock + threadIdx.x;
    if (t >= (io.T + 1) * cols) return;
    const long col = t % cols;
    ieks_candidate_unit(io, t / cols, (int)(col / io.n), col % io.n);
}

// Workgroup b works on chunk b / gb of the columns (b % gb) * 256 .. + 255 (gb: workgroups per chunk), so that neighbouring
// workgroups read neighbouring columns of the same nodes.
__global__ __launch_bounds__(kIeksBlock) void k_ieks_cost_nodes(const IeksCostIo io, const long gb) {
    const long col = ((long)blockIdx.x % gb) * kIeksBlock + threadIdx.x;
    if (col >= io.n * io.reps) return;
    ieks_cost_nodes_unit(io, col, (long)blockIdx.x / gb);
}

__global__ __launch_bounds__(kIeksBlock) void k_ieks_cost_reduce(const IeksCostIo io) {
    const long col = (long)blockIdx.x * kIeksBlock + threadIdx.x;
    if (col >= io.n * io.reps) return;
    ieks_cost_reduce_unit(io, col);
}

// row-major over [T+1][n]
__global__ __launch_bounds__(kIeksBlock) void k_ieks_accept(const IeksAcceptIo io) {
    const long t = (long)blockIdx.x * kIeksBlock + threadIdx.x;
    if (t >= (io.T + 1) * io.n) return;
    ieks_accept_unit(io, t / io.n, t % io.n);
}

hipError_t ieks_launch_filter(const ac_ekf_opts& o, float eps, const IeksIo& io, hipStream_t st, int* grid, int* lds) {
    *grid = (int)((io.n + kIeksGroups - 1) / kIeksGroups);
    *lds = (int)(kIeksGroups * sizeof(IeksShared));
    hipLaunchKernelGGL(k_ieks_filter, *grid, kIeksGroups * kEkfLanes, 0, st, o, eps, io);
    return hipGetLastError();
}

hipError_t ieks_launch_candidates(const IeksCandIo& io, hipStream_t st, int* grid) {
    const long lanes = (io.T + 1) * io.n * io.lad.count;
    *grid = (int)((lanes + kIeksBlock - 1) / kIeksBlock);
    hipLaunchKernelGGL(k_ieks_candidates, *grid, kIeksBlock, 0, st, io);
    return hipGetLastError();
}

hipError_t ieks_launch_cost(const IeksCostIo& io, hipStream_t st, int* grid) {
    const long cols = io.n * io.reps, gb = (cols + kIeksBlock - 1) / kIeksBlock, chunks = ieks_chunks(io.T);
    *grid = (int)(gb * chunks);
    if (chunks > 0) {
        hipLaunchKernelGGL(k_ieks_cost_nodes, *grid, kIeksBlock, 0, st, io, gb);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ieks_cost_reduce, (int)gb, kIeksBlock, 0, st, io);
    return hipGetLastError();
}

hipError_t ieks_launch_accept(const IeksAcceptIo& io, hipStream_t st, int* grid) {
    const long lanes = (io.T + 1) * io.n;
    *grid = (int)((lanes + kIeksBlock - 1) / kIeksBlock);
    hipLaunchKernelGGL(k_ieks_accept, *grid, kIeksBlock, 0, st, io);
    return hipGetLastError();
}

}  // namespace ac
