// ac_group.hpp — what the group kernels share: one instance per 16-lane group, lane r owns row r, what every
// lane reads goes through LDS mirrors of row stride 13, and the work is cut into phases: a phase reads from the mirrors only
// what an EARLIER phase wrote.  Here: the group itself (GroupDev: one lane and the workgroup's barrier after every phase;
// GroupHost: the host build's loop over the lanes, -DAC_HOST_CHECK), where a lane of a group kernel sits in the batch
// (AC_GROUP_SLOT), and the column of the 12 x 12 plain Cholesky on a mirror (grp_chol_column).
#pragma once
#include "ac_math.hpp"

// AC_EKF_FP opens every function body of the estimators' headers: no contraction of a * b + c into one FMA beyond the fmaf
// calls that are written out, so that the device rounds where the host build (-ffp-contract=off) rounds.  The two then differ
// by the library functions alone (atan2f, asinf, logf), and the host build's error against float64 is the device's.
#ifdef AC_HOST_CHECK
#define AC_EKF_INLINE
#define AC_EKF_FP
#else
#define AC_EKF_INLINE __attribute__((always_inline))
#define AC_EKF_FP _Pragma("clang fp contract(off)")
#endif

namespace ac {

constexpr int kGrpLanes = 16;  // lanes of one instance's group (rows 12-15 idle)
constexpr int kGrpLd = 13;     // row stride of the LDS mirrors
constexpr float kEkfFltMax = 3.0e38f;

// The host build: the lanes of a group one after the other, phase by phase.
template <class Lane, int kLanes>
struct GroupHost {
    Lane L[kLanes];
    template <class F>
    void each(F f) {
        for (int r = 0; r < kLanes; ++r) f(L[r], r);
    }
};

#ifndef AC_HOST_CHECK
// One lane of a group: a phase, then the workgroup's barrier (it orders the LDS traffic of the phase).
template <class Lane>
struct GroupDev {
    Lane L;
    int r;
    template <class F>
    __device__ __forceinline__ void each(F f) {
        f(L, r);
        __syncthreads();
    }
};

// Where this lane sits, as the first statement of a group kernel: it declares g (the group of the workgroup), i (the instance
// of the batch of n), store and r (the lane of the group); wg is the workgroup's index within the batch.  A group past the
// end of the batch works on the last instance again and stores nothing (store false): every lane of the workgroup reaches
// every barrier.  (A macro: as a function it moves the read of the workgroup index ahead of g, and the register allocation
// of the kernels with it.)
#define AC_GROUP_SLOT(kLanes, kGroups, wg, n)  \
    const int g = threadIdx.x / (kLanes);      \
    long i = (long)(wg) * (kGroups) + g;       \
    const bool store = i < (n);                \
    if (!store) i = (n)-1;                     \
    const int r = threadIdx.x % (kLanes)
#endif

// Column j of the plain Cholesky L L' = M of the 12 x 12 matrix in the mirror m, which keeps L below its diagonal; one phase
// per column, in order.  Lane r forms L_rj into l[j] (l: row r of L so far), every lane the pivot, every sum in index order;
// w = 1 / L_jj.  A pivot that is <= 0 or not finite sets bad (it is never cleared here) and the column is formed with pivot 1.
// The two triangular solves against the mirror stay with their callers (ac_rts.hpp, ac_em.hpp): through a shared function
// k_ekf_smooth ran 1.2 - 1.8 % slower and k_ekf_em_nodes took 12 more VGPRs (profiles/README.md, group_refactor_ab.jsonl).
AC_DI void grp_chol_column(float (&m)[kGrpLanes][kGrpLd], float (&l)[12], int r, int j, float& w, bool& bad) {
    AC_EKF_FP
    float t = m[r][j], d = m[j][j];  // (row r is overwritten from column j on only after this read)
#pragma unroll
    for (int c = 0; c < j; ++c) {
        const float lj = m[j][c];
        t = fmaf(-l[c], lj, t);
        d = fmaf(-lj, lj, d);
    }
    if (!(d > 0.f && d <= kEkfFltMax)) {
        bad = true;
        d = 1.0f;
    }
    w = 1.0f / sqrtf(d);
    l[j] = t * w;
    if (r > j) m[r][j] = l[j];
}

}  // namespace ac
