// abi_flight.hip — flight mechanics about a steady state: trim, the LQR and its gains, flight modes, and the MPPI controller.
// One unit of the C ABI (include/aircraft_hip.h); the handle and the helpers every unit shares: ac_abi.hpp.
#include "ac_abi.hpp"
#include "ac_eig.hpp"
#include "ac_lqr.hpp"
#include "ac_mppi.hpp"
#include "ac_trim.hpp"

using namespace ac;

extern "C" {

// ---- steady-flight trim (ac_trim.hpp) -----------------------------------------------------------------------------------------
namespace {
// the six workspace buffers each start on a 256-byte boundary, as a torch allocation would
constexpr size_t kTrimWsPad = 6 * 64;
size_t trim_ws_floats(long n) { return (size_t)n * (size_t)kTrimWsFloats + kTrimWsPad; }
}  // namespace

int ac_trim_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "trim is defined for the fixed-wing models only");
    *floats = trim_ws_floats(n);
    return AC_OK;
}

int ac_trim_f32(ac_handle* h, const ac_trim_opts* o, const float* target, const float* Uhold, const float* Z0, int iters, long n,
                float* X, float* U, float* Z, float* R, int* status, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !o || iters < 1 || n < 0 || (o->lateral != 0 && o->lateral != 1)) return AC_ERR_BAD_ARG;
    if (!(o->tol_v > 0.f) || !(o->tol_w > 0.f)) return fail(AC_ERR_BAD_ARG, "trim tolerances must be > 0");
    for (int j = 0; j < 6; ++j)
        if (!(o->lo[j] <= o->hi[j])) return fail(AC_ERR_BAD_ARG, "trim bounds: lo > hi (or NaN)");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "trim is defined for the fixed-wing models only");
    if (n == 0) return AC_OK;
    if (!target || !Uhold || !Z0 || !X || !U || !Z || !R || !status) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const size_t N = (size_t)n;
    if (!ws || ws_floats < trim_ws_floats(n))
        return fail(AC_ERR_WORKSPACE, "trim workspace too small: see ac_trim_workspace_floats");
    float* Xw = align256(ws);
    float* Uw = align256(Xw + 13 * N);
    float* Xd = align256(Uw + 7 * N);
    float* Fx = align256(Xd + 13 * N);
    float* Fu = align256(Fx + 169 * N);
    float* St = align256(Fu + 91 * N);  // ends at most ws + 350 N + 6 * 63 floats
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)((n + kTrimBlock - 1) / kTrimBlock);
    for (int k = 0; k < iters; ++k) {
        hipLaunchKernelGGL(k_trim_assemble, grid, kTrimBlock, 0, st, *o, target, Uhold, Z0, n, (int)(k == 0), Xw, Uw, St);
        AC_HIP(hipGetLastError());
        rc = deriv_sens_impl(h, Xw, Uw, n, n, Xd, Fx, Fu, stream);
        if (rc != AC_OK) return rc;
        hipLaunchKernelGGL(k_trim_update, grid, kTrimBlock, 0, st, *o, target, Uhold, Xd, Fx, Fu, n, (int)(k == iters - 1), St, X, U,
                           Z, R, status);
        AC_HIP(hipGetLastError());
    }
    note_launch(h, "k_trim_update", grid, kTrimBlock, 0);
    return AC_OK;
}

// ---- LQR about steady-flight trims (ac_lqr.hpp, lqr_inst.hip) ----------------------------------------------------------------------
namespace {
constexpr size_t kLqrWsPad = 3 * 64;  // the three workspace buffers each start on a 256-byte boundary
size_t lqr_ws_floats(long n) { return (size_t)n * (size_t)kLqrWsFloats + kLqrWsPad; }
const char* const kLqrFixedWing = "the LQR about a trim is defined for the fixed-wing models only";
}  // namespace

int ac_lqr_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    *floats = lqr_ws_floats(n);
    return AC_OK;
}

int ac_lqr_f32(ac_handle* h, const ac_lqr_opts* o, const float* X, const float* U, float dt, int iters, long n, float* Axi,
               float* Bxi, float* P, float* K, float* resid, int* status, int* used_iters, float* ws, size_t ws_floats,
               void* stream) {
    AC_ENTER(h);
    if (!h || !o || iters < 1 || n < 0) return AC_ERR_BAD_ARG;
    if (!(dt > 0.f) || !(dt <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "lqr: dt must be finite and > 0");
    for (int i = 0; i < 12; ++i)
        if (!(o->q[i] >= 0.f) || !(o->q[i] <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "lqr: q must be finite and >= 0");
    for (int j = 0; j < 7; ++j)
        if (!(o->r[j] > 0.f) || !(o->r[j] <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "lqr: r must be finite and > 0");
    if (!(o->tol >= 0.f)) return fail(AC_ERR_BAD_ARG, "lqr: tol must be >= 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !U || !Axi || !Bxi || !P || !K || !resid || !status || !used_iters) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (!ws || ws_floats < lqr_ws_floats(n)) return fail(AC_ERR_WORKSPACE, "lqr workspace too small: see ac_lqr_workspace_floats");
    const size_t N = (size_t)n;
    float* const Xp = align256(ws);
    float* const A = align256(Xp + 13 * N);
    float* const Bm = align256(A + 169 * N);  // ends at most ws + 273 N + 3 * 63 floats
    rc = sens_impl(h, X, U, dt, nullptr, n, n, Xp, A, Bm, nullptr, stream);
    if (rc != AC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    int grid = 0, lds = 0;
    AC_HIP(lqr_launch_project(X, U, Xp, A, Bm, n, Axi, Bxi, st, &grid));
    AC_HIP(lqr_launch_dare(*o, iters, Axi, Bxi, n, P, K, resid, status, used_iters, st, &grid, &lds));
    note_launch(h, "k_lqr_dare", grid, kLqrGroups * kLqrLanes, lds);
    return AC_OK;
}

int ac_lqr_gains_f32(ac_handle* h, const float* Xnom, const float* K, long n, long H, float* Kx, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || H < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    if (n == 0 || H == 0) return AC_OK;
    if (!Xnom || !K || !Kx) return AC_ERR_BAD_ARG;
    int grid = 0;
    AC_HIP(lqr_launch_gains(Xnom, K, n, H, Kx, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqr_gains", grid, kLqrBlock, 0);
    return AC_OK;
}

int ac_steady_error_f32(ac_handle* h, const float* X, const float* Xnom, long n, float* xi, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !Xnom || !xi) return AC_ERR_BAD_ARG;
    int grid = 0;
    AC_HIP(lqr_launch_error(X, Xnom, n, xi, (hipStream_t)stream, &grid));
    note_launch(h, "k_steady_error", grid, kLqrBlock, 0);
    return AC_OK;
}

// ---- flight modes: batched eigenvalues of the trim linearisation (ac_eig.hpp, modes_inst.hip) ---------------------------------------
namespace {
constexpr size_t kModesWsPad = 5 * 64;  // the five workspace buffers each start on a 256-byte boundary
size_t modes_ws_floats(long n) { return (size_t)n * (size_t)kModesWsFloats + kModesWsPad; }
const char* const kModesFixedWing = "the flight modes about a trim are defined for the fixed-wing models only";
}  // namespace

int ac_eig_f32(ac_handle* h, const float* M, int m, int max_iters, long n, float* wr, float* wi, int* status, int* iters,
               void* stream) {
    AC_ENTER(h);
    if (!h || n < 0) return AC_ERR_BAD_ARG;
    if (m < 1 || m > kEigMaxM) return fail(AC_ERR_BAD_ARG, "eig: m must be 1 .. 13");
    if (max_iters < 0) return fail(AC_ERR_BAD_ARG, "eig: max_iters must be >= 0 (0: 30)");
    if (n == 0) return AC_OK;
    if (!M || !wr || !wi || !status) return fail(AC_ERR_BAD_ARG, "eig: a required pointer is NULL");
    const size_t N = (size_t)n, mm = (size_t)m;
    const RtsSpan in[] = {{M, mm * mm * N}};
    const RtsSpan out[] = {{wr, mm * N}, {wi, mm * N}, {(const float*)status, N}, {(const float*)iters, N}};
    if (modes_overlap(out, 4, in, 1)) return fail(AC_ERR_BAD_ARG, "eig: an output overlaps an input");
    int grid = 0, lds = 0;
    AC_HIP(eig_launch(M, m, max_iters ? max_iters : kEigDefaultIters, n, wr, wi, status, iters, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_eig", grid, eig_lanes(m), lds);
    return AC_OK;
}

int ac_modes_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kModesFixedWing);
    *floats = modes_ws_floats(n);
    return AC_OK;
}

int ac_modes_f32(ac_handle* h, const ac_modes_opts* o, const float* X, const float* U, float dt, const float* K, long n, float* Axi,
                 float* Bxi, float* wr, float* wi, float* sigma, float* omega, int* status, int* iters, float* ws, size_t ws_floats,
                 void* stream) {
    AC_ENTER(h);
    if (!h || !o || n < 0) return AC_ERR_BAD_ARG;
    if (!(dt > 0.f) || !(dt <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "modes: dt must be finite and > 0");
    if (o->max_iters < 0) return fail(AC_ERR_BAD_ARG, "modes: max_iters must be >= 0 (0: 30)");
    const unsigned coords = o->coords ? o->coords : kModesFlight;
    if ((coords & kModesFlight) != kModesFlight || (coords >> 12) != 0u)
        return fail(AC_ERR_BAD_ARG, "modes: coords must keep the chart coordinates 3-7 and 9-11 and set no bit >= 12");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kModesFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !U || !wr || !wi || !sigma || !omega || !status) return fail(AC_ERR_BAD_ARG, "modes: a required pointer is NULL");
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (!ws || ws_floats < modes_ws_floats(n)) return fail(AC_ERR_WORKSPACE, "modes workspace too small: see ac_modes_workspace_floats");
    const size_t N = (size_t)n;
    const RtsSpan in[] = {{X, 13 * N}, {U, 7 * N}, {K, 84 * N}};
    const RtsSpan out[] = {{Axi, 144 * N}, {Bxi, 84 * N}, {wr, 12 * N}, {wi, 12 * N}, {sigma, 12 * N}, {omega, 12 * N},
                           {(const float*)status, N}, {(const float*)iters, N}, {ws, ws_floats}};
    if (modes_overlap(out, 9, in, 3)) return fail(AC_ERR_BAD_ARG, "modes: an output overlaps an input");
    float* const Xp = align256(ws);
    float* const A = align256(Xp + 13 * N);
    float* const Bm = align256(A + 169 * N);
    float* const Aw = align256(Bm + 91 * N);
    float* const Bw = align256(Aw + 144 * N);  // ends at most ws + 501 N + 5 * 63 floats
    if (!Axi) Axi = Aw;
    if (!Bxi) Bxi = Bw;
    rc = sens_impl(h, X, U, dt, nullptr, n, n, Xp, A, Bm, nullptr, stream);
    if (rc != AC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    int grid = 0, lds = 0, m = 0;
    for (int i = 0; i < 12; ++i) m += (int)((coords >> i) & 1u);
    AC_HIP(lqr_launch_project(X, U, Xp, A, Bm, n, Axi, Bxi, st, &grid));
    AC_HIP(modes_launch_eig(Axi, Bxi, K, coords, m, o->max_iters ? o->max_iters : kEigDefaultIters, dt, n, wr, wi, sigma, omega,
                            status, iters, st, &grid, &lds));
    note_launch(h, "k_modes_eig", grid, eig_lanes(m), lds);
    return AC_OK;
}

// ---- MPPI: sampler and softmin update (ac_mppi.hpp, mppi_inst.hip) ---------------------------------------------------------------
namespace {
int mppi_check(const ac_handle* h, const ac_mppi_opts* o, int K, long B, long H) {
    if (!h || !o || K < 1 || B < 1 || H < 1) return AC_ERR_BAD_ARG;
    if ((long)K > 2147483647L / B) return fail(AC_ERR_BAD_ARG, "mppi: K * B exceeds 2^31 - 1");
    if (!(o->lambda > 0.f) || !(o->lambda <= 3.4028235e38f)) return fail(AC_ERR_BAD_ARG, "mppi: lambda must be finite and > 0");
    for (int r = 0; r < 7; ++r) {
        if (!(o->sigma[r] >= 0.f) || !(o->sigma[r] <= 3.4028235e38f))
            return fail(AC_ERR_BAD_ARG, "mppi: sigma must be finite and >= 0");
        if (!(o->u_min[r] <= o->u_max[r])) return fail(AC_ERR_BAD_ARG, "mppi: u_min > u_max (or NaN)");
    }
    return AC_OK;
}
}  // namespace

int ac_mppi_workspace_floats(const ac_handle* h, int K, long B, long H, size_t* floats) {
    if (!h || !floats || K < 1 || B < 1 || H < 1 || (long)K > 2147483647L / B) return AC_ERR_BAD_ARG;
    *floats = (size_t)K * (size_t)B;  // the normalised weights
    return AC_OK;
}

int ac_mppi_sample_f32(ac_handle* h, const ac_mppi_opts* o, const unsigned int* it_dev, const float* Unom, const float* X0, int K,
                       long B, long H, float* Uc, float* X0c, void* stream) {
    AC_ENTER(h);
    const int rc = mppi_check(h, o, K, B, H);
    if (rc != AC_OK) return rc;
    if (!Unom || !Uc) return AC_ERR_BAD_ARG;
    if ((X0 == nullptr) != (X0c == nullptr)) return fail(AC_ERR_BAD_ARG, "mppi: X0 and X0c go together");
    int grid = 0;
    AC_HIP(mppi_launch_sample(*o, it_dev, Unom, X0, K, B, H, Uc, X0c, (hipStream_t)stream, &grid));
    note_launch(h, "k_mppi_sample", grid, kMppiBlock, 0);
    return AC_OK;
}

int ac_mppi_update_f32(ac_handle* h, const ac_mppi_opts* o, unsigned int* it_dev, const float* J, const float* Uc, const float* Unom,
                       int K, long B, long H, float* Unew, float* stats, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    const int rc = mppi_check(h, o, K, B, H);
    if (rc != AC_OK) return rc;
    if (!J || !Uc || !Unom || !Unew || !stats) return AC_ERR_BAD_ARG;
    if (!ws || ws_floats < (size_t)K * (size_t)B)
        return fail(AC_ERR_WORKSPACE, "mppi workspace too small: see ac_mppi_workspace_floats");
    int grid = 0;
    AC_HIP(mppi_launch_update(*o, it_dev, J, Uc, Unom, K, B, H, Unew, stats, ws, (hipStream_t)stream, &grid));
    note_launch(h, "k_mppi_blend", grid, kMppiBlock, 0);
    return AC_OK;
}

}  // extern "C"
