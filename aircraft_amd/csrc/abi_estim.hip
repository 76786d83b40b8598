// abi_estim.hip — state estimation: the EKF and UKF banks, the loop closed through them (LQG), the RTS smoother, EM for the
// noise variances, and the iterated Kalman smoother.
// One unit of the C ABI (include/aircraft_hip.h); the handle and the helpers every unit shares: ac_abi.hpp.
#include <cstring>

#include "ac_abi.hpp"
#include "ac_ekf.hpp"
#include "ac_em.hpp"
#include "ac_ieks.hpp"
#include "ac_lqg.hpp"
#include "ac_rts.hpp"
#include "ac_ukf.hpp"

using namespace ac;

namespace {

// T steps as a host loop over an estimator's step, for a caller that has run the estimator's *_check.  step: its *_step_impl
// on the handle, the options and the workspace; buf: the two (x, P) pairs of the ping-pong in that workspace; name: what the
// messages call it.  Xpreds, Ppreds, Abars: the per-step records a smoother reads (each may be NULL).
template <class Step>
int filter_loop(const char* name, bool predict, Step step, float* const buf[4], const float* X, const float* P, const float* U,
                float dt, const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds,
                float* Ppreds, float* Abars, void* stream) {
    if (!X || !P || !Z || !Rd || !Xo || !Po || !ll) {
        snprintf(g_err, sizeof(g_err), "%s filter: a required pointer is NULL", name);
        return AC_ERR_BAD_ARG;
    }
    if (predict && (!U || !Qd)) {
        snprintf(g_err, sizeof(g_err), "%s filter: U and Qd are required when predict is set", name);
        return AC_ERR_BAD_ARG;
    }
    const size_t N = (size_t)n;
    const float *xin = X, *pin = P;
    for (long t = 0; t < T; ++t) {
        const bool last = t == T - 1;
        float* const xo = last ? Xo : buf[2 * (t & 1)];
        float* const po = last ? Po : buf[2 * (t & 1) + 1];
        const size_t k = (size_t)t;
        const int rc = step(xin, pin, U ? U + k * 7 * N : nullptr, dt, Z + k * 15 * N, mask ? mask + k * N : nullptr, Qd, Rd, n,
                            t ? ll : nullptr, xo, po, nu ? nu + k * 15 * N : nullptr, S ? S + k * 15 * N : nullptr,
                            nis ? nis + k * N : nullptr, ll, used ? used + k * N : nullptr, status ? status + k * N : nullptr,
                            Xpreds ? Xpreds + k * 13 * N : nullptr, Ppreds ? Ppreds + k * 144 * N : nullptr,
                            Abars ? Abars + k * 144 * N : nullptr);
        if (rc != AC_OK) return rc;
        if (Xs) AC_HIP(hipMemcpyAsync(Xs + k * 13 * N, xo, 13 * N * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        if (Ps) AC_HIP(hipMemcpyAsync(Ps + k * 144 * N, po, 144 * N * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        xin = xo;
        pin = po;
    }
    return AC_OK;
}

// ---- the two filter banks: the extended Kalman filter over the step sensitivities (ac_ekf.hpp, ekf_inst.hip) and the unscented
// one beside it (ac_ukf.hpp, ukf_inst.hip).  One set of entry points; a descriptor says what an estimator is ---------------------
const char* const kEkfFixedWing = "the extended Kalman filter is defined for the fixed-wing models only";

// What an estimator is: the name its messages carry, its options, its workspace and where the filter's two (x, P) pairs lie in
// it, one step, the options the loop of ac_lqg_rollout_f32 runs it with, and the checks only it has (extra_check: why not, or
// nullptr), on the options and, once there is work, on n.
struct Ekf {
    using Opts = ac_ekf_opts;
    static constexpr const char* kName = "ekf";
    static constexpr size_t kWsPad = 7 * 64;  // the seven workspace buffers each start on a 256-byte boundary
    static size_t ws_floats(long n) { return (size_t)n * (size_t)(kEkfSensFloats + kEkfChainFloats) + kWsPad; }
    static void pairs(float* ws, size_t N, float* buf[4]) {  // x, P | x, P behind the sensitivity outputs
        buf[0] = align256(align256(align256(align256(ws) + 13 * N) + 169 * N) + 91 * N);
        buf[1] = align256(buf[0] + 13 * N);
        buf[2] = align256(buf[1] + 144 * N);
        buf[3] = align256(buf[2] + 13 * N);  // ends at most ws + 587 N + 7 * 63 floats
    }
    static const char* extra_check(const Opts*) { return nullptr; }
    static const char* extra_check(long) { return nullptr; }
    static Opts lqg_opts(const ac_sense_opts* s, const ac_lqg_opts*) { return {{s->mag_ned[0], s->mag_ned[1], s->mag_ned[2]}, 1}; }

    // one step: the handle's sensitivity launch into the workspace, then k_ekf_step.  ll_in: added to this step's ll (or NULL).
    static int step_impl(ac_handle* h, const Opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                         const int* mask, const float* Qd, const float* Rd, long n, const float* ll_in, float* Xo, float* Po,
                         float* nu, float* S, float* nis, float* ll, int* used, int* status, float* Xpred, float* Ppred,
                         float* Abar, float* ws, void* stream) {
        const size_t N = (size_t)n;
        float* const Xp = align256(ws);
        float* const A = align256(Xp + 13 * N);
        float* const Bm = align256(A + 169 * N);
        if (o->predict) {
            const int rc = sens_impl(h, X, U, dt, nullptr, n, n, Xp, A, Bm, nullptr, stream);
            if (rc != AC_OK) return rc;
        }
        const EkfIo io{X, P, Xp, A, Z, Qd, Rd, mask, ll_in, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, n};
        int grid = 0, lds = 0;
        AC_HIP(ekf_launch_step(*o, h->dp.p.epsilon, io, (hipStream_t)stream, &grid, &lds));
        note_launch(h, "k_ekf_step", grid, kEkfGroups * kEkfLanes, lds);
        return AC_OK;
    }
};

struct Ukf {
    using Opts = ac_ukf_opts;
    static constexpr const char* kName = "ukf";
    static constexpr size_t kWsPad = 9 * 64;  // the nine workspace buffers each start on a 256-byte boundary
    static size_t ws_floats(long n) { return (size_t)n * (size_t)(kUkfInstFloats + kEkfChainFloats) + kWsPad; }
    // the workspace: points [13][25 n] | U [7][25 n] | images [13][25 n] | L [144][n] | flag [n] | the filter's two (x, P) pairs
    struct Ws {
        float *Xw, *Uw, *Fw, *Lw;
        int* flag;
        float* buf[4];
        Ws(float* ws, size_t N) {
            Xw = align256(ws);
            Uw = align256(Xw + 13 * kUkfPts * N);
            Fw = align256(Uw + 7 * kUkfPts * N);
            Lw = align256(Fw + 13 * kUkfPts * N);
            flag = (int*)align256(Lw + 144 * N);
            buf[0] = align256((float*)flag + N);
            buf[1] = align256(buf[0] + 13 * N);
            buf[2] = align256(buf[1] + 144 * N);
            buf[3] = align256(buf[2] + 13 * N);  // ends at most ws + 1284 N + 9 * 63 floats
        }
    };
    static void pairs(float* ws, size_t N, float* buf[4]) {
        const Ws w(ws, N);
        for (int i = 0; i < 4; ++i) buf[i] = w.buf[i];
    }
    static const char* extra_check(const Opts* o) {
        return (!(o->kappa >= 0.f) || !(o->kappa <= 3.0e38f)) ? "ukf: kappa must be finite and >= 0" : nullptr;
    }
    static const char* extra_check(long n) { return n > 0x7fffffffL / (kUkfPts * 13) ? "ukf: 25 n exceeds the step launch" : nullptr; }
    static Opts lqg_opts(const ac_sense_opts* s, const ac_lqg_opts* o) {
        return {{s->mag_ned[0], s->mag_ned[1], s->mag_ned[2]}, 1, o->kappa};
    }

    // one step: k_ukf_sigma, the handle's forward step over the 25 n units, k_ukf_update.  ll_in: added to this step's ll (or NULL).
    static int step_impl(ac_handle* h, const Opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                         const int* mask, const float* Qd, const float* Rd, long n, const float* ll_in, float* Xo, float* Po,
                         float* nu, float* S, float* nis, float* ll, int* used, int* status, float* Xpred, float* Ppred,
                         float* Abar, float* ws, void* stream) {
        const Ws w(ws, (size_t)n);
        const UkfWeights wt = ukf_weights(o->kappa);
        int grid = 0, lds = 0;
        if (o->predict) {
            const UkfSigIo sio{X, P, U, w.Xw, w.Uw, w.Lw, w.flag, n};
            AC_HIP(ukf_launch_sigma(wt, sio, (hipStream_t)stream, &grid, &lds));
            note_launch(h, "k_ukf_sigma", grid, kUkfGroups * kEkfLanes, lds);
            const int rc = ac::step_impl(h, w.Xw, w.Uw, dt, nullptr, kUkfPts * n, kUkfPts * n, w.Fw, stream);
            if (rc != AC_OK) return rc;
        }
        const UkfIo io{X, P, w.Fw, w.Lw, w.flag, Z, Qd, Rd, mask, ll_in, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, n};
        AC_HIP(ukf_launch_update(*o, wt, h->dp.p.epsilon, io, (hipStream_t)stream, &grid, &lds));
        note_launch(h, "k_ukf_update", grid, kUkfGroups * kEkfLanes, lds);
        return AC_OK;
    }
};

// a message with the estimator's name in it (fmt holds %s once, or twice for the same name)
int est_fail(int code, const char* fmt, const char* name) {
    snprintf(g_err, sizeof(g_err), fmt, name, name);
    return code;
}

// the checks the entry points share; *go = false: nothing to do (AC_OK)
template <class E>
int est_check(ac_handle* h, const typename E::Opts* o, float dt, long n, long T, const float* ws, size_t ws_floats, bool* go) {
    *go = false;
    if (!h || !o || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (o->predict && (!(dt > 0.f) || !(dt <= 3.0e38f))) return est_fail(AC_ERR_BAD_ARG, "%s: dt must be finite and > 0", E::kName);
    if (const char* why = E::extra_check(o)) return fail(AC_ERR_BAD_ARG, why);
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    if (n == 0 || T == 0) return AC_OK;
    if (const char* why = E::extra_check(n)) return fail(AC_ERR_BAD_ARG, why);
    const int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (!ws || ws_floats < E::ws_floats(n)) return est_fail(AC_ERR_WORKSPACE, "%s workspace too small: see ac_%s_workspace_floats", E::kName);
    *go = true;
    return AC_OK;
}

template <class E> int est_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *floats = E::ws_floats(n);
    return AC_OK;
}

template <class E>
int est_step(ac_handle* h, const typename E::Opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
             const int* mask, const float* Qd, const float* Rd, long n, float* Xo, float* Po, float* nu, float* S, float* nis,
             float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = est_check<E>(h, o, dt, n, 1, ws, ws_floats, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X || !P || !Z || !Rd || !Xo || !Po || !nu || !S || !nis || !ll || !used || !status)
        return est_fail(AC_ERR_BAD_ARG, "%s step: a required pointer is NULL", E::kName);
    if (o->predict && (!U || !Qd)) return est_fail(AC_ERR_BAD_ARG, "%s step: U and Qd are required when predict is set", E::kName);
    return E::step_impl(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, nullptr, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, ws,
                        stream);
}

template <class E>
int est_filter_rec(ac_handle* h, const typename E::Opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                   const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po, float* ll, float* Xs,
                   float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds, float* Ppreds, float* Abars,
                   float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = est_check<E>(h, o, dt, n, T, ws, ws_floats, &go);
    if (rc != AC_OK || !go) return rc;
    float* buf[4];
    E::pairs(ws, (size_t)n, buf);
    const auto step = [&](auto... a) { return E::step_impl(h, o, a..., ws, stream); };
    return filter_loop(E::kName, o->predict, step, buf, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used,
                       status, Xpreds, Ppreds, Abars, stream);
}
}  // namespace

extern "C" {

int ac_ekf_workspace_floats(const ac_handle* h, long n, size_t* floats) { return est_workspace_floats<Ekf>(h, n, floats); }
int ac_ukf_workspace_floats(const ac_handle* h, long n, size_t* floats) { return est_workspace_floats<Ukf>(h, n, floats); }

int ac_ekf_measure_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, long n, float* Z, void* stream) {
    AC_ENTER(h);
    if (!h || !o || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !Z) return fail(AC_ERR_BAD_ARG, "ekf measure: X and Z must not be NULL");
    int grid = 0;
    AC_HIP(ekf_launch_measure(*o, h->dp.p.epsilon, X, n, Z, (hipStream_t)stream, &grid));
    note_launch(h, "k_ekf_measure", grid, kEkfBlock, 0);
    return AC_OK;
}

int ac_ekf_step_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                    const int* mask, const float* Qd, const float* Rd, long n, float* Xo, float* Po, float* nu, float* S, float* nis,
                    float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar, float* ws, size_t ws_floats,
                    void* stream) {
    return est_step<Ekf>(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, ws, ws_floats,
                         stream);
}
int ac_ukf_step_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                    const int* mask, const float* Qd, const float* Rd, long n, float* Xo, float* Po, float* nu, float* S, float* nis,
                    float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar, float* ws, size_t ws_floats,
                    void* stream) {
    return est_step<Ukf>(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, ws, ws_floats,
                         stream);
}

int ac_ekf_filter_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                      const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po, float* ll, float* Xs,
                      float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* ws, size_t ws_floats, void* stream) {
    return ac_ekf_filter_rec_f32(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status, nullptr,
                                 nullptr, nullptr, ws, ws_floats, stream);
}
int ac_ukf_filter_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                      const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po, float* ll, float* Xs,
                      float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* ws, size_t ws_floats, void* stream) {
    return ac_ukf_filter_rec_f32(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status, nullptr,
                                 nullptr, nullptr, ws, ws_floats, stream);
}

int ac_ekf_filter_rec_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt,
                          const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                          float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds,
                          float* Ppreds, float* Abars, float* ws, size_t ws_floats, void* stream) {
    return est_filter_rec<Ekf>(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status, Xpreds, Ppreds,
                               Abars, ws, ws_floats, stream);
}
int ac_ukf_filter_rec_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt,
                          const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                          float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds,
                          float* Ppreds, float* Abars, float* ws, size_t ws_floats, void* stream) {
    return est_filter_rec<Ukf>(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status, Xpreds, Ppreds,
                               Abars, ws, ws_floats, stream);
}

}  // extern "C"

// ---- the loop closed through the estimator (ac_lqg.hpp, lqg_inst.hip) ---------------------------------------------------------------
namespace {
constexpr long kLqgLoopFloats = 2 * 13 + 2 * 13 + 2 * 144 + 7 + 15 + 1;  // truth x2 | x^ x2 | P x2 | u | z | mask per instance
constexpr size_t kLqgWsPad = 10 * 64;  // the loop's nine buffers and the estimator's workspace each start on a 256-byte boundary
template <class E> size_t lqg_ws_floats(long n) { return E::ws_floats(n) + (size_t)n * (size_t)kLqgLoopFloats + kLqgWsPad; }
// f(Ekf{}) or f(Ukf{}) for an ac_estimator the caller has checked: the loop's body is compiled once per estimator
template <class F> auto with_estimator(int estimator, F&& f) { return estimator == AC_EST_UKF ? f(Ukf{}) : f(Ekf{}); }

bool lqg_sense_opts_ok(const ac_sense_opts* o) {
    for (int j = 0; j < kLqgGroups; ++j)
        if (o->period[j] < 1 || !(o->dropout[j] >= 0.f) || !(o->dropout[j] < 1.f)) return false;
    return true;
}
bool lqg_limits_ok(const ac_ilqr_cost* c) {
    for (int i = 0; i < 7; ++i)
        if (!(c->u_min[i] <= c->u_max[i])) return false;  // (false for a NaN bound)
    return true;
}
LqgLimits lqg_limits(const ac_ilqr_cost* c) {
    LqgLimits l;
    memcpy(l.u_min, c->u_min, sizeof(l.u_min));
    memcpy(l.u_max, c->u_max, sizeof(l.u_max));
    return l;
}
// the checks every entry point here shares; *go = false: nothing to do (AC_OK)
int lqg_check(ac_handle* h, long n, bool* go) {
    *go = false;
    if (!h) return AC_ERR_BAD_ARG;
    if (n < 0) return fail(AC_ERR_BAD_ARG, "lqg: n must be >= 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *go = n > 0;
    return AC_OK;
}
}  // namespace

extern "C" {

int ac_sense_f32(ac_handle* h, const ac_sense_opts* o, int step, const int* step_dev, const float* X, const float* sigma_r, long n,
                 float* Z, int* mask, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK) return rc;
    if (!o || !lqg_sense_opts_ok(o)) return fail(AC_ERR_BAD_ARG, "sense: period must be >= 1 and dropout in [0, 1)");
    if (!go) return AC_OK;
    if (!X || !sigma_r || !Z || !mask) return fail(AC_ERR_BAD_ARG, "sense: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_sense(*o, h->dp.p.epsilon, step, step_dev, X, sigma_r, n, Z, mask, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_disturb_f32(ac_handle* h, const ac_sense_opts* o, int step, const int* step_dev, const float* X, const float* sigma_q, long n,
                   float* Xo, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK) return rc;
    if (!o) return fail(AC_ERR_BAD_ARG, "disturb: the options are NULL");
    if (!go) return AC_OK;
    if (!X || !sigma_q || !Xo) return fail(AC_ERR_BAD_ARG, "disturb: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_disturb(*o, step, step_dev, X, sigma_q, n, Xo, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_policy_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* Fb, const float* Xnom, const float* Unom, const float* Kx,
                  long n, float* U, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK) return rc;
    if (!limits || !lqg_limits_ok(limits)) return fail(AC_ERR_BAD_ARG, "policy: limits with u_min <= u_max are required");
    if (!go) return AC_OK;
    if (!Fb || !Xnom || !Unom || !Kx || !U) return fail(AC_ERR_BAD_ARG, "policy: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_control(lqg_limits(limits), Fb, Xnom, Unom, Kx, n, U, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_control", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_estimate_score_f32(ac_handle* h, const float* X, const float* Xhat, const float* P, long n, float* e, float* nees, int* status,
                          void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X || !Xhat || !P || !e || !nees || !status) return fail(AC_ERR_BAD_ARG, "estimate score: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_score(X, Xhat, P, n, e, nees, status, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_score", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_lqg_workspace_floats(const ac_handle* h, int estimator, long n, size_t* floats) {
    if (!h || !floats || n < 0 || (estimator != AC_EST_EKF && estimator != AC_EST_UKF)) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *floats = with_estimator(estimator, [&](auto est) { return lqg_ws_floats<decltype(est)>(n); });
    return AC_OK;
}

int ac_lqg_rollout_f32(ac_handle* h, const ac_lqg_opts* o, const ac_sense_opts* s, const ac_ilqr_cost* limits, const float* X0,
                       const float* Xhat0, const float* P0, const float* Xnom, const float* Unom, const float* Kx, const float* Qd,
                       const float* Rd, const float* sigma_q, const float* sigma_r, float dt, long n, long T, float* Xo, float* Po,
                       float* Xtrue, float* Xhat, float* U, float* Ps, float* Z, int* mask, float* nis, float* nees, int* used,
                       int* est_status, int* score_status, float* err, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h) return AC_ERR_BAD_ARG;
    if (!o || !s || !limits || n < 0 || T < 0) return fail(AC_ERR_BAD_ARG, "lqg: NULL options or limits, n < 0 or T < 0");
    if ((long long)o->step0 + (long long)T > 0x7fffffffLL) return fail(AC_ERR_BAD_ARG, "lqg: step0 + T exceeds the 32-bit step index");
    if (o->estimator != AC_EST_EKF && o->estimator != AC_EST_UKF) return fail(AC_ERR_BAD_ARG, "lqg: unknown estimator");
    if (o->feedback != AC_FB_ESTIMATE && o->feedback != AC_FB_TRUTH) return fail(AC_ERR_BAD_ARG, "lqg: unknown feedback");
    if (!lqg_sense_opts_ok(s)) return fail(AC_ERR_BAD_ARG, "lqg: period must be >= 1 and dropout in [0, 1)");
    if (!lqg_limits_ok(limits)) return fail(AC_ERR_BAD_ARG, "lqg: limits need u_min <= u_max");
    return with_estimator(o->estimator, [&](auto est) -> int {
        using E = decltype(est);
        const typename E::Opts eo = E::lqg_opts(s, o);
        // the estimator's own checks (dt, kappa, the quadrotor, the model, n == 0 or T == 0), against its part of the workspace
        bool go = false;
        const size_t est_floats = E::ws_floats(n);
        const bool ws_ok = ws && ws_floats >= lqg_ws_floats<E>(n);
        int rc = est_check<E>(h, &eo, dt, n, T, ws_ok ? ws : nullptr, est_floats, &go);
        if (rc == AC_ERR_WORKSPACE) return fail(AC_ERR_WORKSPACE, "lqg workspace too small: see ac_lqg_workspace_floats");
        if (rc != AC_OK || !go) return rc;
        if (!X0 || !Xhat0 || !P0 || !Xnom || !Unom || !Kx || !Qd || !Rd || !sigma_r || !Xo || !Po)
            return fail(AC_ERR_BAD_ARG, "lqg: a required pointer is NULL");
        const size_t N = (size_t)n;
        hipStream_t st = (hipStream_t)stream;
        // the loop's buffers behind the estimator's workspace
        float* xt[2];
        float* xh[2];
        float* pp[2];
        xt[0] = align256(ws + est_floats);
        xt[1] = align256(xt[0] + 13 * N);
        xh[0] = align256(xt[1] + 13 * N);
        xh[1] = align256(xh[0] + 13 * N);
        pp[0] = align256(xh[1] + 13 * N);
        pp[1] = align256(pp[0] + 144 * N);
        float* const ub = align256(pp[1] + 144 * N);
        float* const zb = align256(ub + 7 * N);
        int* const mb = (int*)align256(zb + 15 * N);  // ends at most ws + est_floats + 363 N + 9 * 63 floats
        const LqgLimits lim = lqg_limits(limits);
        const bool score = err || nees || score_status;
        auto copy = [&](void* dst, const void* src, size_t floats) { return hipMemcpyAsync(dst, src, floats * sizeof(float), hipMemcpyDeviceToDevice, st); };
        if (Xtrue) AC_HIP(copy(Xtrue, X0, 13 * N));
        if (Xhat) AC_HIP(copy(Xhat, Xhat0, 13 * N));
        const float *xt_in = X0, *xh_in = Xhat0, *p_in = P0;
        int grid = 0;
        for (long t = 0; t < T; ++t) {
            const size_t k = (size_t)t;
            const bool last = t == T - 1;
            float* const xt_o = xt[t & 1];
            float* const xh_o = last ? Xo : xh[t & 1];
            float* const p_o = last ? Po : pp[t & 1];
            float* const u_k = U ? U + k * 7 * N : ub;
            float* const z_k = Z ? Z + k * 15 * N : zb;
            int* const m_k = mask ? mask + k * N : mb;
            // 1. the control law on the estimate (or the truth)
            AC_HIP(lqg_launch_control(lim, o->feedback == AC_FB_TRUTH ? xt_in : xh_in, Xnom + k * 13 * N, Unom + k * 7 * N, Kx + k * 91 * N, n,
                                      u_k, st, &grid));
            note_launch(h, "k_lqg_control", grid, kLqgBlock, 0);
            // 2. the truth: the handle's forward step, then the process noise of step step0 + k
            rc = step_impl(h, xt_in, u_k, dt, nullptr, n, n, xt_o, stream);
            if (rc != AC_OK) return rc;
            if (sigma_q) {
                AC_HIP(lqg_launch_disturb(*s, o->step0 + (int)t, nullptr, xt_o, sigma_q, n, xt_o, st, &grid));
                note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
            }
            if (Xtrue) AC_HIP(copy(Xtrue + (k + 1) * 13 * N, xt_o, 13 * N));
            // 3. the sensors at step step0 + k + 1
            AC_HIP(lqg_launch_sense(*s, h->dp.p.epsilon, o->step0 + (int)t + 1, nullptr, xt_o, sigma_r, n, z_k, m_k, st, &grid));
            note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
            // 4. the estimator's own step
            float* const nis_k = nis ? nis + k * N : nullptr;
            int* const used_k = used ? used + k * N : nullptr;
            int* const st_k = est_status ? est_status + k * N : nullptr;
            rc = E::step_impl(h, &eo, xh_in, p_in, u_k, dt, z_k, m_k, Qd, Rd, n, nullptr, xh_o, p_o, nullptr, nullptr, nis_k, nullptr, used_k,
                              st_k, nullptr, nullptr, nullptr, ws, stream);
            if (rc != AC_OK) return rc;
            if (Xhat) AC_HIP(copy(Xhat + (k + 1) * 13 * N, xh_o, 13 * N));
            if (Ps) AC_HIP(copy(Ps + k * 144 * N, p_o, 144 * N));
            // 5. the estimate against the truth
            if (score) {
                AC_HIP(lqg_launch_score(xt_o, xh_o, p_o, n, err ? err + k * 12 * N : nullptr, nees ? nees + k * N : nullptr,
                                        score_status ? score_status + k * N : nullptr, st, &grid));
                note_launch(h, "k_lqg_score", grid, kLqgBlock, 0);
            }
            xt_in = xt_o;
            xh_in = xh_o;
            p_in = p_o;
        }
        return AC_OK;
    });
}

// ---- RTS smoother over the EKF trace (ac_rts.hpp, rts_inst.hip) ---------------------------------------------------------------------
int ac_ekf_smooth_f32(ac_handle* h, const float* X0, const float* P0, const float* Xf, const float* Pf, const float* Xpred,
                      const float* Ppred, const float* Abar, long n, long T, float* Xs, float* Ps, float* Xs0, float* Ps0, float* Cg,
                      int* status, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    const int given = (X0 != nullptr) + (P0 != nullptr) + (Xs0 != nullptr) + (Ps0 != nullptr);
    if (given != 0 && given != 4) return fail(AC_ERR_BAD_ARG, "ekf smooth: X0, P0, Xs0, Ps0 go together (all or none)");
    if (n == 0 || T == 0) return AC_OK;
    if (!Xf || !Pf || !Xpred || !Ppred || !Abar || !Xs || !Ps || !status)
        return fail(AC_ERR_BAD_ARG, "ekf smooth: a required pointer is NULL");
    const size_t N = (size_t)n, K = (size_t)T;
    const RtsSpan in[] = {{X0, 13 * N}, {P0, 144 * N}, {Xf, K * 13 * N}, {Pf, K * 144 * N}, {Xpred, K * 13 * N}, {Ppred, K * 144 * N},
                          {Abar, K * 144 * N}};
    const RtsSpan out[] = {{Xs, K * 13 * N}, {Ps, K * 144 * N}, {Xs0, 13 * N}, {Ps0, 144 * N}, {Cg, K * 144 * N}};
    for (const RtsSpan& a : out)
        for (const RtsSpan& b : in)
            if (rts_overlap(a, b)) return fail(AC_ERR_BAD_ARG, "ekf smooth: an output overlaps an input");
    const RtsIo io{X0, P0, Xf, Pf, Xpred, Ppred, Abar, Xs, Ps, Xs0, Ps0, Cg, status, n, T};
    int grid = 0, lds = 0;
    AC_HIP(rts_launch_smooth(io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_ekf_smooth", grid, kRtsGroups * kEkfLanes, lds);
    return AC_OK;
}

// ---- EM statistics for the noise variances of the EKF (ac_em.hpp, em_inst.hip) --------------------------------------------------------
namespace {
constexpr size_t kEmWsPad = 2 * 64;  // the two workspace buffers each start on a 256-byte boundary
// [chunks][27][n] float64, then [chunks][16][n] int32
size_t em_ws_floats(long n, long T) { return (size_t)em_chunks(T) * (size_t)n * (size_t)(2 * kEmRows + kEmCounts) + kEmWsPad; }
}  // namespace

int ac_ekf_em_workspace_floats(const ac_handle* h, long n, long T, size_t* floats) {
    if (!h || !floats || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *floats = em_ws_floats(n, T);
    return AC_OK;
}

int ac_ekf_em_f32(ac_handle* h, const ac_ekf_em_opts* o, const float* Xpred, const float* Ppred, const float* Xs, const float* Ps,
                  const float* Z, const int* used, const float* Qd, const float* Rd, long n, long T, float* Qsum, float* Rsum,
                  int* nq, int* nr, int* status, float* Qn, float* Rn, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !o || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (!(o->floor_rel >= 0.f) || !(o->floor_rel <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "ekf em: floor_rel must be finite and >= 0 (0: 1e-4)");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    if (n == 0) return AC_OK;
    if (!Qd || !Rd || !Qsum || !Rsum || !nq || !nr || (T > 0 && (!Xpred || !Ppred || !Xs || !Ps || !Z || !used || !status)))
        return fail(AC_ERR_BAD_ARG, "ekf em: a required pointer is NULL");
    const size_t N = (size_t)n, K = (size_t)T;
    const long gb = (n + kEmGroups - 1) / kEmGroups;
    if (em_chunks(T) > 2147483647L / gb || (long)kEmRows * n / kEmBlock >= 2147483647L)
        return fail(AC_ERR_BAD_ARG, "ekf em: n * T exceeds the launch dimension");
    if (!ws || ws_floats < em_ws_floats(n, T)) return fail(AC_ERR_WORKSPACE, "ekf em workspace too small: see ac_ekf_em_workspace_floats");
    const RtsSpan in[] = {{Xpred, K * 13 * N}, {Ppred, K * 144 * N}, {Xs, K * 13 * N}, {Ps, K * 144 * N}, {Z, K * 15 * N},
                          {(const float*)used, K * N}, {Qd, 12 * N}, {Rd, 15 * N}};
    const RtsSpan out[] = {{Qsum, 12 * N}, {Rsum, 15 * N}, {(const float*)nq, N}, {(const float*)nr, 15 * N},
                           {(const float*)status, K * N}, {Qn, 12 * N}, {Rn, 15 * N}, {ws, ws_floats}};
    if (modes_overlap(out, 8, in, 8)) return fail(AC_ERR_BAD_ARG, "ekf em: an output overlaps an input");
    double* const part = (double*)align256(ws);
    int* const cnt = (int*)align256((float*)part + (size_t)em_chunks(T) * 2 * kEmRows * N);  // ends at most ws + 70 chunks N + 2 * 63 floats
    EmIo io{Xpred, Ppred, Xs, Ps, Z, used, Qd, Rd, part, cnt, Qsum, Rsum, nq, nr, status, Qn, Rn, {o->mag_ned[0], o->mag_ned[1], o->mag_ned[2]},
            h->dp.p.epsilon, o->floor_rel, n, T};
    int grid = 0, lds = 0;
    AC_HIP(em_launch(io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, T > 0 ? "k_ekf_em_nodes" : "k_ekf_em_reduce", grid, kEmGroups * kEkfLanes, lds);
    return AC_OK;
}

// ---- iterated extended Kalman smoother (ac_ieks.hpp, ieks_inst.hip) -----------------------------------------------------------------
namespace {
// The workspace: F [T][13][n] | A [T][169][n] | B [T][91][n] (the pass) | the cost's region for `cols` columns: F [T][13][cols] |
// partial sums [chunks][2][cols] float64 | status [chunks][cols] int32 | then the solve's own: Xc [T+1][13][cols] | Uc [T][7][cols] |
// Jc [cols] | stc [cols] int32 | the smoother's status [T][n] int32.  Every buffer starts on a 256-byte boundary.
struct IeksCostWs {
    float* Fc;
    double* part;
    int* pst;
    float* end;
    IeksCostWs(float* ws, size_t cols, size_t K) {
        Fc = align256(ws);
        part = (double*)align256(Fc + K * 13 * cols);
        pst = (int*)align256((float*)part + (size_t)ieks_chunks((long)K) * 4 * cols);
        end = (float*)pst + (size_t)ieks_chunks((long)K) * cols;
    }
};
struct IeksWs {
    float *F, *A, *Bm, *cost, *Xc, *Uc, *Jc, *end;
    int *stc, *rst;
    float* pass_end;
    IeksWs(float* ws, size_t N, size_t K, size_t C) {
        const size_t cols = N * (C ? C : 1);
        F = align256(ws);
        A = align256(F + K * 13 * N);
        Bm = align256(A + K * 169 * N);
        pass_end = Bm + K * 91 * N;
        cost = align256(pass_end);
        Xc = align256(IeksCostWs(cost, cols, K).end);
        Uc = align256(Xc + (K + 1) * 13 * cols);
        Jc = align256(Uc + K * 7 * cols);
        stc = (int*)align256(Jc + cols);
        rst = (int*)align256((float*)stc + cols);
        end = (float*)rst + K * N;
    }
};
constexpr size_t kIeksWsPad = 11 * 64;
size_t ieks_pass_floats(long n, long T) { return (size_t)(IeksWs(nullptr, (size_t)n, (size_t)T, 1).pass_end - (float*)nullptr) + 3 * 64; }
size_t ieks_cost_floats(long cols, long T) { return (size_t)(IeksCostWs(nullptr, (size_t)cols, (size_t)T).end - (float*)nullptr) + 3 * 64; }
size_t ieks_ws_floats(long n, long T, int C) { return (size_t)(IeksWs(nullptr, (size_t)n, (size_t)T, (size_t)C).end - (float*)nullptr) + kIeksWsPad; }
const char* const kIeksFixedWing = "the iterated Kalman smoother is defined for the fixed-wing models only";

int ieks_ladder(const float* ladder, int candidates, IeksLadder* lad) {
    if (!ladder || candidates < 1 || candidates > kIeksMaxCand) return fail(AC_ERR_BAD_ARG, "ieks: the ladder has 1 .. 8 values");
    lad->count = candidates;
    for (int c = 0; c < kIeksMaxCand; ++c) lad->a[c] = 0.f;
    for (int c = 0; c < candidates; ++c) {
        if (!(ladder[c] > 0.f) || !(ladder[c] <= 1.0f)) return fail(AC_ERR_BAD_ARG, "ieks: the ladder's values must lie in (0, 1]");
        lad->a[c] = ladder[c];
    }
    return AC_OK;
}

// the checks the entry points share; *go = false: nothing to do (AC_OK)
int ieks_check(ac_handle* h, const ac_ekf_opts* o, float dt, long n, long T, bool* go) {
    *go = false;
    if (!h || !o || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (!(dt > 0.f) || !(dt <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "ieks: dt must be finite and > 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    if (n == 0 || T == 0) return AC_OK;
    if (T + 1 > 2147483647L / ((n * kIeksMaxCand + kIeksBlock - 1) / kIeksBlock + 1)) return fail(AC_ERR_BAD_ARG, "ieks: n * T exceeds the launch dimension");
    const int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    *go = true;
    return AC_OK;
}

int ieks_pass_impl(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xbar, const float* U, float dt,
                   const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xs, float* Ps, float* ll,
                   float* nu, float* S, float* nis, int* used, int* status, float* Xpreds, float* Ppreds, float* Abars, float* ws,
                   void* stream) {
    const IeksWs w(ws, (size_t)n, (size_t)T, 1);
    const int rc = sens_impl(h, Xbar, U, dt, nullptr, n * T, n, w.F, w.A, w.Bm, nullptr, stream);
    if (rc != AC_OK) return rc;
    const IeksIo io{X0, P0, Xbar, w.F, w.A, Z, Qd, Rd, mask, Xs, Ps, ll, nu, S, nis, used, status, Xpreds, Ppreds, Abars, n, T};
    int grid = 0, lds = 0;
    AC_HIP(ieks_launch_filter(*o, h->dp.p.epsilon, io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_ieks_filter", grid, kIeksGroups * kEkfLanes, lds);
    return AC_OK;
}

// wsc: a region of at least ieks_cost_floats(reps n, T) floats
int ieks_cost_impl(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xt, const float* Ut, float dt,
                   const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long reps, long T, float* J, float* Jprior,
                   float* Jproc, float* Jmeas, int* status, float* wsc, void* stream) {
    const long cols = n * reps;
    const IeksCostWs w(wsc, (size_t)cols, (size_t)T);
    const int rc = step_impl(h, Xt, Ut, dt, nullptr, cols * T, cols, w.Fc, stream);
    if (rc != AC_OK) return rc;
    const IeksCostIo io{X0, P0, Xt, w.Fc, Z, Qd, Rd, mask, w.part, w.pst, J, Jprior, Jproc, Jmeas, status,
                        {o->mag_ned[0], o->mag_ned[1], o->mag_ned[2]}, h->dp.p.epsilon, n, reps, T};
    int grid = 0;
    AC_HIP(ieks_launch_cost(io, (hipStream_t)stream, &grid));
    note_launch(h, "k_ieks_cost_nodes", grid, kIeksBlock, 0);
    return AC_OK;
}
}  // namespace

int ac_ieks_workspace_floats(const ac_handle* h, long n, long T, int candidates, size_t* floats) {
    if (!h || !floats || n < 0 || T < 0 || candidates < 0 || candidates > kIeksMaxCand) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    *floats = ieks_ws_floats(n, T, candidates);
    return AC_OK;
}

int ac_ieks_pass_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xbar, const float* U, float dt,
                     const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xs, float* Ps, float* ll,
                     float* nu, float* S, float* nis, int* used, int* status, float* Xpreds, float* Ppreds, float* Abars, float* ws,
                     size_t ws_floats, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = ieks_check(h, o, dt, n, T, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X0 || !P0 || !Xbar || !U || !Z || !Qd || !Rd || !Xs || !Ps || !Xpreds || !Ppreds || !Abars)
        return fail(AC_ERR_BAD_ARG, "ieks pass: a required pointer is NULL");
    if (!ws || ws_floats < ieks_pass_floats(n, T)) return fail(AC_ERR_WORKSPACE, "ieks workspace too small: see ac_ieks_workspace_floats");
    return ieks_pass_impl(h, o, X0, P0, Xbar, U, dt, Z, mask, Qd, Rd, n, T, Xs, Ps, ll, nu, S, nis, used, status, Xpreds, Ppreds, Abars,
                          ws, stream);
}

int ac_ieks_cost_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xtraj, const float* Utraj,
                     float dt, const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long reps, long T, float* J,
                     float* Jprior, float* Jproc, float* Jmeas, int* status, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (reps < 1 || reps > kIeksMaxCand) return fail(AC_ERR_BAD_ARG, "ieks cost: reps must be 1 .. 8");
    bool go = false;
    const int rc = ieks_check(h, o, dt, n, T, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X0 || !P0 || !Xtraj || !Utraj || !Z || !Qd || !Rd || !J || !status)
        return fail(AC_ERR_BAD_ARG, "ieks cost: a required pointer is NULL");
    if (!ws || ws_floats < ieks_cost_floats(n * reps, T)) return fail(AC_ERR_WORKSPACE, "ieks workspace too small: see ac_ieks_workspace_floats");
    return ieks_cost_impl(h, o, X0, P0, Xtraj, Utraj, dt, Z, mask, Qd, Rd, n, reps, T, J, Jprior, Jproc, Jmeas, status, ws, stream);
}

int ac_ieks_candidates_f32(ac_handle* h, const float* Xbar, const float* Xs0, const float* Xs, const float* U, const float* ladder,
                           int candidates, long n, long T, float* Xc, float* Uc, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    IeksLadder lad;
    const int rc = ieks_ladder(ladder, candidates, &lad);
    if (rc != AC_OK) return rc;
    if (n == 0 || T == 0) return AC_OK;
    if (!Xbar || !Xs0 || !Xs || !U || !Xc || !Uc) return fail(AC_ERR_BAD_ARG, "ieks candidates: a required pointer is NULL");
    const IeksCandIo io{Xbar, Xs0, Xs, U, Xc, Uc, lad, n, T};
    int grid = 0;
    AC_HIP(ieks_launch_candidates(io, (hipStream_t)stream, &grid));
    note_launch(h, "k_ieks_candidates", grid, kIeksBlock, 0);
    return AC_OK;
}

int ac_ieks_accept_f32(ac_handle* h, const float* Jcur, const float* Jc, const int* stc, const float* Xc, const float* ladder,
                       int candidates, long n, long T, float* Xbar, float* alpha, float* Jout, int* status, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    IeksLadder lad;
    const int rc = ieks_ladder(ladder, candidates, &lad);
    if (rc != AC_OK) return rc;
    if (n == 0 || T == 0) return AC_OK;
    if (!Jcur || !Jc || !stc || !Xc || !Xbar || !alpha || !Jout || !status) return fail(AC_ERR_BAD_ARG, "ieks accept: a required pointer is NULL");
    if (rts_overlap({Jcur, (size_t)n}, {Jout, (size_t)n})) return fail(AC_ERR_BAD_ARG, "ieks accept: Jout overlaps Jcur");
    const IeksAcceptIo io{Jcur, Jc, stc, Xc, Xbar, alpha, Jout, status, lad, n, T};
    int grid = 0;
    AC_HIP(ieks_launch_accept(io, (hipStream_t)stream, &grid));
    note_launch(h, "k_ieks_accept", grid, kIeksBlock, 0);
    return AC_OK;
}

int ac_ieks_solve_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, float* Xbar, const float* U, float dt,
                      const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, int iters, const float* ladder,
                      int candidates, float* Xs, float* Ps, float* Xs0, float* Ps0, float* Xf, float* Pf, float* ll, float* nu, float* S,
                      float* nis, int* used, int* fstatus, float* Xpreds, float* Ppreds, float* Abars, float* cost, float* alpha,
                      int* status, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (iters < 0) return fail(AC_ERR_BAD_ARG, "ieks solve: iters must be >= 0");
    bool go = false;
    int rc = ieks_check(h, o, dt, n, T, &go);
    if (rc != AC_OK) return rc;
    IeksLadder lad;
    rc = ieks_ladder(ladder, candidates, &lad);
    if (rc != AC_OK || !go) return rc;
    if (!X0 || !P0 || !Xbar || !U || !Z || !Qd || !Rd || !Xs || !Ps || !Xs0 || !Ps0 || !Xf || !Pf || !Xpreds || !Ppreds || !Abars || !cost ||
        !status || (iters > 0 && !alpha))
        return fail(AC_ERR_BAD_ARG, "ieks solve: a required pointer is NULL");
    if (!ws || ws_floats < ieks_ws_floats(n, T, candidates)) return fail(AC_ERR_WORKSPACE, "ieks workspace too small: see ac_ieks_workspace_floats");
    const IeksWs w(ws, (size_t)n, (size_t)T, (size_t)candidates);
    const size_t N = (size_t)n;
    rc = ieks_cost_impl(h, o, X0, P0, Xbar, U, dt, Z, mask, Qd, Rd, n, 1, T, cost, nullptr, nullptr, nullptr, status, w.cost, stream);
    for (int it = 0; it <= iters && rc == AC_OK; ++it) {
        rc = ieks_pass_impl(h, o, X0, P0, Xbar, U, dt, Z, mask, Qd, Rd, n, T, Xf, Pf, ll, nu, S, nis, used, fstatus, Xpreds, Ppreds, Abars,
                            ws, stream);
        if (rc != AC_OK) break;
        rc = ac_ekf_smooth_f32(h, X0, P0, Xf, Pf, Xpreds, Ppreds, Abars, n, T, Xs, Ps, Xs0, Ps0, nullptr, w.rst, stream);
        if (rc != AC_OK || it == iters) break;
        rc = ac_ieks_candidates_f32(h, Xbar, Xs0, Xs, U, ladder, candidates, n, T, w.Xc, w.Uc, stream);
        if (rc != AC_OK) break;
        rc = ieks_cost_impl(h, o, X0, P0, w.Xc, w.Uc, dt, Z, mask, Qd, Rd, n, candidates, T, w.Jc, nullptr, nullptr, nullptr, w.stc, w.cost,
                            stream);
        if (rc != AC_OK) break;
        rc = ac_ieks_accept_f32(h, cost + (size_t)it * N, w.Jc, w.stc, w.Xc, ladder, candidates, n, T, Xbar, alpha + (size_t)it * N,
                                cost + (size_t)(it + 1) * N, status, stream);
    }
    return rc;
}

}  // extern "C"
