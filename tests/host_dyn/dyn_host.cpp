// dyn_host.cpp — the kernels' own arithmetic headers (ac_math.hpp, ac_dynamics.hpp) compiled for the HOST (g++,
// -DAC_HOST_CHECK) behind a small C API, so that `pytest -m "not gpu"` can check the device math (fp32 forward-mode
// tangents of the RK4 step, lane group by lane group) against the float64 oracle without a GPU.  TEST INFRASTRUCTURE:
// nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include <cmath>
#include <cstring>

#include "../../aircraft_amd/csrc/ac_adjoint.hpp"

using namespace ac;

namespace {

template <int N, bool QUAD> void scatter(int g, const Dual<N> x[13], float* A, float* B, float* c) {
    for (int j = 0; j < N; ++j) {
        const int d = N * g + j;
        for (int i = 0; i < 13; ++i) {
            if (d < 10) A[i * 13 + 3 + d] = x[i].d[j];
            else if (d < 13) B[i * 7 + (d - 10)] = x[i].d[j];
            else if (d == 13) B[i * 7 + (QUAD ? 3 : 6)] = x[i].d[j];
            else if (d == 14) c[i] = x[i].d[j];
        }
    }
}

template <int N, class Coeffs> void unit_step_sens_with(const DevParams& P, Coeffs& coeffs, const float xv[13], const float uv[7],
                                                        float dt, float xn[13], float A[169], float B[91], float c[13]) {
    for (int i = 0; i < 169; ++i) A[i] = 0.f;
    for (int i = 0; i < 91; ++i) B[i] = 0.f;
    for (int i = 0; i < 3; ++i) A[i * 13 + i] = 1.f;  // dF/dp = [I; 0]
    for (int g = 0; g < 16 / N; ++g) {
        Dual<N> x[13];
        rk4_step_seeded<N>(P, coeffs, g, xv, uv, dt, 1.0f, x);
        if (P.p.normalise) normalise_q(x);
        scatter<N, Coeffs::kModel == AC_MODEL_QUAD>(g, x, A, B, c);
        for (int i = 0; i < 13; ++i) xn[i] = x[i].v;
    }
}

template <int MODEL, int N> void unit_step_sens(const DevParams& P, const float xv[13], const float uv[7], float dt,
                                                float xn[13], float A[169], float B[91], float c[13]) {
    AnalyticCoeffs<MODEL> coeffs;
    unit_step_sens_with<N>(P, coeffs, xv, uv, dt, xn, A, B, c);
}

template <int MODEL, int N> void unit_deriv_sens(const DevParams& P, const float xv[13], const float uv[7],
                                                 float xd[13], float Fx[169], float Fu[91]) {
    for (int i = 0; i < 169; ++i) Fx[i] = 0.f;
    for (int i = 0; i < 91; ++i) Fu[i] = 0.f;
    float cdummy[13];
    AnalyticCoeffs<MODEL> coeffs;
    for (int g = 0; g < 16 / N; ++g) {
        Dual<N> xs[13], u[7], k[13];
        for (int i = 0; i < 13; ++i) xs[i] = SeedsT<N>::state(g, i, xv[i]);
        SeedsT<N>::template controls<MODEL == AC_MODEL_QUAD>(g, uv, u);
        state_derivative(P, coeffs, xs, u, k);
        scatter<N, MODEL == AC_MODEL_QUAD>(g, k, Fx, Fu, cdummy);
        for (int i = 0; i < 13; ++i) xd[i] = k[i].v;
    }
}

template <int MODEL, int N>
void run(const DevParams& P, int what, const float* X, const float* U, float dt, long n, float* Xn, float* A, float* B,
         float* c) {
    for (long u = 0; u < n; ++u) {
        float xv[13], uv[7], xn[13], a[169], b[91], cc[13] = {0};
        for (int i = 0; i < 13; ++i) xv[i] = X[i * n + u];
        for (int i = 0; i < 7; ++i) uv[i] = U[i * n + u];
        if (what == 0) unit_step_sens<MODEL, N>(P, xv, uv, dt, xn, a, b, cc);
        else unit_deriv_sens<MODEL, N>(P, xv, uv, xn, a, b);
        for (int i = 0; i < 13; ++i) Xn[i * n + u] = xn[i];
        for (int i = 0; i < 169; ++i) A[i * n + u] = a[i];
        for (int i = 0; i < 91; ++i) B[i * n + u] = b[i];
        if (c) for (int i = 0; i < 13; ++i) c[i * n + u] = cc[i];
    }
}

// gradient of lam . F over z = (x[13], u[7], dt) by the reverse sweep in plain floats, and its Hessian by the same sweep in
// duals (N directions at a time) — ac_adjoint.hpp
template <int MODEL, int N> void unit_adjoint(const DevParams& P, const float xv[13], const float uv[7], float dt, const float lam[13],
                                              float grad[21], float Hm[441]) {
    AdjAnalyticCoeffs<MODEL> coeffs;
    {
        float xo[13], gx[13], gu[7], gh;
        rk4_vjp<float>(P, coeffs, xv, uv, dt, lam, xo, gx, gu, gh);
        for (int i = 0; i < 13; ++i) grad[i] = gx[i];
        for (int i = 0; i < 7; ++i) grad[13 + i] = gu[i];
        grad[20] = gh;
    }
    for (int i = 0; i < 441; ++i) Hm[i] = 0.f;
    for (int g = 0; g < (21 + N - 1) / N; ++g) {
        typedef Dual<N> T;
        T x[13], u[7], h(dt);
        for (int i = 0; i < 13; ++i) x[i] = T(xv[i]);
        for (int i = 0; i < 7; ++i) u[i] = T(uv[i]);
        for (int j = 0; j < N; ++j) {
            const int z = N * g + j;
            if (z < 13) x[z].d[j] = 1.f;
            else if (z < 20) u[z - 13].d[j] = 1.f;
            else if (z == 20) h.d[j] = 1.f;
        }
        T xo[13], gx[13], gu[7], gh;
        rk4_vjp<T>(P, coeffs, x, u, h, lam, xo, gx, gu, gh);
        for (int j = 0; j < N; ++j) {
            const int z = N * g + j;
            if (z > 20) continue;
            for (int i = 0; i < 13; ++i) Hm[i * 21 + z] = gx[i].d[j];
            for (int i = 0; i < 7; ++i) Hm[(13 + i) * 21 + z] = gu[i].d[j];
            Hm[20 * 21 + z] = gh.d[j];
        }
    }
}

}  // namespace

extern "C" int host_dyn_adjoint(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept, int N,
                                const float* X, const float* U, float dt, const float* Lam, long n, float* grad /*[21][n]*/,
                                float* Hm /*[21][21][n]*/) {
    DevParams P{};
    P.p = *p;
    if (linear_W) for (int i = 0; i < 36; ++i) P.linear_W[i] = linear_W[i];
    alignas(64) static thread_local float tab[kPolyTabFloats];
    if (poly_coef && poly_intercept) {
        float gradt[6 * 4 * 15], hesst[6 * 10 * 5];
        poly_gradient_tables(poly_coef, gradt);
        poly_hessian_tables(gradt, hesst);
        poly_pack_tables(poly_coef, poly_intercept, gradt, hesst, tab);
        P.poly_tab = tab;
    }
    if (P.p.substeps > 1) return -1;
    for (long u = 0; u < n; ++u) {
        float xv[13], uv[7], lam[13], g[21], H[441];
        for (int i = 0; i < 13; ++i) { xv[i] = X[i * n + u]; lam[i] = Lam[i * n + u]; }
        for (int i = 0; i < 7; ++i) uv[i] = U[i * n + u];
        bool done = false;
#define AC_CASE(M_, N_) if (!done && P.p.model_kind == M_ && N == N_) { unit_adjoint<M_, N_>(P, xv, uv, dt, lam, g, H); done = true; }
        AC_CASE(AC_MODEL_DEFAULT, 1) AC_CASE(AC_MODEL_DEFAULT, 2) AC_CASE(AC_MODEL_DEFAULT, 4)
        AC_CASE(AC_MODEL_LINEAR, 1) AC_CASE(AC_MODEL_LINEAR, 2) AC_CASE(AC_MODEL_QUAD, 2)
        AC_CASE(AC_MODEL_POLY, 1) AC_CASE(AC_MODEL_POLY, 2)
#undef AC_CASE
        if (!done) return -2;
        for (int i = 0; i < 21; ++i) grad[i * n + u] = g[i];
        for (int i = 0; i < 441; ++i) Hm[i * n + u] = H[i];
    }
    return 0;
}

// what: 0 = one RK4 step with A, B, c (substeps must be 1); 1 = f with df/dx, df/du.  N = tangent directions per lane
// group (2, 4 or 8).  Arrays component-major like the device ABI: X [13][n], A [13][13][n], ...
extern "C" int host_dyn_sens(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                             int what, int N, const float* X, const float* U, float dt, long n, float* Xn, float* A,
                             float* B, float* c) {
    DevParams P{};
    P.p = *p;
    if (linear_W) for (int i = 0; i < 36; ++i) P.linear_W[i] = linear_W[i];
    alignas(64) static thread_local float tab[kPolyTabFloats];
    if (poly_coef && poly_intercept) {
        float grad[6 * 4 * 15], hess[6 * 10 * 5];
        poly_gradient_tables(poly_coef, grad);
        poly_hessian_tables(grad, hess);
        poly_pack_tables(poly_coef, poly_intercept, grad, hess, tab);
        P.poly_tab = tab;
    }
    if (what == 0 && P.p.substeps > 1) return -1;
#define AC_CASE(M_, N_) if (P.p.model_kind == M_ && N == N_) { run<M_, N_>(P, what, X, U, dt, n, Xn, A, B, c); return 0; }
    AC_CASE(AC_MODEL_DEFAULT, 2) AC_CASE(AC_MODEL_DEFAULT, 4) AC_CASE(AC_MODEL_DEFAULT, 8)
    AC_CASE(AC_MODEL_LINEAR, 2) AC_CASE(AC_MODEL_LINEAR, 4) AC_CASE(AC_MODEL_LINEAR, 8)
    AC_CASE(AC_MODEL_POLY, 2) AC_CASE(AC_MODEL_POLY, 4) AC_CASE(AC_MODEL_POLY, 8)
    AC_CASE(AC_MODEL_QUAD, 2) AC_CASE(AC_MODEL_QUAD, 4) AC_CASE(AC_MODEL_QUAD, 8)
#undef AC_CASE
    return -2;
}

// Value, gradient and second derivatives of fit k at the points F [4][n] through the PACKED tables and the device's own
// streaming evaluators (poly_value_grad, poly_hess): out [15][n] = val, g[4], h[10] (entry order: PolyTab::hess_row).
extern "C" int host_poly_point(const float* poly_coef, const float* poly_intercept, int k, const float* F, long n, float* out) {
    DevParams P{};
    alignas(64) static thread_local float tab[kPolyTabFloats];
    float grad[6 * 4 * 15], hess[6 * 10 * 5];
    poly_gradient_tables(poly_coef, grad);
    poly_hessian_tables(grad, hess);
    poly_pack_tables(poly_coef, poly_intercept, grad, hess, tab);
    P.poly_tab = tab;
    if (k < 0 || k > 5) return -1;
    for (long u = 0; u < n; ++u) {
        const float f[4] = {F[u], F[n + u], F[2 * n + u], F[3 * n + u]};
        const int ks[1] = {k};
        float val[1], g[1][4], h[1][10];
        poly_value_grad<1>(P, ks, f, val, g);
        poly_hess<1>(P, ks, f, h);
        out[u] = val[0];
        for (int v = 0; v < 4; ++v) out[(1 + v) * n + u] = g[0][v];
        for (int e = 0; e < 10; ++e) out[(5 + e) * n + u] = h[0][e];
    }
    return 0;
}

// ---- the MLP surrogate's step with tangents, restated -----------------------------------------------------------------
// A coefficient provider to the protocol of ac_dynamics.hpp (prefetch, operator() for float and Dual<N>, no kFusedTangent:
// rk4_step_seeded takes the phase-structured path) over a plain network evaluation written HERE, not ac_mlp.hpp's:
// z = (in - mean) / std, y and the unscaled J = dy/dz from the net, C = fma(y, out_std, out_mean), the rudder term on C[5],
// dC = sum_j (J jscale) d in_j with jscale = out_std / in_std rounded once (what MlpCoeffs does with the engine's y and J).
// The hidden (hidden x hidden) layers run in one of three arithmetics; the edge layers are fp32 fmaf chains in all of them:
//   0  plain fp32: every output a k-ascending fmaf chain from the bias
//   1  two-plane f16 (tests/test_mlp_f16_planes.py::layer_f16): hi = f16(x), lo' = f16((x - hi) 2^11), subnormals kept; per
//      32-deep chunk lo'.hi then hi.lo' into `lo` and hi.hi into `hi` (bias there), each 32-product sum rounded once to fp32;
//      tile = fma(lo, 2^-11, hi)
//   2  three-plane bf16: per chunk w3.x1, w1.x3, w2.x2, w2.x1, w1.x2 (smallest first) into `lo`,
//      w1.x1 alone into `hi` (bias there); tile = hi + lo
// drop: index of one product left out (mode 1: 0 lo'.hi, 1 hi.lo', 2 hi.hi; mode 2: 0 w1.x1, 1 w1.x2, 2 w2.x1, 3 w2.x2,
// 4 w1.x3, 5 w3.x1), -1 none: how the CPU test shows what the block metric can see.
namespace {

constexpr int kNetMaxWidth = 128, kNetMaxLayers = 8;

float round_f16(float x) {  // nearest even onto 11 significant bits, exponent floor -14 (gradual underflow), as a float
    const float a = std::fabs(x);
    if (!(a < 65520.f)) return x * INFINITY;
    if (a == 0.f) return x;
    int e;
    std::frexp(a, &e);  // a in [2^(e-1), 2^e)
    const int q = (e - 1 < -14 ? -14 : e - 1) - 10;
    return std::copysign(std::ldexp(std::nearbyint(std::ldexp(a, -q)), q), x);
}
float round_bf16(float x) {  // nearest even onto the top 16 bits
    unsigned u;
    std::memcpy(&u, &x, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}
int split_planes(int mode, float x, float p[3]) {  // -> number of planes
    if (mode == 1) {
        p[0] = round_f16(x);
        p[1] = round_f16((x - p[0]) * 2048.0f);
        return 2;
    }
    p[0] = round_bf16(x);
    const float r1 = x - p[0];
    p[1] = round_bf16(r1);
    p[2] = round_bf16(r1 - p[1]);
    return 3;
}

struct HostNet {
    int n_layers, widths[kNetMaxLayers + 1], act[kNetMaxLayers];
    const float* W[kNetMaxLayers];  // [widths[l + 1]][widths[l]] row-major
    const float* b[kNetMaxLayers];
    int mode, drop;
    float* wp[kNetMaxLayers];  // planes of the hidden weights, [3][nout][nin]

    static float tanh_k(float x) { return 1.0f - 2.0f / (1.0f + std::exp(2.0f * x)); }  // the kernels' formula

    // out[r][i] = sum_k W[i][k] in[r][k] (+ b[i] on row 0), rows r = value, five tangents
    void hidden(int l, const float in[6][kNetMaxWidth], float out[6][kNetMaxWidth]) const {
        const int nin = widths[l], nout = widths[l + 1];
        if (mode == 0) {
            for (int r = 0; r < 6; ++r)
                for (int i = 0; i < nout; ++i) {
                    float s = r == 0 ? b[l][i] : 0.f;
                    for (int k = 0; k < nin; ++k) s = std::fma(W[l][(long)i * nin + k], in[r][k], s);
                    out[r][i] = s;
                }
            return;
        }
        // product list in the order it enters the accumulators: {weight plane, activation plane, accumulator (0 hi, 1 lo), drop index}
        static const int kF16[3][4] = {{1, 0, 1, 0}, {0, 1, 1, 1}, {0, 0, 0, 2}};
        static const int kBf16[6][4] = {{2, 0, 1, 5}, {0, 2, 1, 4}, {1, 1, 1, 3}, {1, 0, 1, 2}, {0, 1, 1, 1}, {0, 0, 0, 0}};
        const int (*prod)[4] = mode == 1 ? kF16 : kBf16;
        const int nprod = mode == 1 ? 3 : 6;
        const float* w = wp[l];
        for (int r = 0; r < 6; ++r) {
            float xp[3][kNetMaxWidth];
            for (int k = 0; k < nin; ++k) {
                float p[3] = {0.f, 0.f, 0.f};
                split_planes(mode, in[r][k], p);
                for (int q = 0; q < 3; ++q) xp[q][k] = p[q];
            }
            for (int i = 0; i < nout; ++i) {
                float acc[2] = {r == 0 ? b[l][i] : 0.f, 0.f};
                for (int k0 = 0; k0 < nin; k0 += 32) {
                    const int k1 = k0 + 32 < nin ? k0 + 32 : nin;
                    for (int t = 0; t < nprod; ++t) {
                        if (prod[t][3] == drop) continue;
                        const float* wr = w + ((long)prod[t][0] * nout + i) * nin;
                        const float* xr = xp[prod[t][1]];
                        double s = 0.0;  // (products of 8- or 11-bit planes: exact; the sum of 32 is exact to ~1e-16)
                        for (int k = k0; k < k1; ++k) s += (double)wr[k] * (double)xr[k];
                        acc[prod[t][2]] = (float)((double)acc[prod[t][2]] + s);  // one rounding per 32-deep product sum
                    }
                }
                out[r][i] = mode == 1 ? std::fma(acc[1], 1.0f / 2048.0f, acc[0]) : acc[0] + acc[1];
            }
        }
    }

    void forward(const float z[5], float y[6], float J[6][5]) const {
        float cur[6][kNetMaxWidth], nxt[6][kNetMaxWidth];
        const int L = n_layers;
        {  // first layer: value chain from the bias; tangent j of output i is act'(h_i) W0[i][j]
            const int nout = widths[1];
            for (int i = 0; i < nout; ++i) {
                float s = b[0][i];
                for (int k = 0; k < 5; ++k) s = std::fma(W[0][i * 5 + k], z[k], s);
                const float h = act[0] ? tanh_k(s) : s, sp = act[0] ? std::fma(-h, h, 1.0f) : 1.0f;
                cur[0][i] = h;
                for (int j = 0; j < 5; ++j) cur[1 + j][i] = sp * W[0][i * 5 + j];
            }
        }
        for (int l = 1; l < L - 1; ++l) {
            hidden(l, cur, nxt);
            const int nout = widths[l + 1];
            for (int i = 0; i < nout; ++i) {
                const float h = act[l] ? tanh_k(nxt[0][i]) : nxt[0][i], sp = act[l] ? std::fma(-h, h, 1.0f) : 1.0f;
                cur[0][i] = h;
                for (int j = 0; j < 5; ++j) cur[1 + j][i] = sp * nxt[1 + j][i];
            }
        }
        const int nin = widths[L - 1];
        for (int o = 0; o < 6; ++o) {  // last layer: fp32 chains
            float s = b[L - 1][o];
            for (int k = 0; k < nin; ++k) s = std::fma(W[L - 1][(long)o * nin + k], cur[0][k], s);
            const float h = act[L - 1] ? tanh_k(s) : s, sp = act[L - 1] ? std::fma(-h, h, 1.0f) : 1.0f;
            y[o] = h;
            for (int j = 0; j < 5; ++j) {
                float t = 0.f;
                for (int k = 0; k < nin; ++k) t = std::fma(W[L - 1][(long)o * nin + k], cur[1 + j][k], t);
                J[o][j] = sp * t;
            }
        }
    }
};

struct HostNnCoeffs {
    static constexpr int kModel = AC_MODEL_NN;
    const HostNet& net;
    float y[6], J[6][5];
    // the four lane groups of a unit evaluate the net at the same four stage inputs: the results are kept by input
    struct Kept { float z[5], y[6], J[6][5]; } kept[4];
    int n_kept = 0;
    explicit HostNnCoeffs(const HostNet& n) : net(n) {}

    template <class T> void prefetch(const DevParams& P, const T x[13], const float uv[7]) {
        float xf[13];
        for (int i = 0; i < 13; ++i) xf[i] = value_of(x[i]);
        AeroPre<float> a;
        aero_pre(P, xf, a);
        const float in[5] = {a.qbar, a.alpha, a.beta, uv[0], uv[1]};
        float z[5];
        for (int j = 0; j < 5; ++j) z[j] = (in[j] - P.mlp_in_mean[j]) / P.mlp_in_std[j];
        for (int e = 0; e < n_kept; ++e)
            if (!std::memcmp(kept[e].z, z, sizeof z)) {
                std::memcpy(y, kept[e].y, sizeof y);
                std::memcpy(J, kept[e].J, sizeof J);
                return;
            }
        net.forward(z, y, J);
        if (n_kept < 4) {
            Kept& k = kept[n_kept++];
            std::memcpy(k.z, z, sizeof z);
            std::memcpy(k.y, y, sizeof y);
            std::memcpy(k.J, J, sizeof J);
        }
    }
    void operator()(const DevParams& P, const AeroPre<float>&, const float*, const float u[7], float C[6]) const {
        for (int k = 0; k < 6; ++k) C[k] = std::fma(y[k], P.mlp_out_std[k], P.mlp_out_mean[k]);
        C[5] += (-0.1f * 6.0f * kDeg) * u[2];
    }
    template <int N>
    void operator()(const DevParams& P, const AeroPre<Dual<N>>& a, const Dual<N>*, const Dual<N> u[7], Dual<N> C[6]) const {
        const Dual<N> in[5] = {a.qbar, a.alpha, a.beta, u[0], u[1]};
        for (int k = 0; k < 6; ++k) {
            C[k].v = std::fma(y[k], P.mlp_out_std[k], P.mlp_out_mean[k]);
            for (int i = 0; i < N; ++i) {
                float s = 0.f;
                for (int j = 0; j < 5; ++j) s = std::fma(J[k][j] * P.mlp_jscale[k][j], in[j].d[i], s);
                C[k].d[i] = s;
            }
        }
        const float kr = -0.1f * 6.0f * kDeg;
        C[5].v += kr * u[2].v;
        for (int i = 0; i < N; ++i) C[5].d[i] += kr * u[2].d[i];
    }
};

}  // namespace

// One RK4 step with A, B, c through HostNnCoeffs, four directions per lane group as k_nn_step_sens splits them.  W[l]:
// [widths[l + 1]][widths[l]] row-major; act[l] = 1: tanh after layer l; mode / drop: above.  dt_per_unit: NULL or [n].
// Arrays component-major as host_dyn_sens'.  Sub-steps must be 1.
extern "C" int host_nn_sens(const ac_params* p, int n_layers, const int* widths, const int* act, const float* const* W,
                            const float* const* b, const float* in_mean, const float* in_std, const float* out_mean,
                            const float* out_std, int mode, int drop, const float* X, const float* U, float dt,
                            const float* dt_per_unit, long n, float* Xn, float* A, float* B, float* c) {
    if (n_layers < 2 || n_layers > kNetMaxLayers || widths[0] != 5 || widths[n_layers] != 6 || mode < 0 || mode > 2) return -2;
    for (int l = 1; l < n_layers; ++l) if (widths[l] < 1 || widths[l] > kNetMaxWidth) return -2;
    if (p->substeps > 1 || p->model_kind != AC_MODEL_NN) return -1;
    DevParams P{};
    P.p = *p;
    for (int j = 0; j < 5; ++j) { P.mlp_in_mean[j] = in_mean[j]; P.mlp_in_std[j] = in_std[j]; }
    for (int k = 0; k < 6; ++k) {
        P.mlp_out_mean[k] = out_mean[k]; P.mlp_out_std[k] = out_std[k];
        for (int j = 0; j < 5; ++j) P.mlp_jscale[k][j] = out_std[k] / in_std[j];
    }
    HostNet net{};
    net.n_layers = n_layers; net.mode = mode; net.drop = drop;
    for (int l = 0; l <= n_layers; ++l) net.widths[l] = widths[l];
    for (int l = 0; l < n_layers; ++l) { net.act[l] = act[l]; net.W[l] = W[l]; net.b[l] = b[l]; net.wp[l] = nullptr; }
    if (mode != 0)
        for (int l = 1; l < n_layers - 1; ++l) {
            const long cnt = (long)widths[l] * widths[l + 1];
            net.wp[l] = new float[3 * cnt];
            for (long i = 0; i < cnt; ++i) {
                float pl[3] = {0.f, 0.f, 0.f};
                split_planes(mode, W[l][i], pl);
                for (int q = 0; q < 3; ++q) net.wp[l][q * cnt + i] = pl[q];
            }
        }
    for (long u = 0; u < n; ++u) {
        float xv[13], uv[7], xn[13], a[169], bb[91], cc[13] = {0};
        for (int i = 0; i < 13; ++i) xv[i] = X[i * n + u];
        for (int i = 0; i < 7; ++i) uv[i] = U[i * n + u];
        HostNnCoeffs coeffs(net);
        unit_step_sens_with<4>(P, coeffs, xv, uv, dt_per_unit ? dt_per_unit[u] : dt, xn, a, bb, cc);
        for (int i = 0; i < 13; ++i) Xn[i * n + u] = xn[i];
        for (int i = 0; i < 169; ++i) A[i * n + u] = a[i];
        for (int i = 0; i < 91; ++i) B[i * n + u] = bb[i];
        if (c) for (int i = 0; i < 13; ++i) c[i * n + u] = cc[i];
    }
    for (int l = 0; l < n_layers; ++l) delete[] net.wp[l];
    return 0;
}

// the plane roundings above on their own (kind 1: f16, 2: bf16), so that the CPU test can hold them to NumPy's conversions
extern "C" void host_plane_round(int kind, const float* x, long n, float* out) {
    for (long i = 0; i < n; ++i) out[i] = kind == 1 ? round_f16(x[i]) : round_bf16(x[i]);
}
