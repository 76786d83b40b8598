// mppi_host.cpp — the MPPI per-unit code (aircraft_amd/csrc/ac_mppi.hpp: Philox, Box-Muller, the sample of one column, the
// weight of one cost) compiled for the HOST (g++, -DAC_HOST_CHECK) behind a small C API, so that `pytest -m "not gpu"` checks
// it against the NumPy restatement (tests/mppi_ref.py) without a GPU.
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include "../../aircraft_amd/csrc/ac_mppi.hpp"

using namespace ac;

// words [4][n] of Philox4x32-10 at counters c [4][n], keys k [2][n]
extern "C" int host_philox(long n, const unsigned* c, const unsigned* k, unsigned* out) {
    for (long i = 0; i < n; ++i) {
        const Philox4 p = philox4x32_10(c[i], c[n + i], c[2 * n + i], c[3 * n + i], k[i], k[n + i]);
        for (int j = 0; j < 4; ++j) out[j * n + i] = p.x[j];
    }
    return 0;
}

// the two normals of every word pair
extern "C" int host_box_muller(long n, const unsigned* xa, const unsigned* xb, float* na, float* nb) {
    for (long i = 0; i < n; ++i) mppi_box_muller(xa[i], xb[i], na[i], nb[i]);
    return 0;
}

// Unom [H][7][B] -> Uc [H][7][K*B], column k*B + b, as k_mppi_sample forms it
extern "C" int host_mppi_sample(const ac_mppi_opts* o, unsigned it, const float* Unom, int K, long B, long H, float* Uc) {
    const long N = (long)K * B;
    for (long t = 0; t < H; ++t)
        for (long k = 0; k < K; ++k)
            for (long b = 0; b < B; ++b) {
                float unom[7], out[7];
                for (int r = 0; r < 7; ++r) unom[r] = Unom[(t * 7 + r) * B + b];
                mppi_sample_column(*o, (unsigned)k, o->instance_offset + (unsigned)b, (unsigned)t, it, o->keep_nominal && k == 0,
                                   unom, out);
                for (int r = 0; r < 7; ++r) Uc[(t * 7 + r) * N + k * B + b] = out[r];
            }
    return 0;
}

// unnormalised weights of n costs against Jmin; fin [n] = 1 where the cost may win
extern "C" int host_mppi_weight(long n, const float* J, float Jmin, float lambda, float* w, int* fin) {
    for (long i = 0; i < n; ++i) {
        w[i] = mppi_weight(J[i], Jmin, lambda);
        fin[i] = mppi_finite(J[i]) ? 1 : 0;
    }
    return 0;
}

extern "C" int host_mppi_better(float Ja, int ka, float Jb, int kb) { return mppi_better(Ja, ka, Jb, kb) ? 1 : 0; }
