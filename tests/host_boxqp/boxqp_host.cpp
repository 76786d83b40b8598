// Stand-alone host program for the box-QP routine of the control-limited Riccati pass (aircraft_amd/csrc/ac_boxqp.hpp compiled as
// plain C++ with -DAC_HOST_CHECK).  Reads problems from the file named on the command line — a count n, then per problem 49
// floats of Q (row-major), 7 of q, 7 of lo, 7 of hi, all as text — solves each in fp32 and prints one line per problem:
//   x[0..6] (%.9g)  act[0..6]  iterations  capped
// tests/test_host_box.py builds it with -fsanitize=address,undefined and compares the lines with tests/box_ddp_ref.py.
#include <cstdio>
#include <vector>

#include "../../aircraft_amd/csrc/ac_boxqp.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s problems.txt\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    long n = 0;
    if (std::fscanf(f, "%ld", &n) != 1 || n < 0) { std::fprintf(stderr, "bad count\n"); return 2; }
    std::vector<float> buf(70);
    for (long p = 0; p < n; ++p) {
        for (int i = 0; i < 70; ++i)
            if (std::fscanf(f, "%f", &buf[i]) != 1) { std::fprintf(stderr, "problem %ld: short read\n", p); return 2; }
        float Q[7][7], q[7], lo[7], hi[7];
        for (int i = 0; i < 7; ++i) {
            for (int m = 0; m < 7; ++m) Q[i][m] = buf[i * 7 + m];
            q[i] = buf[49 + i]; lo[i] = buf[56 + i]; hi[i] = buf[63 + i];
        }
        ac::BoxQp r;
        ac::boxqp7(Q, q, lo, hi, r);
        for (int i = 0; i < 7; ++i) std::printf("%.9g ", (double)r.x[i]);
        for (int i = 0; i < 7; ++i) std::printf("%d ", r.act(i));
        std::printf("%d %d\n", r.iters, r.capped);
    }
    std::fclose(f);
    return 0;
}
