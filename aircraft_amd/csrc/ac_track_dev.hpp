// ac_track_dev.hpp — the track as the kernels of ac_track.hpp take it, on its own so that the handle (ac_abi.hpp) holds one
// without those kernels behind it.
#pragma once

namespace ac {

struct TrackDev {
    const float* __restrict__ coef;  // [nseg][3][4]
    const float* __restrict__ knot_exact;  // [nseg + 1]: 1 where the knot's float64 value is an fp32 number
    int nseg;
    float inv_length;   // 1 / track.length()
    float end_pos[3];   // track.eval(1.0), the terminal-alignment target (moving_horizon.py:91)
};

}  // namespace ac
