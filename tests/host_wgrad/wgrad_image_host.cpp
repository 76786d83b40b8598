// Host harness of tests/test_wgrad_host.py: build_mlp_model + build_wgrad_image (aircraft_amd/csrc/ac_wgrad.hpp, host part)
// compiled with g++ alone, handed to Python as flat arrays.
#include "../../aircraft_amd/csrc/ac_wgrad.hpp"

extern "C" {
// plan: the WgradPlan as ints; image: caller's buffer of at least `cap` floats.  Returns the image size in floats, or the
// (negative) status of build_mlp_model.
long host_wgrad_image(int n_layers, const int* widths, const int* act, const float* const* W, const float* const* b, int* plan,
                      int* wt, float* image, long cap) {
    ac::MlpModel m;
    char err[256] = "";
    const int rc = ac::build_mlp_model(n_layers, widths, act, W, b, 1, m, err, sizeof(err));
    if (rc != AC_OK) return rc;
    ac::WgradPlan p;
    std::vector<float> img;
    ac::build_wgrad_image(m, p, img);
    std::memcpy(plan, &p, sizeof(p));
    *wt = m.wt;
    if ((long)img.size() > cap) return -100;
    std::memcpy(image, img.data(), img.size() * sizeof(float));
    return (long)img.size();
}
int host_wgrad_plan_ints(void) { return (int)(sizeof(ac::WgradPlan) / sizeof(int)); }
int host_wgrad_lds_bytes(int n_layers, int wt) { return ac::wgrad_lds_bytes(n_layers, wt); }
}
