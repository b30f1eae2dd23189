// tools/libmr_shim.cpp -- a C interface of our own over the reference's libMR, for tools/pin_openmax.py only.
// The pin tool compiles it together with the reference's MetaRecognition.cpp and weibull.c (read from the reference tree,
// never copied) into oracle/_ref/libmr_shim.so, which stays out of git; tests read only tests/golden/openmax.npz.
#include "MetaRecognition.h"

namespace {
struct Fit : MetaRecognition {
    Fit() : MetaRecognition(0, 9, false, 5.0, 10000) {}     // the defaults of libmr.pyx's MR()
    double scale() const { return parmhat[0]; }
    double shape() const { return parmhat[1]; }
};
}  // namespace

extern "C" {
void* mr_new() { return new Fit(); }
void mr_free(void* p) { delete static_cast<Fit*>(p); }
int mr_fit_high(void* p, const double* data, int n, int fit_size) {
    double* copy = new double[n];
    for (int i = 0; i < n; ++i) copy[i] = data[i];
    const int rc = static_cast<Fit*>(p)->FitHigh(copy, n, fit_size);
    delete[] copy;
    return rc;
}
double mr_w_score(void* p, double x) { return static_cast<Fit*>(p)->W_score(x); }
double mr_small_score(void* p) { return static_cast<Fit*>(p)->get_small_score(); }
int mr_valid(void* p) { return static_cast<Fit*>(p)->is_valid() ? 1 : 0; }
double mr_scale(void* p) { return static_cast<Fit*>(p)->scale(); }
double mr_shape(void* p) { return static_cast<Fit*>(p)->shape(); }
}
