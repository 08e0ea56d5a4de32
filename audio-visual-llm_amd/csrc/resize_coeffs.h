// Pillow's 8-bit BICUBIC resample as csrc/preprocess.hip and csrc/video_augment.hip apply it: the fixed-point constants, the device rounding
// step, and the host recipe of the coefficient tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc, bicubic a = -0.5, support 2), the
// shortest-edge output shape and the rescale / normalise table.  One copy, so the plain and the augmented pass cannot drift apart.
#pragma once
#include <cmath>
#include <vector>

namespace av_resize {

constexpr int PBITS = 32 - 8 - 2;            // Resample.c PRECISION_BITS

__device__ __forceinline__ int clip8(int v) {
    v >>= PBITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

inline double bicubic(double x) {
    const double a = -0.5;
    if (x < 0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
inline int coeff_ksize(int in_size, int out_size) {
    double fs = (double)in_size / out_size;
    if (fs < 1.0) fs = 1.0;
    return (int)std::ceil(2.0 * fs) * 2 + 1;
}
// coefficients of output samples [o0, o0+cnt_out) of an in_size -> out_size resample
inline void coeffs(int in_size, int out_size, int o0, int cnt_out, std::vector<int>& bounds, std::vector<int>& kk, int ksize) {
    const double scale = (double)in_size / out_size;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale, ss = 1.0 / filterscale;
    bounds.assign((size_t)cnt_out * 2, 0);
    kk.assign((size_t)cnt_out * ksize, 0);
    std::vector<double> w(ksize);
    for (int t = 0; t < cnt_out; ++t) {
        const int xx = o0 + t;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) { w[x] = bicubic((x + xmin - center + 0.5) * ss); ww += w[x]; }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            kk[(size_t)t * ksize + x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << PBITS)) : (int)(0.5 + w[x] * (1 << PBITS));
        }
        bounds[2 * t] = xmin; bounds[2 * t + 1] = xmax;
    }
}
inline void resized_shape(int H, int W, int image, int& nh, int& nw) {     // image_transforms.get_resize_output_image_size(shortest_edge)
    if (W <= H) { nw = image; nh = (int)((double)image * H / W); }
    else        { nh = image; nw = (int)((double)image * W / H); }
}
// lut[c][v] = (v / 255 - mean[c]) / std[c] as the PIL backend rounds it
inline void normalize_lut(const float* mean3, const float* std3, float* lut) {
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const float r = (float)((double)v * (1.0 / 255.0));          // image_transforms.rescale: float64 product, then float32
            lut[c * 256 + v] = (r - mean3[c]) / std3[c];                  // image_transforms.normalize in float32
        }
}

}  // namespace av_resize
