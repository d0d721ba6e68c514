// The pixel front end's host arithmetic, with no runtime call in it: Pillow's bicubic tap tables for the resampler behind mmd_preprocess_frames / mmd_vit_encode_frames,
// OpenCV's 8-bit INTER_LINEAR tap table and the letterbox geometry behind mmd_letterbox_frames, and the exact-2x decision of that resize.  model.hip uploads what these
// return, caches it and launches; tests/pixel_taps_shim.cpp asks them without a GPU (tests/test_pixel_taps_host.py).  Every double, cast and order of operations below is
// the library's own (Pillow src/libImaging/Resample.c, OpenCV imgproc/resize.cpp, the reference's test/datasets.py): a bit of difference here is a pixel of difference there.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// Pillow's bicubic tap tables (src/libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc)
static inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
// coef [out_size][ksize] int32 taps at 2^22 scale (zero beyond a row's count), bounds [out_size][2] = {first source index, tap count}
static inline void pil_coeffs(int in_size, int out_size, std::vector<int32_t>& coef, std::vector<int32_t>& bounds, int& ksize) {
    double scale = (double)in_size / out_size, filterscale = scale < 1.0 ? 1.0 : scale;
    double support = 2.0 * filterscale;
    ksize = (int)ceil(support) * 2 + 1;
    coef.assign((size_t)out_size * ksize, 0); bounds.assign((size_t)out_size * 2, 0);
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        double center = (xx + 0.5) * scale, ww = 0.0, ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5); if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5); if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < ksize; ++x) k[x] = 0.0;
        for (int x = 0; x < xmax; ++x) { double w = bicubic_filter((x + xmin - center + 0.5) * ss); k[x] = w; ww += w; }
        for (int x = 0; x < xmax; ++x) if (ww != 0.0) k[x] /= ww;
        for (int x = 0; x < ksize; ++x) coef[(size_t)xx * ksize + x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << 22)) : (int32_t)(0.5 + k[x] * (1 << 22));
        bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
    }
}

// OpenCV's 8-bit INTER_LINEAR tap table for one axis (imgproc/resize.cpp, resize() -> ResizeLinear setup):
//   f = (float)((d + 0.5) * scale - 0.5); s = floor(f); f -= s; weights = saturate_cast<short>(w * 2048) (round half to even).
// The x axis clamps the tap pair at the borders (s < 0 -> s = 0, f = 0; s >= n-1 -> s = n-1, f = 0); the y axis keeps f and
// clips the two row indices instead.  Entry: {s0, s1, w0, w1}.
static inline void cv_linear_taps(int src_n, int dst_n, bool x_axis, std::vector<int32_t>& tab) {
    const double inv_scale = (double)dst_n / src_n, scale = 1.0 / inv_scale;
    tab.resize((size_t)dst_n * 4);
    for (int d = 0; d < dst_n; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        int s0, s1;
        if (x_axis) {
            if (s < 0) { f = 0.f; s = 0; }
            if (s >= src_n - 1) { f = 0.f; s = src_n - 1; }
            s0 = s; s1 = s + 1 < src_n ? s + 1 : src_n - 1;
        } else {
            s0 = s < 0 ? 0 : (s < src_n ? s : src_n - 1);
            s1 = s + 1 < 0 ? 0 : (s + 1 < src_n ? s + 1 : src_n - 1);
        }
        const float w0 = (1.f - f) * 2048.f, w1 = f * 2048.f;
        long r0 = lrintf(w0), r1 = lrintf(w1);
        r0 = r0 < -32768 ? -32768 : (r0 > 32767 ? 32767 : r0); r1 = r1 < -32768 ? -32768 : (r1 > 32767 ? 32767 : r1);
        tab[4 * d] = s0; tab[4 * d + 1] = s1; tab[4 * d + 2] = (int32_t)r0; tab[4 * d + 3] = (int32_t)r1;
    }
}

// the resize target and pad widths of the reference's load_video (test/datasets.py:53-60, :63-68) for a W x H frame at resolution R (all > 0)
struct LetterboxGeom { int new_w, new_h, top, bottom, left, right; };
static inline LetterboxGeom letterbox_geom(int W, int H, int R) {
    LetterboxGeom g;
    if (W > H) { g.new_w = R; g.new_h = (int)(((double)H / (double)W) * R); }
    else { g.new_h = R; g.new_w = (int)(((double)W / (double)H) * R); }
    g.top = (R - g.new_h) / 2; g.bottom = (R - g.new_h + 1) / 2;
    g.left = (R - g.new_w) / 2; g.right = (R - g.new_w + 1) / 2;
    return g;
}
// resize.cpp: INTER_LINEAR with both scales exactly 2 is routed to the 2x2 INTER_AREA kernel (new_w, new_h > 0)
static inline int letterbox_area2x(int W, int H, int new_w, int new_h) {
    const double sx = 1.0 / ((double)new_w / W), sy = 1.0 / ((double)new_h / H);
    return (fabs(sx - 2.0) < DBL_EPSILON && fabs(sy - 2.0) < DBL_EPSILON) ? 1 : 0;
}
