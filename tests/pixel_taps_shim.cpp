// C entries around the host-only tap tables of the pixel front end (mmduet_amd/csrc/pixel_taps.h) for tests/test_pixel_taps_host.py: built with the host C++ compiler
// alone, never part of the library.
#include "../mmduet_amd/csrc/pixel_taps.h"

// taps per table row for in_size -> out_size (what the caller must leave room for: coef [out_size * ksize], bounds [out_size * 2])
extern "C" int pixel_ksize_shim(int in_size, int out_size) {
    std::vector<int32_t> coef, bounds; int ks = 0;
    pil_coeffs(in_size, out_size, coef, bounds, ks);
    return ks;
}
// -> ksize; coef_room / bounds_room in elements: nothing is written when the tables do not fit (-1)
extern "C" int pil_coeffs_shim(int in_size, int out_size, int* coef, long long coef_room, int* bounds, long long bounds_room) {
    std::vector<int32_t> c, b; int ks = 0;
    pil_coeffs(in_size, out_size, c, b, ks);
    if ((long long)c.size() != (long long)out_size * ks || (long long)b.size() != 2LL * out_size) return -2;
    if ((long long)c.size() > coef_room || (long long)b.size() > bounds_room) return -1;
    for (size_t i = 0; i < c.size(); ++i) coef[i] = c[i];
    for (size_t i = 0; i < b.size(); ++i) bounds[i] = b[i];
    return ks;
}
// tab [dst_n][4] = {s0, s1, w0, w1}
extern "C" int cv_linear_taps_shim(int src_n, int dst_n, int x_axis, int* tab) {
    std::vector<int32_t> t;
    cv_linear_taps(src_n, dst_n, x_axis != 0, t);
    if ((long long)t.size() != 4LL * dst_n) return -2;
    for (size_t i = 0; i < t.size(); ++i) tab[i] = t[i];
    return 0;
}
// out: {new_w, new_h, top, bottom, left, right, area2x (-1 where the frame collapses: mmd_letterbox_frames refuses it before asking)}
extern "C" void letterbox_geom_shim(int W, int H, int R, int* out) {
    const LetterboxGeom g = letterbox_geom(W, H, R);
    out[0] = g.new_w; out[1] = g.new_h; out[2] = g.top; out[3] = g.bottom; out[4] = g.left; out[5] = g.right;
    out[6] = (g.new_w > 0 && g.new_h > 0) ? letterbox_area2x(W, H, g.new_w, g.new_h) : -1;
}
// the same over a whole grid W, H in 1..n at one R, in one call: out [n][n][7], W outermost
extern "C" void letterbox_grid_shim(int n, int R, int* out) {
    for (int W = 1; W <= n; ++W) for (int H = 1; H <= n; ++H) letterbox_geom_shim(W, H, R, out + ((long long)(W - 1) * n + (H - 1)) * 7);
}
