// N3: the coordinate rule of the affine crop (OpenCV's WarpAffineInvoker, restated in preprocess.hip's head comment) as __host__
// __device__ code, written once: warp_affine_u8_kernel and the crop-aware JPEG route (jpeg_batch.hip) sample with it on the device, and
// capf_jpeg_crop_rect asks it on the host which source pixels a crop can read -- as jpeg_sync.h shares the entropy rules.
//
// Every floating-point step is a single rounded operation (contraction off), so the build host and the device compute the same integers.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace capf {

struct WarpMap { double a00, a01, a10, a11, b0, b1; };     // the inverse map, in double

__host__ __device__ inline long warp_rn(double v) {         // rint, half to even
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn(v);
#else
    return llrint(v);
#endif
}

__host__ __device__ inline WarpMap warp_inverse(const double* m) {
#pragma clang fp contract(off)
    double d = m[0] * m[4] - m[1] * m[3];
    d = d != 0.0 ? 1.0 / d : 0.0;
    WarpMap w;
    w.a00 = m[4] * d; w.a11 = m[0] * d; w.a01 = m[1] * -d; w.a10 = m[3] * -d;
    w.b0 = -w.a00 * m[2] - w.a01 * m[5];
    w.b1 = -w.a10 * m[2] - w.a11 * m[5];
    return w;
}

// the two addends of a source coordinate in 1/1024 pixel: column x contributes dx (adelta / bdelta), row y contributes X0 / Y0.  Each is
// monotonic in its argument, so the extremes of their sum over an output rectangle lie at its corners.
__host__ __device__ inline void warp_col(const WarpMap& w, int x, long& ax, long& ay) {
#pragma clang fp contract(off)
    ax = warp_rn(w.a00 * (double)x * 1024.0);
    ay = warp_rn(w.a10 * (double)x * 1024.0);
}
__host__ __device__ inline void warp_row(const WarpMap& w, int y, long& X0, long& Y0) {
#pragma clang fp contract(off)
    X0 = warp_rn((w.a01 * (double)y + w.b0) * 1024.0) + 16;
    Y0 = warp_rn((w.a11 * (double)y + w.b1) * 1024.0) + 16;
}

__host__ __device__ inline long warp_clamp16(long v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// output pixel (x, y) -> first tap (sx, sy) and the 5-bit fractions; the taps are (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1)
__host__ __device__ inline void warp_source(const WarpMap& w, int x, int y, long& sx, long& sy, int& fx, int& fy) {
    long ax, ay, X0, Y0;
    warp_col(w, x, ax, ay);
    warp_row(w, y, X0, Y0);
    const long X = (X0 + ax) >> 5, Y = (Y0 + ay) >> 5;
    sx = warp_clamp16(X >> 5);
    sy = warp_clamp16(Y >> 5);
    fx = (int)(X & 31); fy = (int)(Y & 31);
}

// Smallest source rectangle [x0, x1) x [y0, y1) holding every tap of an out_w x out_h crop of a W x H image, clamped to the image.  The
// first tap of each axis is evaluated at the four output corners (exact extremes, see warp_col / warp_row); taps lie at it and at + 1.
// Returns false, and an all-zero rectangle, when no tap falls inside the image (the crop is all border).
__host__ __device__ inline bool warp_source_rect(int W, int H, const double* m, int out_w, int out_h, int rect[4]) {
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (W <= 0 || H <= 0 || out_w <= 0 || out_h <= 0) return false;
    const WarpMap w = warp_inverse(m);
    long lox = 0, hix = 0, loy = 0, hiy = 0;
    for (int c = 0; c < 4; ++c) {
        long sx, sy;
        int fx, fy;
        warp_source(w, (c & 1) ? out_w - 1 : 0, (c & 2) ? out_h - 1 : 0, sx, sy, fx, fy);
        if (c == 0 || sx < lox) lox = sx;
        if (c == 0 || sx > hix) hix = sx;
        if (c == 0 || sy < loy) loy = sy;
        if (c == 0 || sy > hiy) hiy = sy;
    }
    const long x0 = lox < 0 ? 0 : lox, x1 = hix + 2 > W ? W : hix + 2;
    const long y0 = loy < 0 ? 0 : loy, y1 = hiy + 2 > H ? H : hiy + 2;
    if (x0 >= x1 || y0 >= y1) return false;
    rect[0] = (int)x0; rect[1] = (int)y0; rect[2] = (int)x1; rect[3] = (int)y1;
    return true;
}

// Widens a pixel rectangle to whole MCUs (8 hs x 8 vs pixels), after one more pixel on every side along which the chroma is subsampled:
// the h2v1 / h2v2 triangle filters (jpeg.h jpeg_chroma) read the chroma sample next to the pixel's own -- left of an even column, right
// of an odd one, likewise for rows under h2v2 -- and replicate only at the true image edge.  The neighbouring sample covers the pixel
// next to the rectangle, so one pixel of margin reaches exactly the MCUs the filter reads.  mcu = [mx0, my0, mx1, my1), MCU units.
// Chroma narrower than three samples is replicated, not filtered (jpeg_chroma, downsampled_width <= 2), and reads no neighbour; the
// margin is kept there all the same -- such an image is one MCU wide, and a margin that is too large only keeps an MCU it need not.
__host__ __device__ inline void warp_mcu_rect(int W, int H, int hs, int vs, const int rect[4], int mcu[4]) {
    mcu[0] = mcu[1] = mcu[2] = mcu[3] = 0;
    if (rect[0] >= rect[2] || rect[1] >= rect[3]) return;
    const int mw = 8 * hs, mh = 8 * vs;
    const int x0 = rect[0] - (hs == 2), x1 = rect[2] + (hs == 2), y0 = rect[1] - (vs == 2), y1 = rect[3] + (vs == 2);
    mcu[0] = (x0 < 0 ? 0 : x0) / mw;
    mcu[1] = (y0 < 0 ? 0 : y0) / mh;
    mcu[2] = ((x1 > W ? W : x1) + mw - 1) / mw;
    mcu[3] = ((y1 > H ? H : y1) + mh - 1) / mh;
}

// One output pixel of cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) for 8-bit BGR: 15-bit weights from the 5-bit fractions, taps outside
// the H x W image count as 0.  PATCH: `src` holds only the image's pixels [rect[0], rect[2]) x [rect[1], rect[3]) (row pitch `pitch`); the
// border is still the image's, and a tap outside the patch -- none, when rect comes from warp_source_rect -- is never dereferenced.
template <bool PATCH>
__device__ __forceinline__ void warp_affine_pixel(const unsigned char* __restrict__ src, int H, int W, long pitch, const int* rect, const WarpMap& w,
                                                  int x, int y, unsigned char* __restrict__ o) {
    long sx, sy;
    int ax, ay;
    warp_source(w, x, y, sx, sy, ax, ay);
    const int w00 = (32 - ay) * (32 - ax) * 32, w01 = (32 - ay) * ax * 32, w10 = ay * (32 - ax) * 32, w11 = ay * ax * 32;
    bool y0ok = sy >= 0 && sy < H, y1ok = sy + 1 >= 0 && sy + 1 < H;
    bool x0ok = sx >= 0 && sx < W, x1ok = sx + 1 >= 0 && sx + 1 < W;
    if (PATCH) {
        y0ok = y0ok && sy >= rect[1] && sy < rect[3]; y1ok = y1ok && sy + 1 >= rect[1] && sy + 1 < rect[3];
        x0ok = x0ok && sx >= rect[0] && sx < rect[2]; x1ok = x1ok && sx + 1 >= rect[0] && sx + 1 < rect[2];
        sx -= rect[0]; sy -= rect[1];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int acc = 16384;
        if (y0ok && x0ok) acc += w00 * src[sy * pitch + sx * 3 + c];
        if (y0ok && x1ok) acc += w01 * src[sy * pitch + (sx + 1) * 3 + c];
        if (y1ok && x0ok) acc += w10 * src[(sy + 1) * pitch + sx * 3 + c];
        if (y1ok && x1ok) acc += w11 * src[(sy + 1) * pitch + (sx + 1) * 3 + c];
        o[c] = (unsigned char)(acc >> 15);
    }
}

}  // namespace capf
