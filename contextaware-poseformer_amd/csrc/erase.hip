// Joint-centred occlusion of uint8 crops: erase_image of ContextPose/mvn/utils/img.py:179-198 for a whole batch, between
// the crop (capf_jpeg_decode_crop_batch / capf_warp_affine) and the normalisation (capf_preprocess / capf_forward_u8).  Per frame b:
//   erase_image(images[b], [centers[b, p] for p ascending if mask is NULL or mask[b, p] != 0], size, use_mean)
// Two launches, no atomics, no allocation, no host synchronisation:
//   erase_patch_kernel  one block per (frame, patch): judges the centre, writes the patch's rectangle and -- use_mean -- the per-channel integer
//                       mean of the ORIGINAL image over it into the caller's scratch (one 32-byte record per patch);
//   erase_paint_kernel  every pixel scans its frame's records from the last patch to the first and takes the first that covers it (the
//                       reference paints in ascending order, so the highest p wins), else its own value; a thread first keeps, as a bit
//                       mask, the patches that can touch its 16 bytes at all -- none, for most of a crop.  A thread reads and writes the same
//                       bytes and the means are final before this launch starts, so out == images gives the same bits as out of place.
// The rule, all of it in integers: a centre (x, y) counts iff -1 < x < W and -1 < y < H on the floats -- the reference's int() truncation toward
// zero followed by its range test (-0.5 -> 0 counts, -1.0 does not, W - 0.25 counts); false for NaN and +-Inf, and a float is converted to int only
// after it passed.  xc = (int)x, left = max(0, xc - size / 2), right = min(W, xc + size / 2 + 1), rows likewise.  The mean is sum / count in
// integers: what numpy stores when the float64 mean of uint8 values goes into a uint8 array (the quotient is exact in float64 unless it is
// no integer, and then it is at least 1 / count away from one).
#include "kernels.h"

namespace capf {

// one patch of one frame as the paint kernel reads it: x1 == 0 marks a patch that does not count (a counting one has x1 >= 1)
struct alignas(16) ErasePatch {
    int x0, x1, y0, y1;
    unsigned value;          // channel c of the patch in bits [8c, 8c + 8), memory order
    int pad0, pad1, pad2;
};
static_assert(sizeof(ErasePatch) == ERASE_PATCH_BYTES, "capf_erase_scratch_bytes counts 32 bytes per patch");

__global__ __launch_bounds__(256) void erase_patch_kernel(const unsigned char* __restrict__ images, const float* __restrict__ centers,
                                                          const unsigned char* __restrict__ mask, int H, int W, int P, int size,
                                                          int use_mean, ErasePatch* __restrict__ patches) {
    const long bp = blockIdx.x;                        // frame * P + patch
    const long b = bp / P;
    const float x = centers[bp * 2], y = centers[bp * 2 + 1];
    const bool counts = (!mask || mask[bp] != 0) && x > -1.0f && (double)x < (double)W && y > -1.0f && (double)y < (double)H;
    ErasePatch rec{};
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    if (counts) {                                      // block-uniform
        const int xc = (int)x, yc = (int)y, half = size / 2;
        rec.x0 = xc - half > 0 ? xc - half : 0;
        rec.y0 = yc - half > 0 ? yc - half : 0;
        rec.x1 = (int)((long)xc + half + 1 < W ? (long)xc + half + 1 : W);
        rec.y1 = (int)((long)yc + half + 1 < H ? (long)yc + half + 1 : H);
        if (use_mean) {
            const int pw = rec.x1 - rec.x0, n = pw * (rec.y1 - rec.y0);          // (a frame's bytes fit an int: the launcher's rule)
            const unsigned char* img = images + b * H * W * 3;
            for (int i = threadIdx.x; i < n; i += 256) {
                const int r = i / pw, c = i - r * pw;
                const unsigned char* px = img + ((long)(rec.y0 + r) * W + rec.x0 + c) * 3;
                s0 += px[0]; s1 += px[1]; s2 += px[2];
            }
        }
    }
    if (!counts || !use_mean) {                        // nothing to sum: the record alone
        if (threadIdx.x == 0) patches[bp] = rec;
        return;
    }
    // integer sums: lanes of a wave by shuffle, the four waves through LDS, always in this order
    for (int d = 32; d > 0; d >>= 1) {
        s0 += __shfl_down(s0, d, 64); s1 += __shfl_down(s1, d, 64); s2 += __shfl_down(s2, d, 64);
    }
    __shared__ unsigned long long part[4][3];
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = s0; part[threadIdx.x >> 6][1] = s1; part[threadIdx.x >> 6][2] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long n = (unsigned long long)(rec.x1 - rec.x0) * (unsigned long long)(rec.y1 - rec.y0);
        for (int c = 0; c < 3; ++c) rec.value |= (unsigned)((part[0][c] + part[1][c] + part[2][c] + part[3][c]) / n) << (8 * c);
        patches[bp] = rec;
    }
}

// the patches of a frame that may cover a pixel of the run (xa, ya) .. (xb, yb) of consecutive pixels, one bit each: exact for a run inside one
// row, by rows alone for a run that wraps (a patch that does not count holds zeros and never passes)
__device__ __forceinline__ unsigned erase_candidates(const ErasePatch* rec, int P, int xa, int ya, int xb, int yb) {
    unsigned cand = 0;
    for (int p = 0; p < P; ++p) {
        const ErasePatch r = rec[p];              // (one address for the whole wave: an LDS broadcast)
        const bool rows = ya < r.y1 && yb >= r.y0, cols = ya != yb || (xa < r.x1 && xb >= r.x0);
        cand |= (unsigned)(rows && cols) << p;
    }
    return cand;
}

// the last counting patch among `cand` that covers pixel (x, y), or -1
__device__ __forceinline__ int erase_hit(const ErasePatch* rec, unsigned cand, int x, int y) {
    while (cand) {
        const int p = 31 - __clz((int)cand);
        if (x >= rec[p].x0 && x < rec[p].x1 && y >= rec[p].y0 && y < rec[p].y1) return p;
        cand &= ~(1u << p);
    }
    return -1;
}

// VEC: 16 bytes of a frame per thread (frames start 16-byte aligned in both buffers and hold a multiple of 16 bytes); else a pixel per thread
template <bool VEC>
__global__ __launch_bounds__(256) void erase_paint_kernel(const unsigned char* images, unsigned char* out, int W, int frame_bytes, int P,
                                                          const ErasePatch* __restrict__ patches, int blocks_per_frame) {
    const int b = blockIdx.x / blocks_per_frame;
    const int item = (blockIdx.x - b * blocks_per_frame) * 256 + threadIdx.x;
    __shared__ ErasePatch rec[MAX_JOINTS];
    if (threadIdx.x < P) rec[threadIdx.x] = patches[(long)b * P + threadIdx.x];
    __syncthreads();
    const long base = (long)b * frame_bytes;
    if (VEC) {
        if ((long)item * 16 >= frame_bytes) return;
        const int o = item * 16;
        uint4 v = *reinterpret_cast<const uint4*>(images + base + o);
        unsigned w[4] = {v.x, v.y, v.z, v.w};
        int pix = o / 3, c = o - pix * 3;
        const int last = (o + 15) / 3;
        const unsigned cand = erase_candidates(rec, P, pix % W, pix / W, last % W, last / W);
        int hit = erase_hit(rec, cand, pix % W, pix / W);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (hit >= 0) w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (((rec[hit].value >> (8 * c)) & 0xffu) << (8 * (j & 3)));
            if (++c == 3 && j < 15) {
                c = 0;
                ++pix;
                hit = erase_hit(rec, cand, pix % W, pix / W);
            }
        }
        *reinterpret_cast<uint4*>(out + base + o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        if (item >= frame_bytes / 3) return;
        const unsigned char* s = images + base + (long)item * 3;
        unsigned v = s[0] | (s[1] << 8) | (s[2] << 16);
        const int x = item % W, y = item / W;
        const int hit = erase_hit(rec, erase_candidates(rec, P, x, y, x, y), x, y);
        if (hit >= 0) v = rec[hit].value;
        unsigned char* d = out + base + (long)item * 3;
        d[0] = (unsigned char)v; d[1] = (unsigned char)(v >> 8); d[2] = (unsigned char)(v >> 16);
    }
}

// Every argument was judged by capf_erase_patches (engine.cpp): B * P and the paint grid fit a grid dimension, a frame's bytes fit an int.
hipError_t launch_erase_patches(const unsigned char* images, int B, int H, int W, const float* centers, const unsigned char* mask, int P,
                                int size, int use_mean, unsigned char* out, void* scratch, hipStream_t s) {
    if (B < 1 || H < 1 || W < 1 || P < 1 || P > MAX_JOINTS || size < 0 || (long)H * W * 3 > 0x7fffffffL) return hipErrorInvalidValue;
    ErasePatch* patches = static_cast<ErasePatch*>(scratch);
    const int frame_bytes = H * W * 3;
    const bool vec = frame_bytes % 16 == 0 && ((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const long items = vec ? frame_bytes / 16 : frame_bytes / 3;
    const long per_frame = (items + 255) / 256;
    if ((long)B * P > 0x7fffffffL || per_frame * B > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(erase_patch_kernel, dim3((unsigned)((long)B * P)), dim3(256), 0, s, images, centers, mask, H, W, P, size, use_mean, patches);
    if (vec)
        hipLaunchKernelGGL(erase_paint_kernel<true>, dim3((unsigned)(per_frame * B)), dim3(256), 0, s, images, out, W, frame_bytes, P, patches,
                           (int)per_frame);
    else
        hipLaunchKernelGGL(erase_paint_kernel<false>, dim3((unsigned)(per_frame * B)), dim3(256), 0, s, images, out, W, frame_bytes, P, patches,
                           (int)per_frame);
    return hipGetLastError();
}

}  // namespace capf
