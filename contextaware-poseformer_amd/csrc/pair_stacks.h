// The outputs of a flip-test pair's decode (capf_kp_head_forward_pair, capf_cpn_decode_pair), written by the thread that holds joint j of source
// frame b: both sets of the stacks kcrop2 / k2d2 [2, B, J, 2] and score [B, J].  Set 1 is capf_preprocess_points(mode = 2)'s mirrored set with
// mirror_w in place of its 192 -- x -> (mirror_w - x) - 1 in crop pixels, x -> -x in image coordinates, joint j stored at swap[j] -- and swap
// is a permutation, so every element has one writer.  include/capf.h states the expressions; this is their one implementation.  Contraction
// is off whatever the including file is compiled with: every product and every sum is rounded on its own, so k2d2[0] is the float32
// expression itself and the stacks are capf_preprocess_points' bits.
//   o = b * J + j, om = (B + b) * J + swap[j]: the (frame, joint) elements of set 0 and of the mirrored set (the caller holds them already)
//   A: frame b's crop -> image matrix [2, 3], or NULL: no k2d2 is written
#pragma once
#include <stddef.h>

namespace capf {

__device__ __forceinline__ void write_pair_stacks(float* kcrop2, float* k2d2, float* score_out, const size_t o, const size_t om, const float* A,
                                                  const float mirror_w, const float kx, const float ky, const float score) {
#pragma clang fp contract(off)
    kcrop2[o * 2] = kx;
    kcrop2[o * 2 + 1] = ky;
    if (score_out) score_out[o] = score;
    kcrop2[om * 2] = (mirror_w - kx) - 1.0f;
    kcrop2[om * 2 + 1] = ky;
    if (A) {
        const float ix = (A[0] * kx + A[1] * ky) + A[2], iy = (A[3] * kx + A[4] * ky) + A[5];
        k2d2[o * 2] = ix;
        k2d2[o * 2 + 1] = iy;
        k2d2[om * 2] = -ix;
        k2d2[om * 2 + 1] = iy;
    }
}

}  // namespace capf
