// Host sanitizer check of a handle's life, no GPU needed: creates and destroys plan-only handles of the three backbones, asks each the
// questions a host asks before it has a device (schema, workspace size, op table), makes every run entry refuse it, walks the refusal paths
// of the stand-alone keypoint head entries (capf_kp_head_forward / capf_kp_head_backward / capf_cpn_decode / capf_cpn_decode_pair:
// arguments judged before any launch), and lets capf_create fail both in front of the plan (a refused configuration) and behind it (a device that is not there: the branch that releases what a
// handle already owns).  Built by `make -C contextaware-poseformer_amd/csrc hostcheck`: the engine's host sources with
// -fsanitize=address,undefined, the device objects of the product build; it runs on the build machine and is not loaded into Python.
#include <stdio.h>
#include <string.h>

#include "capf.h"

static capf_config config(int backbone, int width, int dtype, int training) {
    capf_config c;
    memset(&c, 0, sizeof(c));
    c.backbone = backbone;
    for (int i = 0; i < 4; ++i) c.hr_channels[i] = width << i;
    c.hr_modules[0] = 1; c.hr_modules[1] = 4; c.hr_modules[2] = 3;
    c.hr_blocks = 4;
    c.base_dim = backbone == CAPF_CPN50 ? 256 : width;
    c.embed_dim_ratio = 128;
    c.levels = 4; c.num_joints = 17; c.num_heads = 8; c.deform_heads = 4; c.deform_samples = 4; c.context_blocks = 1;
    c.compute_dtype = dtype;
    c.max_batch = 64;
    c.height = 64; c.width = 64;
    c.training = training;
    return c;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    float mem[64] = {0};
    const uint8_t bytes[16] = {0};
    const float* maps[4] = {mem, mem, mem, mem};
    int handles = 0;
    for (int backbone : {CAPF_HRNET, CAPF_CPN50})
        for (int width : {32, 48})
            for (int dtype : {CAPF_F32, CAPF_BF16})
            for (int flags : {0, (int)CAPF_PLAN_BN_BATCH_STATS, (int)CAPF_PLAN_CPN_PREDICT}) {      // (the batch-statistics route's units and unfolded packs
                                                                                                    // next to the plan; CPN's final_predict head behind the cascades)
                if (backbone == CAPF_CPN50 && width == 48) continue;
                if (flags == CAPF_PLAN_BN_BATCH_STATS && (backbone != CAPF_HRNET || dtype != CAPF_F32)) continue;
                if (flags == CAPF_PLAN_CPN_PREDICT && backbone != CAPF_CPN50) {      // refused in front of the plan, by name
                    capf_config r = config(backbone, width, dtype, 1);
                    r.plan_flags = flags;
                    capf_handle* none = nullptr;
                    CHECK(capf_create(&r, -1, &none) == CAPF_ERR_UNSUPPORTED && !none && strstr(capf_last_error(nullptr), "CAPF_PLAN_CPN_PREDICT"));
                    continue;
                }
                capf_config c = config(backbone, width, dtype, 1);
                c.plan_flags = flags;
                capf_handle* h = nullptr;
                CHECK(capf_create(&c, -1, &h) == CAPF_OK && h);
                const int n = capf_num_ops(h);
                CHECK(n > 0 && capf_num_params(h) > 0 && capf_workspace_bytes(h, 2) > 0 && capf_workspace_bytes(h, 0) == 0);
                for (int i = 0; i < n; ++i) {
                    const char *name, *kernel;
                    double flops;
                    CHECK(capf_op_info(h, i, 24, &name, &kernel, &flops) == CAPF_OK);
                }
                CHECK(capf_forward(h, nullptr, mem, mem, mem, 2, mem) == CAPF_ERR_STATE);
                CHECK(capf_backbone_forward(h, nullptr, mem, 2) == CAPF_ERR_STATE);
                CHECK(capf_backbone_forward_bn(h, nullptr, mem, 2, 0.1f) == CAPF_ERR_STATE);
                CHECK(capf_forward_train(h, nullptr, mem, mem, mem, 2, mem, nullptr) == CAPF_ERR_STATE);
                CHECK(capf_forward_u8(h, nullptr, bytes, mem, nullptr, 2, mem, mem, 2, mem) == CAPF_ERR_STATE);
                CHECK(capf_backbone_forward_u8(h, nullptr, bytes, mem, mem, 3, 2) == CAPF_ERR_INVALID);
                CHECK(capf_forward_train_u8(h, nullptr, bytes, nullptr, nullptr, 0, mem, mem, 2, mem, nullptr) == CAPF_ERR_INVALID);
                CHECK(capf_lifter_forward(h, nullptr, mem, mem, 2, mem) == CAPF_ERR_STATE);
                CHECK(capf_lifter_forward_train(h, nullptr, mem, mem, 2, mem, nullptr) == CAPF_ERR_STATE);
                CHECK(capf_set_features(h, nullptr, maps, 2) == (dtype == CAPF_F32 ? CAPF_ERR_STATE : CAPF_ERR_UNSUPPORTED));
                CHECK(capf_forward_prefix(h, nullptr, mem, nullptr, nullptr, 2, nullptr, 1) == CAPF_ERR_STATE);
                CHECK(capf_forward_profile(h, nullptr, mem, mem, mem, 2, mem, mem, n - 1) == CAPF_ERR_INVALID);
                {   // the named tensor of the head exists under its flag alone
                    int64_t shape[4];
                    int nd = 0;
                    const int rc = capf_tensor(h, "heat", nullptr, shape, &nd);
                    CHECK(flags == CAPF_PLAN_CPN_PREDICT ? (rc == (dtype == CAPF_F32 ? 0 : 2) && nd == 4 && shape[1] == 64 && shape[2] == 48 && shape[3] == 20)
                                                         : rc == CAPF_ERR_INVALID);
                }
                CHECK(capf_set_workspace(h, mem, sizeof(mem)) == CAPF_OK && capf_train_generation(h) == 1);
                capf_destroy(h);
                ++handles;
            }
    capf_destroy(nullptr);
    // the stand-alone keypoint head entries judge every argument before a launch: each refusal path, none of which touches a device
    {
        const float dec[4] = {1.f, 0.f, 1.f, 0.f};
        const size_t fwd = capf_kp_head_scratch_bytes(2, 8, 8, 32, 17, 0), bwd = capf_kp_head_scratch_bytes(2, 8, 8, 32, 17, 1);
        CHECK(fwd > 0 && bwd > fwd && capf_kp_head_scratch_bytes(2, 8, 8, 30, 17, 0) == 0 && capf_kp_head_scratch_bytes(2, 8, 8, 32, 33, 1) == 0);
        alignas(16) static float big[4096];
        CHECK(capf_kp_head_forward(nullptr, nullptr, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 0, 1.f, dec, nullptr, mem, nullptr, nullptr, nullptr, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_forward(nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 0, 1.f, dec, nullptr, nullptr, nullptr, nullptr, nullptr, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_forward(nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 33, 0, 1.f, dec, nullptr, mem, nullptr, nullptr, nullptr, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_forward(nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 36, 17, 2, 1.f, dec, nullptr, mem, nullptr, nullptr, nullptr, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_forward(nullptr, big, 3, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, nullptr, nullptr, nullptr, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_forward(nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 0.f, dec, nullptr, mem, nullptr, nullptr, nullptr, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_forward(nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, nullptr, nullptr, nullptr, big, fwd - 1) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_forward(nullptr, big + 1, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, nullptr, nullptr, nullptr, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_backward(nullptr, mem, nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 0, 1.f, dec, nullptr, mem, mem, nullptr, 0, big, sizeof(big)) == CAPF_ERR_UNSUPPORTED);
        CHECK(capf_kp_head_backward(nullptr, mem, nullptr, big, CAPF_BF16, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, mem, nullptr, 0, big, sizeof(big)) == CAPF_ERR_UNSUPPORTED);
        CHECK(capf_kp_head_backward(nullptr, nullptr, nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, mem, nullptr, 0, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_backward(nullptr, nullptr, mem, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, mem, nullptr, 0, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_backward(nullptr, mem, nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, nullptr, mem, nullptr, 0, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_backward(nullptr, mem, nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, mem, big + 1, 1, big, sizeof(big)) == CAPF_ERR_INVALID);
        CHECK(capf_kp_head_backward(nullptr, mem, nullptr, big, CAPF_F32, mem, mem, 2, 8, 8, 32, 17, 1, 1.f, dec, nullptr, mem, mem, nullptr, 0, big, fwd) == CAPF_ERR_INVALID);
    }
    // ... and capf_cpn_decode
    {
        const float dec[4] = {4.f, 2.f, 4.f, 2.f};
        alignas(16) static float big[64];
        double taps[21];
        capf_cpn_decode_taps(taps);
        double sum = 0.0;
        for (int i = 0; i < 21; ++i) { CHECK(taps[i] == taps[20 - i] && taps[i] > 0.0); sum += taps[i]; }
        CHECK(sum > 1.0 - 1e-14 && sum < 1.0 + 1e-14);
        CHECK(capf_cpn_decode_lds_bytes(64, 48) == 256 + 8 * 84 * 68 + 4 * 64 * 48 && capf_cpn_decode_lds_bytes(0, 48) == 0);
        CHECK(capf_cpn_decode(nullptr, nullptr, CAPF_F32, 2, 8, 8, 20, 17, dec, nullptr, mem, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, dec, nullptr, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big, CAPF_F32, 2, 8, 8, 20, 21, dec, nullptr, mem, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big, CAPF_F32, 2, 8, 8, 33, 17, dec, nullptr, mem, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big, CAPF_F32, 2, 0, 8, 20, 17, dec, nullptr, mem, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big + 1, CAPF_F32, 2, 8, 8, 20, 17, dec, nullptr, mem, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big, 3, 2, 8, 8, 20, 17, dec, nullptr, mem, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, dec, nullptr, mem, mem, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode(nullptr, big, CAPF_BF16, 2, 128, 128, 20, 17, dec, nullptr, mem, nullptr, nullptr, nullptr) == CAPF_ERR_UNSUPPORTED);
        // ... and its flip-test pair: the swap table is the one argument that is read (on the host) before any refusal behind it
        const int32_t h36m[17] = {0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13};
        int32_t cycle[17], outside[17];
        for (int j = 0; j < 17; ++j) cycle[j] = outside[j] = j;
        cycle[1] = 2; cycle[2] = 3; cycle[3] = 1;
        outside[16] = 17;
        CHECK(capf_cpn_decode_pair(nullptr, nullptr, CAPF_F32, 2, 8, 8, 20, 17, h36m, dec, nullptr, 192.f, mem, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, nullptr, dec, nullptr, 192.f, mem, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, h36m, dec, nullptr, 192.f, nullptr, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, h36m, dec, nullptr, 192.f, mem, mem, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, cycle, dec, nullptr, 192.f, mem, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, outside, dec, nullptr, 192.f, mem, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_F32, 2, 8, 8, 20, 17, h36m, dec, nullptr, INFINITY, mem, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_INVALID);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_BF16, 2, 128, 128, 20, 17, h36m, dec, nullptr, 192.f, mem, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_UNSUPPORTED);
        CHECK(capf_cpn_decode_pair(nullptr, big, CAPF_F32, 1 << 27, 8, 8, 20, 16, outside, dec, nullptr, 192.f, mem, nullptr, nullptr, nullptr, nullptr) == CAPF_ERR_UNSUPPORTED);
    }
    // refused in front of the plan, inside it, and behind it (no device 0 on a machine without a GPU: what the handle owns is released)
    capf_handle* h = nullptr;
    capf_config c = config(CAPF_HRNET, 32, 7, 0);
    CHECK(capf_create(&c, -1, &h) == CAPF_ERR_UNSUPPORTED && !h);
    c = config(CAPF_HRNET, 32, CAPF_F32, 0);
    c.height = 72;
    CHECK(capf_create(&c, -1, &h) == CAPF_ERR_UNSUPPORTED && !h && strstr(capf_last_error(nullptr), "multiples of 32"));
    c.height = 64;
    const int rc = capf_create(&c, 0, &h);
    if (rc == CAPF_OK) capf_destroy(h);      // (a machine with a GPU: the handle's device resources, allocated and released)
    else CHECK(rc == CAPF_ERR_HIP && !h);
    printf("handle_lifecycle: %d plan-only handles created and destroyed, 2 configurations refused, capf_create(device 0) -> %d\n", handles, rc);
    return 0;
}
