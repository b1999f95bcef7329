"""Seeded inputs of the map-gradient fixtures (tests/golden/feature_grads.npz, tools/make_feature_grad_golden.py, test_features_api.py):
HRNet-32 context maps at a 128 x 96 crop, regenerated from seeds like every other golden's inputs."""
import torch

from capf import synth

GOLDEN = {"backbone": "hrnet_32", "B": 2, "H": 128, "W": 96, "wseed": 41, "iseed": 42}
HRNET32_128x96 = [(32, 32, 24), (64, 16, 12), (128, 8, 6), (256, 4, 3)]      # (C_l, H_l, W_l)


def synth_maps(B, geometry, seed):
    """Four NCHW fp32 maps ~ N(0, 1): [B, C_l, H_l, W_l]."""
    return [torch.from_numpy(synth._normal(seed, f"feat{l}/{B}x{c}x{h}x{w}", (B, c, h, w), 1.0)) for l, (c, h, w) in enumerate(geometry)]


def golden_inputs(case=GOLDEN):
    """(maps NCHW fp32, k2d, ref = the crop keypoints normalised as conpose.py:34-35 does, gt) of the fixture."""
    _, k2d, kc, gt = synth.synth_inputs(case["B"], case["H"], case["W"], seed=case["iseed"], crop_range=(192, 256), with_gt=True)
    ref = kc.clone()
    ref[..., 0] = ref[..., 0] / 96.0 - 1.0
    ref[..., 1] = ref[..., 1] / 128.0 - 1.0
    return synth_maps(case["B"], HRNET32_128x96, case["iseed"]), k2d, ref, gt
