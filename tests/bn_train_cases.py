"""The seeded case behind tests/golden/mpi_bn_train_w32_64x64.npz, shared by its recipe (tools/make_bn_train_golden.py) and its test."""
from capf import synth

GOLDEN = {"backbone": "hrnet_32", "wseed": 3, "batch": 2, "height": 64, "width": 64, "steps": 3, "seed": 90}

# running statistics stored whole: the stem, a layer1 bottleneck's last BatchNorm and its projection shortcut's, the last transition, a
# fuse-layer BatchNorm and the last BatchNorm of stage4's last module (names relative to the backbone)
NAMED_LAYERS = ("bn1", "layer1.0.bn3", "layer1.0.downsample.1", "transition3.3.0.1", "stage3.1.fuse_layers.2.0.1.1",
                "stage4.2.branches.3.3.bn2")


def golden_frames(step):
    """images [B, H, W, 3] fp32 NHWC of training step `step` (0-based)"""
    g = GOLDEN
    return synth.synth_inputs(g["batch"], g["height"], g["width"], seed=g["seed"] + step)[0]
