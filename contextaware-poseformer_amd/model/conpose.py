"""VolumetricTriangulationNet — drop-in for ContextPose_mpi/model/conpose.py:15-46 on libcapf.so.

Same call as CA_PF, but the lifter has no DeformableBlocks (ContextPose_mpi/model/pose_dformer.py:234-261),
and forward returns `(x, None)` with x laid out [B, 3, 1, 17, 1] (the `.view(b,1,p,-1,1).permute(0,3,1,2,4)`
at pose_dformer.py:260).  Everything runs through the same C ABI with `context_blocks = 0`."""
from mvn.models.conpose import CA_PF


class VolumetricTriangulationNet(CA_PF):
    def __init__(self, config, device="cuda:0", compute_dtype="fp32", backbone_bn="running", keypoint_head=None, keypoint_beta=1.0):
        # ContextPose_mpi/common/cfg.py has no backbone.type key: the width list names the backbone
        width = config.model.backbone.STAGE2.NUM_CHANNELS[0]
        if width not in (32, 48):
            raise NotImplementedError("This backbone is not implemented yet.")     # run_3dhp.py:234-235
        config.model.backbone["type"] = "hrnet_32" if width == 32 else "hrnet_48"
        pf = config.model.poseformer
        # this variant's PoseTransformer builds `config.depth` blocks per group (pose_dformer.py:199, 217-227): the engine reads it
        # from the same key (capf_config.depth, 1..8, inference and, at this app's two widths, training; the shipped configuration has 4 == 4).  Training
        # (run_3dhp.py:60-101) goes through CA_PF's native step: `out, _ = model(...)` backpropagates into volume_net.
        # backbone_bn="batch": the frozen backbone's BatchNorm follows backbone.training as in run_3dhp.py:31-35 (CA_PF.__init__)
        # keypoint_head / keypoint_beta: CA_PF's optional native 2-D keypoint head on feat0 (detect / forward_detect); None: today's module
        super().__init__(config, device, compute_dtype=compute_dtype, context_blocks=False, backbone_bn=backbone_bn,
                         keypoint_head=keypoint_head, keypoint_beta=keypoint_beta)

    def forward(self, images, keypoints_2d_cpn, keypoints_2d_cpn_crop):
        x = super().forward(images, keypoints_2d_cpn, keypoints_2d_cpn_crop)       # [B, 1, 17, 3]
        return self._layout(x), None

    def forward_u8(self, images_u8, keypoints_2d_cpn, keypoints_2d_cpn_crop, mirror="none"):
        """CA_PF.forward_u8 (the forward from uint8 BGR crops) in this variant's output layout: (x [B, 3, 1, 17, 1], None)."""
        return self._layout(super().forward_u8(images_u8, keypoints_2d_cpn, keypoints_2d_cpn_crop, mirror)), None

    def forward_features(self, features_list, keypoints_2d_cpn, keypoints_2d_cpn_crop):
        """CA_PF.forward_features in this variant's output layout: (x [B, 3, 1, 17, 1], None)."""
        return self._layout(super().forward_features(features_list, keypoints_2d_cpn, keypoints_2d_cpn_crop)), None

    def forward_detect(self, images, to_image):
        """CA_PF.forward_detect in this variant's output layout: (x [B, 3, 1, 17, 1], kcrop_px, score)."""
        x, kcrop, score = super().forward_detect(images, to_image)
        return self._layout(x), kcrop, score

    def keypoint_loss(self, images, keypoints_2d_crop, target_weight=None, sigma=2.0, reduction="mean", topk=8, return_accuracy=False):
        """CA_PF.keypoint_loss: heatmap supervision of the native head (a 0-d loss, or (loss, acc) with return_accuracy; there is no layout
        to change)."""
        return super().keypoint_loss(images, keypoints_2d_crop, target_weight, sigma, reduction, topk, return_accuracy)

    def detect_flip_test(self, images, to_image=None, shift=True, flip_pairs=None):
        """CA_PF.detect_flip_test; flip_pairs None: this variant's skeleton (capf.lib.MPI_SWAP, as forward_flip_test)."""
        from capf.lib import MPI_SWAP
        return super().detect_flip_test(images, to_image, shift, MPI_SWAP if flip_pairs is None else flip_pairs)

    def forward_detect_flip_test(self, images, to_image, shift=True, flip_pairs=None):
        """CA_PF.forward_detect_flip_test in this variant's output layout: (x [B, 3, 1, 17, 1], kcrop_px, score); flip_pairs None: this
        variant's skeleton (capf.lib.MPI_SWAP, as forward_flip_test)."""
        from capf.lib import MPI_SWAP
        x, kcrop, score = super().forward_detect_flip_test(images, to_image, shift, MPI_SWAP if flip_pairs is None else flip_pairs)
        return self._layout(x), kcrop, score

    @staticmethod
    def _layout(x):
        b, _, p, _ = x.shape
        return x.view(b, 1, p, 3, 1).permute(0, 3, 1, 2, 4).contiguous()

    def forward_flip_test(self, images2, keypoints_2d_cpn2, keypoints_2d_cpn_crop2):
        """input_augmentation (run_3dhp.py:169-180) as ONE forward of 2B frames: images2 / keypoints [2, B, ...] hold the original
        view (the reference's img[:, 0], input_2D[:, 0], ...) followed by the already-mirrored one (img[:, 1], ...), as the data
        loader provides them.  The mirrored prediction is un-mirrored with the 3DHP table (capf.lib.MPI_SWAP: x negated, joints_left
        and joints_right swapped) and averaged by capf_fliptest_fuse_swap.  Returns (out [B, 3, 1, 17, 1], None) like forward; the
        crop keypoints are normalised in place."""
        from capf.lib import MPI_SWAP, fliptest_fuse
        two, B = images2.shape[0], images2.shape[1]
        assert two == 2 and images2.is_contiguous() and keypoints_2d_cpn_crop2.is_contiguous()
        pred = CA_PF.forward(self, images2.view(2 * B, *images2.shape[2:]), keypoints_2d_cpn2.reshape(2 * B, 17, 2),
                             keypoints_2d_cpn_crop2.view(2 * B, 17, 2))
        return self._layout(fliptest_fuse(pred.view(2, B, 1, 17, 3), swap=MPI_SWAP)), None


def mpi_preset(cfg, backbone):
    """The per-backbone patch of ContextPose_mpi/run_3dhp.py:219-235 on top of common/cfg.py's defaults."""
    cfg.model.backbone.type = backbone
    cfg.model.backbone.fix_weights = True
    cfg.model.poseformer.depth = 4
    cfg.model.poseformer.levels = 4
    if backbone == "hrnet_48":
        cfg.model.backbone.STAGE2.NUM_CHANNELS = [48, 96]
        cfg.model.backbone.STAGE3.NUM_CHANNELS = [48, 96, 192]
        cfg.model.backbone.STAGE4.NUM_CHANNELS = [48, 96, 192, 384]
        cfg.model.poseformer.base_dim = 48
        cfg.model.poseformer.embed_dim_ratio = 96
    elif backbone == "hrnet_32":
        cfg.model.backbone.STAGE2.NUM_CHANNELS = [32, 64]
        cfg.model.backbone.STAGE3.NUM_CHANNELS = [32, 64, 128]
        cfg.model.backbone.STAGE4.NUM_CHANNELS = [32, 64, 128, 256]
        cfg.model.poseformer.base_dim = 32
        cfg.model.poseformer.embed_dim_ratio = 64
    else:
        raise NotImplementedError("This backbone is not implemented yet.")
    return cfg
