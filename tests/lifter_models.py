"""Host models of any lifter width with a synthetic checkpoint (conftest.make_model builds the default width only): shared by
test_gpu_lifter_ops.py, test_gpu_train_widths.py and test_gpu_features.py."""
import contextlib
import copy
import io

from capf import synth


def lifter_model(backbone, dtype="fp32", embed=None, plan_flags=0, mpi=False, depth=None, wseed=81, tweak=None, joints=None, heads=None):
    """CA_PF (mpi: the MPI-INF-3DHP variant at `depth`) in eval mode on the GPU with cfg.model.poseformer.embed_dim_ratio = embed (None: the
    preset's), cfg.model.backbone.num_joints = joints and cfg.model.poseformer.num_heads = heads (None: 17 and 8); returns (model, the state_dict it was loaded with, on the CPU).  tweak(sd) edits the checkpoint before it is loaded."""
    from mvn.utils.cfg import backbone_preset, config
    if mpi:
        from model.conpose import VolumetricTriangulationNet, mpi_preset
        cfg = mpi_preset(copy.deepcopy(config), backbone)
        if depth:
            cfg.model.poseformer.depth = depth
        with contextlib.redirect_stdout(io.StringIO()):
            model = VolumetricTriangulationNet(cfg, compute_dtype=dtype).eval()
    else:
        from mvn.models.conpose import CA_PF
        cfg = backbone_preset(copy.deepcopy(config), backbone)
        cfg.model.backbone.fix_weights = True
        if embed:
            cfg.model.poseformer.embed_dim_ratio = embed
        if joints:
            cfg.model.backbone.num_joints = joints
        if heads:
            cfg.model.poseformer.num_heads = heads
        with contextlib.redirect_stdout(io.StringIO()):
            model = CA_PF(cfg, compute_dtype=dtype, plan_flags=plan_flags).eval()
    sd = synth.load_synthetic(model, seed=wseed, bn_mode="random")
    if tweak is not None:
        tweak(sd)
        model.load_state_dict(sd, strict=True)
    return model.cuda(), sd
