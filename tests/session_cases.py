"""The call sessions tests/test_gpu_sessions.py runs on ONE engine each, and whose route crossings tests/test_session_cases.py pins on the CPU
plan: plain data plus the helpers that made it.

CA_PF keeps one engine per (device, H, W) for the life of the process and sends it every batch size and every entry point its caller uses.
The engine carries state from call to call -- routes and weight packs are a function of the batch, every workspace buffer lives at
offset * batch inside an arena that only grows, lazy pack flags (h2g_lifter_dirty), self-resetting split-K counters, the stem's input
selector (Session::image), feat_batch / train_batch / t_h2_base / last_batch, debug, lanes, the fork / join events -- so a session here is an ordered
list of calls whose every result must have the bits of a fresh engine that made that one call alone.

    Step    = (kind, batch, options)           options: sorted (name, value) pairs; batch 0 where the kind has none
    Session = (id, variant, plan, steps)       plan = (backbone, H, W, dtype, plan_flags) as small_geometry_cases spells it;
                                               variant "h36m" (CA_PF) or "mpi" (no context blocks, depth 2, embed 64)

Step kinds (what runs, what is compared: test_gpu_sessions.py):
    forward            capf_forward
    backbone+lifter    capf_backbone_forward, capf_lifter_forward
    forward_u8         capf_forward_u8, option mode 0 / 1 / 2 (batch counts ENGINE frames: mode 2 reads batch / 2 crops)
    features           capf_set_features, capf_lifter_forward
    prefix             capf_forward_prefix ending inside a fork / join region of the backbone (prefix_ops below)
    profile            capf_forward_profile
    profile_launches   capf_forward_profile_launches
    set_debug          capf_set_debug, option on
    set_lanes          capf_set_lanes, option mode 0 .. 3
    train              capf_forward_train, capf_mpjpe, capf_backward; option masks (DropPath multipliers)
    train_u8           capf_forward_train_u8 (mode 0), capf_mpjpe, capf_backward
    train_features     capf_set_features, capf_lifter_forward_train, capf_mpjpe, capf_backward_maps under map_grad_mode 1
    optim              one in-place AdamW update of volume_net from the last training step's gradient; option how: "torch"
                       (torch.optim.AdamW) or "fused" (capf.optim.flatten_ + FusedAdamW + lifter_params_changed)
    stream             the following calls run on a second torch stream that waited on the first; option side

Option `at` = (H, W): the step runs at another crop size of the same model, i.e. on the model's second engine (session 6).
Inputs of a step are synth.synth_inputs(batch, H, W, seed=step_seed(kind, batch)): the same step has the same inputs in every session.
The geometries are the smallest at which the routes still switch: rows of small_geometry_cases.ROWS wherever a batch has one."""
import collections

Step = collections.namedtuple("Step", "kind batch options")
Session = collections.namedtuple("Session", "id variant plan steps")

KINDS = ("forward", "backbone+lifter", "forward_u8", "features", "prefix", "profile", "profile_launches", "set_debug", "set_lanes",
         "train", "train_u8", "train_features", "optim", "stream")
INFERENCE = ("forward", "backbone+lifter", "forward_u8", "profile", "profile_launches")      # a whole backbone and the lifter, no step saved
TRAINING = ("train", "train_u8", "train_features")
U8 = ("forward_u8", "train_u8")


def s(kind, batch=0, **options):
    assert kind in KINDS, kind
    return Step(kind, batch, tuple(sorted(options.items())))


def opt(step, name, default=None):
    return dict(step.options).get(name, default)


def step_seed(kind, batch):
    return 7000 + 101 * KINDS.index(kind) + batch


def step_id(st):
    o = "".join(f" {k}={v}" for k, v in st.options)
    return f"{st.kind}{' ' + str(st.batch) if st.batch else ''}{o}"


def ladder(*batches):
    return [s("forward", b) for b in batches]


F32 = ("hrnet_32", 64, 64, "fp32", "0")
BF16 = ("hrnet_32", 64, 64, "bf16", "0")
F16 = ("hrnet_32", 64, 64, "fp16", "0")
CPN = ("cpn", 64, 96, "fp32", "0")
SECOND_CROP = (32, 64)          # session 6's other engine: HRNet-32 32 x 64 (top map 1 x 2), rows 23 | 24 of small_geometry_cases

# ---- the named route switches: (plan, the batch below, the batch above, what moves) ------------------------------------------------------
# "kernels": the kernel of some op differs between the two batches; "streams": capf_op_stream_class does (the two-chain window 16 .. 128)
SWITCHES = {
    "fp32 4|5 two-piece GEMM":      (F32, 4, 5, "kernels"),
    "fp32 23|24 Winograd":          (F32, 23, 24, "kernels"),
    "fp32 78|83 tile takes all":    (F32, 78, 83, "kernels"),
    "fp32 15|16 two chains":        (F32, 15, 16, "streams"),
    "bf16 26|27 halo tile":         (BF16, 26, 27, "kernels"),
    "bf16 52|53 halo tile 256x64":  (BF16, 52, 53, "kernels"),
    "bf16 211|212 halo tile all":   (BF16, 211, 212, "kernels"),
    "bf16 255|256 bottlenecks":     (BF16, 255, 256, "kernels"),
    "fp16 26|27 halo tile":         (F16, 26, 27, "kernels"),
    "fp16 52|53 halo tile 256x64":  (F16, 52, 53, "kernels"),
    "fp16 255|256 bottlenecks":     (F16, 255, 256, "kernels"),
    "cpn 4|5 two-piece GEMM":       (CPN, 4, 5, "kernels"),
    "cpn 23|24 F(2,3)":             (CPN, 23, 24, "kernels"),
}

TRAIN_MIXED = [s("train", 6), s("forward", 83), s("train", 3), s("train", 6, masks=1), s("optim", how="torch"), s("forward", 8),
               s("forward", 2), s("train", 6)]

SESSIONS = [
    # 1. 4 | 5, 23 | 24, 78 | 83 and the 16 .. 128 two-chain window in both directions, large after small and small after large, 83 twice
    Session("ladder-fp32", "h36m", F32, ladder(83, 3, 24, 5, 128, 1, 23, 83, 4, 16, 78)),
    # 2. the halo tile at 27 / 53 / 212 and the fused bottlenecks at 256
    Session("ladder-bf16", "h36m", BF16, ladder(257, 3, 29, 53, 26, 257, 60, 211)),
    Session("ladder-fp16", "h36m", F16, ladder(257, 26, 53, 257)),
    # 3. maxpool, the two bilinear kernels, F(2,3)
    Session("ladder-cpn", "h36m", CPN, ladder(24, 1, 5, 4, 23, 24)),
    # 4. every entry point on one handle
    Session("mixed-entries", "h36m", F32, [
        s("forward", 24), s("backbone+lifter", 6), s("forward_u8", 12, mode=2), s("forward", 5), s("features", 5), s("prefix", 24),
        s("forward", 24), s("profile", 24), s("forward", 3), s("profile_launches", 24),
        s("set_debug", on=1), s("forward", 24), s("set_debug", on=0), s("forward", 24),
        s("set_lanes", mode=1), s("forward", 24), s("set_lanes", mode=0), s("forward", 5), s("set_lanes", mode=3), s("forward", 24),
        s("stream", side=1), s("forward", 24), s("forward", 3)]),
    # 5. training and inference interleaved: train 3 runs the fp32 pipe (no W / W^T packs); forward 8 after optim finds the lifter's lazy
    # two-piece packs stale; the last training step runs under capf_set_debug(1), whose taps the fp64 yardstick needs
    Session("train-infer", "h36m", F32, TRAIN_MIXED + [
        s("train_features", 6), s("optim", how="fused"), s("set_debug", on=1), s("train_u8", 6), s("set_debug", on=0), s("forward", 24),
        s("backbone+lifter", 8)]),
    Session("train-infer-bf16", "h36m", BF16, TRAIN_MIXED),
    # 6. two engines of one model (conpose.py: _bound_generation / _lifter_print are per engine)
    Session("two-engines", "h36m", F32, [
        s("forward", 24), s("forward", 24, at=SECOND_CROP), s("optim", how="torch", grad="synthetic"), s("forward", 24, at=SECOND_CROP),
        s("forward", 5), s("train", 6), s("optim", how="fused"), s("forward", 24), s("forward", 24, at=SECOND_CROP)]),
    # 7. the MPI-INF-3DHP variant
    Session("mpi", "mpi", F32, [s("train", 6), s("forward", 24), s("optim", how="fused"), s("forward", 3), s("train", 6)]),
]

LADDERS = ("ladder-fp32", "ladder-bf16", "ladder-fp16", "ladder-cpn")


def session(sid):
    return next(x for x in SESSIONS if x.id == sid)


def step_plan(sess, st):
    """the plan a step runs on: the session's, at the step's own crop size where it names one"""
    at = opt(st, "at")
    return sess.plan if at is None else (sess.plan[0], at[0], at[1]) + sess.plan[3:]


def crossed(plan, a, b):
    """names of the switches of `plan` that lie between batches a and b, with the direction of the move"""
    out = []
    for name, (p, lo, hi, _) in SWITCHES.items():
        if p == plan and min(a, b) <= lo and max(a, b) >= hi:
            out.append((name, "up" if a < b else "down"))
    return out


def inference_batches():
    """{(plan, batch)} of every step that runs a whole inference forward, over the sessions of the H36M model (the variant without context
    blocks shares their backbone plans; its lifter is held to float64 through its training step)"""
    return sorted({(step_plan(x, st), st.batch) for x in SESSIONS if x.variant == "h36m" for st in x.steps if st.kind in INFERENCE})


def prefix_ops(descs):
    """n for capf_forward_prefix: a checkpoint (the op count behind a region's join) of the middle fork / join region of the backbone,
    from capf_op_describe's descriptors, as test_gpu_workspace_hygiene.py picks it; -> (n, index of the last conv / fuse op that names it)"""
    n_backbone = sum(1 for d in descs if d.backbone)
    cps = sorted({d.checkpoint for d in descs[:n_backbone] if d.kind in (0, 1) and 0 < d.checkpoint < n_backbone})
    n = cps[len(cps) // 2]
    last = max(i for i in range(n_backbone) if descs[i].kind in (0, 1) and descs[i].checkpoint == n)
    return n, last
