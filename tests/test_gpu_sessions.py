"""GPU: a reused engine against a fresh one, bit for bit, over the mixed call sessions of tests/session_cases.py.

Every other GPU test builds a model, makes one kind of call at one batch and throws the model away.  CA_PF keeps ONE engine per (device, H, W)
for the life of the process and sends it every batch and every entry point; the engine carries state from call to call (session_cases.py
lists it).  Here every session runs on one model and so on one engine, and after EVERY step everything the step produced -- joints, the
crop keypoints as written back, feat0..3 where a whole backbone ran, and for training steps the loss, the flat gradient and (ordered mode)
dL/d(maps) -- is compared with the FRESH TWIN: the same state dict (optimizer updates included) behind a new handle with its own workspace,
which makes that one step's calls and nothing else (_twin_model: the twins of a plan share a host module, never a handle).

The assertion is torch.equal: the forward and the flat gradient are documented and tested to be bit-reproducible, so there is no tolerance.
To keep a reproducibility failure apart from a state leak, the first time a (plan, kind, batch) is met the twin is built twice and the two
must agree; if they do not, the step fails as "not reproducible".  Twin results are cached in the module, keyed by (variant, plan, parameter
tag, kind, batch, options), so sessions share them.

Bit-equality to a twin means something because the twin is held to a reference: test_session_values_are_held_to_a_reference.
Refused calls (CAPF_ERR_STATE / CAPF_ERR_INVALID through the C entry) must leave no trace: test_refused_calls_leave_no_trace."""
import contextlib
import ctypes
import hashlib
import time

import pytest
import torch

import capf_oracle as oracle
import session_cases as sc
import small_geometry_cases as sg
from capf import synth
from conftest import make_model
from feature_cases import synth_maps
from test_gpu_parity import TOL_OUT
from train_yardstick import GRAD_L2_BOUND, GRAD_MAX_BOUND, check_gradients, engine_cells, engine_clip_sides, lifter64

pytestmark = pytest.mark.gpu

J = 17
WSEED = 21                 # the weights of test_gpu_small_geometry.test_end_to_end's models
MPI_DEPTH = 2
STATE, INVALID = -4, -1    # include/capf.h: CAPF_ERR_STATE, CAPF_ERR_INVALID

TWINS = {}                 # (variant, plan, parameter tag, kind, batch, options, lanes 1?) -> {name: tensor}
RESULTS = {}               # session id -> _Run
COVERED = set()            # what the sessions ran, for test_coverage
RAN_KERNELS = {}           # (plan, batch) -> backbone kernel names of the session engine's plan at that batch
TIMES = {"twin": []}       # seconds per twin (handle, packs, workspace, the step's calls)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _new_model(variant, plan, sd=None):
    """a new host model of the plan with the synthetic checkpoint (`sd`: the state dict to load over it), in train mode with the backbone
    in eval mode so that _drop_masks draws multipliers"""
    bb, _, _, dt, fl = plan
    if variant == "mpi":
        from lifter_models import lifter_model
        model, _ = lifter_model(bb, dtype=dt, mpi=True, depth=MPI_DEPTH, wseed=WSEED)
    else:
        model, _ = make_model(bb, device="cuda", wseed=WSEED, bn="random", compute_dtype=dt, plan_flags=sg.flag_bits(fl))
    if sd is not None:
        model.load_state_dict(sd, strict=True)
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = 0.2
    return model


TWIN_HOSTS = {}            # (variant, backbone, dtype, plan_flags) -> [host model, the parameter tag it holds, its synthetic state dict]


def _twin_model(variant, plan, tag, sd):
    """The host module of a twin.  Building one costs 1.9 s of host time (1.4 s of it the synthetic checkpoint) and nothing of that touches
    the engine, so the twins of a plan share one host module that holds the state dict of `tag`; what makes a twin fresh -- its handle, its
    workspace, every bit of engine state -- is created for each twin and destroyed behind it (_close)."""
    key = (variant, plan[0], plan[3], plan[4])
    if key not in TWIN_HOSTS:
        model = _new_model(variant, plan)
        TWIN_HOSTS[key] = [model, "synthetic", {k: v.detach().clone() for k, v in model.state_dict().items()}]
    host = TWIN_HOSTS[key]
    if host[1] != tag:
        host[0].load_state_dict(host[2] if sd is None else sd, strict=True)
        host[1] = tag
    return host[0]


def _close(model):
    for e in model._engines.values():
        e.close()
    model._engines.clear()


def _param_tag(model):
    h = hashlib.sha1()
    for p in model.volume_net.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


# ---- inputs: a function of (kind, batch, crop size) alone ------------------------------------------------------------------------------------
def _inputs(st, H, W):
    img, k2d, kc, gt = synth.synth_inputs(st.batch, H, W, seed=sc.step_seed(st.kind, st.batch), crop_range=(W, H), with_gt=True)
    return img, k2d, kc, gt


def _crops(st, H, W):
    """uint8 BGR crops [Bsrc, H, W, 3] of a uint8 step (mode 2: batch / 2 of them), 0 and 255 among the bytes"""
    bsrc = st.batch // 2 if sc.opt(st, "mode", 0) == 2 else st.batch
    g = torch.Generator().manual_seed(sc.step_seed(st.kind, st.batch))
    return torch.randint(0, 256, (bsrc, H, W, 3), generator=g, dtype=torch.uint8)


def _maps(eng, st):
    """caller-supplied context maps, NHWC fp32, of the engine's geometry"""
    geometry = [(c, h, w) for h, w, c in eng.feature_shapes()]
    return [m.permute(0, 2, 3, 1).contiguous().cuda() for m in synth_maps(st.batch, geometry, sc.step_seed(st.kind, st.batch))]


def _masks(model, B):
    torch.manual_seed(7)
    m = model._drop_masks(B, torch.device("cuda"))
    assert m is not None and bool((m == 0).any())
    return m


# ---- one step's calls ----------------------------------------------------------------------------------------------------------------------
def _feats(eng, B):
    return {f"feat{l}": eng.tensor(f"feat{l}")[:B] for l in range(4)}


def _run_step(model, variant, plan, st, debug=False):
    """the calls of one step on `model`'s engine of the plan's crop size; -> ({name: tensor} of everything the step produced, the engine).
    Tensors are clones on the device; scalars are 1-element tensors."""
    from capf.lib import input_constants
    _, H, W, _, _ = plan
    B, kind = st.batch, st.kind
    img, k2d, kc, gt = _inputs(st, H, W)
    eng = model.engine_for(torch.empty(1, H, W, 3, device="cuda"))
    s = _stream()
    k2d, kc = k2d.cuda(), kc.clone().cuda()
    out = torch.full((B, 1, J, 3), float("nan"), device="cuda")
    got = {}
    if kind in sc.U8:
        crops = _crops(st, H, W).cuda()
        mean, std = input_constants("cpn" if plan[0] == "cpn" else "hrnet_32")
    elif kind not in ("features", "train_features"):
        img = img.cuda()
    with torch.no_grad():
        if kind == "forward":
            eng.forward(img, k2d, kc, out, s)
        elif kind == "backbone+lifter":
            eng.backbone_forward(img, s)
            eng.lifter_forward(k2d, kc, out, s)
        elif kind == "forward_u8":
            eng.forward_u8(crops, mean, std, sc.opt(st, "mode", 0), k2d, kc, out, s)
        elif kind == "features":
            eng.set_features(_maps(eng, st), s)
            eng.lifter_forward(k2d, kc, out, s)
        elif kind == "profile":
            ms = eng.forward_profile(img, k2d, kc, out, s)
            assert len(ms) == eng.lib.capf_num_ops(eng.h)
        elif kind == "profile_launches":
            ms, leader = eng.forward_profile_launches(img, k2d, kc, out, s)
            assert max(leader) >= 0
        elif kind == "prefix":
            descs = [eng.op_describe(i) for i in range(eng.lib.capf_num_ops(eng.h))]
            n, last = sc.prefix_ops(descs)
            eng.forward_prefix(img, n, s)
            torch.cuda.synchronize()
            d = descs[last]
            t = eng.op_tensor(last, 5, (B, d.Ho, d.Wo, d.Cout), d.out_dtype).clone()
            return {"prefix output": t}, eng
        elif kind in sc.TRAINING:
            if variant == "mpi":
                gt = gt.clone()
                gt[:, :, 14] = 0                                  # run_3dhp.py:66
            gt = gt.cuda()
            masks = _masks(model, B) if sc.opt(st, "masks") else None
            _, total = eng.grad_layout_cached()
            flat = torch.full((total,), float("nan"), device="cuda")
            loss, dpred = torch.full((1,), float("nan"), device="cuda"), torch.full((B, 1, J, 3), float("nan"), device="cuda")
            P = lambda t: ctypes.c_void_p(t.data_ptr())
            if kind == "train":
                eng.forward_train(img, k2d, kc, out, s, masks)
            elif kind == "train_u8":
                eng.forward_train_u8(crops, mean, std, 0, k2d, kc, out, s, masks)
            else:
                eng.set_map_grad_mode(1)
                eng.set_features(_maps(eng, st), s)
                eng.lifter_forward_train(k2d, kc, out, s, masks)
            assert eng.lib.capf_mpjpe(ctypes.c_void_p(s), P(out), P(gt), B * J, P(loss), P(dpred), 1.0) == 0
            if kind == "train_features":
                dfeat = [torch.full((B, h, w, c), float("nan"), device="cuda") for h, w, c in eng.feature_shapes()]
                eng.backward_maps(dpred, flat, dfeat, s, masks)
                got.update({f"dfeat{l}": t for l, t in enumerate(dfeat)})
            else:
                eng.backward(dpred, flat, s, masks)
            got.update({"loss": loss, "flat gradient": flat})
        else:
            raise AssertionError(kind)
    torch.cuda.synchronize()
    got.update({"joints": out, "kcrop": kc})
    if kind not in ("features", "train_features"):
        got.update(_feats(eng, B))
    if debug and kind in sc.TRAINING and variant != "mpi":
        got["_cells"], got["_sides"] = engine_cells(eng, B), engine_clip_sides(eng, B)
    got["_k2d"], got["_gt"] = k2d, (gt if kind in sc.TRAINING else None)
    return got, eng


def _differing(a, b):
    """names of the tensors of two step results that do not have the same bits (entries whose name starts with _ are not results)"""
    keys = sorted(k for k in a if not k.startswith("_"))
    assert keys == sorted(k for k in b if not k.startswith("_")), (keys, sorted(b))
    bad = []
    for k in keys:
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or not torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)):
            bad.append(k)
    return bad


def _twin(variant, plan, tag, sd, st, lanes):
    """the fresh twin's result of a step: a new model with the state dict `sd` (None: the synthetic checkpoint), its own handle and workspace,
    this step's calls alone.  The first time a (plan, kind, batch) is met it is built twice and the two must agree."""
    options = tuple(kv for kv in st.options if kv[0] != "at")
    key = (variant, plan, tag, st.kind, st.batch, options, lanes == 1)
    if key in TWINS:
        return TWINS[key]
    first = not any(k[:2] == key[:2] and k[3:5] == key[3:5] for k in TWINS)
    results = []
    for _ in range(2 if first else 1):
        t0 = time.perf_counter()
        model = _twin_model(variant, plan, tag, sd)
        assert not model._engines
        try:
            if lanes == 1:        # capf_set_lanes(1) runs without the split-K scratch: bits of its own (test_gpu_workspace_hygiene.py)
                model.engine_for(torch.empty(1, plan[1], plan[2], 3, device="cuda")).set_lanes(1)
            got, _ = _run_step(model, variant, plan, st)
        finally:
            _close(model)
        TIMES["twin"].append(time.perf_counter() - t0)
        results.append(got)
    if first:
        bad = _differing(results[0], results[1])
        assert not bad, f"not reproducible: two fresh twins of `{sc.step_id(st)}` on {plan} differ in {bad}"
    for name, t in results[0].items():
        if not name.startswith("_"):
            assert bool(torch.isfinite(t.float()).all()), f"fresh twin of `{sc.step_id(st)}`: non-finite {name}"
    TWINS[key] = results[0]
    return results[0]


# ---- a session -------------------------------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, sess):
        self.sess = sess
        self.failures = []          # (step index, step id, what differs)
        self.compared = 0
        self.last_train = None      # what the yardstick needs of the last training step
        self.seconds = 0.0
        self.twin_seconds = 0.0
        self.error = None           # what ended the session early (raised again for every test that needs the session)


def _optim(model, st, run_state):
    """one in-place AdamW update of volume_net: from the last training step's flat gradient, or a synthetic one before any"""
    from capf.optim import FusedAdamW, flatten_, module_layout
    eng = next(iter(model._engines.values()))
    layout, total = eng.grad_layout_cached()
    grad = run_state.get("flat")
    if sc.opt(st, "grad") == "synthetic":
        grad = torch.from_numpy(synth._normal(sc.step_seed("optim", 0), "flat_grad", (total,), 1e-3)).cuda()
    assert grad is not None and grad.numel() == total
    named = list(model.volume_net.named_parameters())
    if sc.opt(st, "how") == "torch":
        if "torch_opt" not in run_state:
            run_state["torch_opt"] = torch.optim.AdamW(model.volume_net.parameters(), lr=6.4e-4, weight_decay=0.1)
        for n, p in named:
            off, cnt = layout["volume_net." + n]
            p.grad = grad[off:off + cnt].view(p.shape).clone()
        run_state["torch_opt"].step()
        run_state["torch_opt"].zero_grad(set_to_none=True)
    else:
        if "fused" not in run_state:
            flat_p = flatten_(model.volume_net)
            assert module_layout(model.volume_net, flat_p, "volume_net.") == {k: tuple(v) for k, v in layout.items()}
            run_state["fused"] = FusedAdamW(flat_p, lr=6.4e-4, weight_decay=0.1)
        run_state["fused"].step(grad)
        model.lifter_params_changed()
    torch.cuda.synchronize()


def _run_session(sid):
    if sid in RESULTS:
        if RESULTS[sid].error is not None:
            raise RESULTS[sid].error
        return RESULTS[sid]
    sess = sc.session(sid)
    run = RESULTS[sid] = _Run(sess)
    t_start = time.perf_counter()
    model = _new_model(sess.variant, sess.plan)
    tag, sd = "synthetic", None
    state, lanes, debug, side = {}, 3, False, None
    try:
        for i, st in enumerate(sess.steps):
            plan = sc.step_plan(sess, st)
            COVERED.add(st.kind)
            if st.kind == "set_debug":
                debug = bool(sc.opt(st, "on"))
                for e in model._engines.values():
                    e.set_debug(debug)
                continue
            if st.kind == "set_lanes":
                lanes = sc.opt(st, "mode")
                for e in model._engines.values():
                    e.set_lanes(lanes)
                continue
            if st.kind == "stream":
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                continue
            if st.kind == "optim":
                before = _param_tag(model)
                _optim(model, st, state)
                tag = _param_tag(model)
                assert tag != before, "the update moved no parameter"
                sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
                continue
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                got, eng = _run_step(model, sess.variant, plan, st, debug)
            if st.kind in sc.INFERENCE and (plan, st.batch) not in RAN_KERNELS:
                n_backbone = sum(1 for j in range(eng.lib.capf_num_ops(eng.h)) if eng.op_describe(j).backbone)
                RAN_KERNELS[(plan, st.batch)] = {k for _, k, _ in eng.op_table(st.batch)[:n_backbone]}
            t0 = time.perf_counter()
            want = _twin(sess.variant, plan, tag, sd, st, lanes)
            run.twin_seconds += time.perf_counter() - t0
            bad = _differing(got, want)
            run.compared += 1
            if bad:
                run.failures.append((i, sc.step_id(st), bad))
            if st.kind in sc.TRAINING:
                state["flat"] = got["flat gradient"]
                if st.kind != "train_features":
                    run.last_train = dict(got, batch=st.batch, debug=debug, masks=sc.opt(st, "masks"),
                                          params={"volume_net." + n: p.detach().cpu().clone() for n, p in model.volume_net.named_parameters()},
                                          layout=eng.grad_layout_cached()[0])
    except BaseException as e:
        run.error = e
        raise
    finally:
        torch.cuda.synchronize()
        _close(model)
    run.seconds = time.perf_counter() - t_start
    return run


@pytest.mark.parametrize("sid", [x.id for x in sc.SESSIONS])
def test_session(sid):
    """every step of the session on ONE engine has the bits of a fresh engine that made that step alone"""
    run = _run_session(sid)
    n = len(TIMES["twin"])
    print(f"{sid}: {run.compared} steps compared in {run.seconds:.2f} s ({run.twin_seconds:.2f} s of it in twins); "
          f"{n} twins so far, {sum(TIMES['twin']) / max(n, 1):.3f} s each, slowest {max(TIMES['twin'], default=0):.3f} s")
    assert run.compared == sum(1 for st in run.sess.steps if st.kind not in ("set_debug", "set_lanes", "stream", "optim"))
    assert not run.failures, "steps whose results differ from the fresh twin's (index, step, tensors): " + "; ".join(
        f"#{i} `{s}`: {', '.join(b)}" for i, s, b in run.failures)


# ---- the twins are held to a reference -----------------------------------------------------------------------------------------------------------
ROW_KEYS = {(r[:5], r.batch) for r in sg.ROWS}
NOT_ROWS = [pb for pb in sc.inference_batches() if pb not in ROW_KEYS]
YARDSTICK_SESSIONS = ["train-infer", "mpi"]


def _oracle_check(plan, B):
    """test_gpu_small_geometry.test_end_to_end for a (plan, batch) that is no row of its table: the twin of `forward B` (the step's own
    inputs, the twins' weights), its first E2E_FRAMES frames against capf_oracle.ca_pf_forward under that file's bounds"""
    from bf16_report import bf16_stage_report, check_bf16_report
    from f16_report import fp16_emulation
    bb, H, W, dt, fl = plan
    st = sc.s("forward", B)
    pick = list(sg.frames_for(H, W, B)[:sg.E2E_FRAMES])
    model, sd = make_model(bb, device="cuda", wseed=WSEED, bn="random", compute_dtype=dt, plan_flags=sg.flag_bits(fl))
    img, k2d, kc, _ = _inputs(st, H, W)
    tag = f"{bb}-{H}x{W}-{dt}-B{B}"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    try:
        with torch.no_grad():
            if dt == "fp32":
                want = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone=bb)
                got = _twin("h36m", plan, "synthetic", None, st, 3)["joints"].cpu()
                err = (got[pick] - want).abs().max().item()
                print(f"{tag}: max|twin - oracle| {err:.3e} ({len(pick)} frames)")
                assert bool(torch.isfinite(want).all()) and err <= TOL_OUT
                return
            taps_e, taps_f = {}, {}
            with (fp16_emulation() if dt == "fp16" else contextlib.nullcontext()):
                want_e = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone=bb, taps=taps_e, emulate_bf16=True)
            want_f = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone=bb, taps=taps_f)
            eng = model.engine_for(img.cuda())
            eng.set_debug(True)
            got = model.eval()(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
            assert torch.equal(got, _twin("h36m", plan, "synthetic", None, st, 3)["joints"].cpu())      # (the debug run IS the twin's forward)
            rep = bf16_stage_report(tag, eng, got, pick, taps_e, want_e, taps_f, want_f)
        check_bf16_report(rep)
    finally:
        _close(model)


def _yardstick_check(sid):
    """the SESSION's own last training step (not the twin's) against the lifter in float64 on the engine's maps, with the bounds of
    test_gpu_train_matrix.py / test_gpu_mpi_train.py: prediction 1e-5, loss 1e-6 relative, every gradient GRAD_L2_BOUND / GRAD_MAX_BOUND"""
    run = _run_session(sid)
    lt = run.last_train
    assert lt is not None
    B = lt["batch"]
    torch.set_num_threads(min(16, torch.get_num_threads()))
    feats = [lt[f"feat{l}"].cpu().double().permute(0, 3, 1, 2).contiguous() for l in range(4)]
    k2d, ref, gt = lt["_k2d"].cpu(), lt["kcrop"].cpu(), lt["_gt"].cpu()
    flat = lt["flat gradient"].cpu()
    got = {k: flat[off:off + n].view(lt["params"][k].shape).clone() for k, (off, n) in lt["layout"].items()}
    pred, loss = lt["joints"].cpu(), lt["loss"].item()
    tag = f"session {sid}, last training step (B = {B})"
    assert not lt["masks"]
    if run.sess.variant == "mpi":
        Q = {k: v.double().clone().requires_grad_(True) for k, v in lt["params"].items()}
        w64 = oracle.lifter_forward(Q, k2d.double(), ref.double(), feats, context_blocks=False, depth=MPI_DEPTH)
        l64 = oracle.mpjpe(w64, gt.double())
        l64.backward()
        g64, w64, l64 = {k: q.grad for k, q in Q.items()}, w64.detach(), l64.item()
    else:
        assert lt["debug"], "the step must have run under capf_set_debug(1): the yardstick needs the samplers' cells"
        g64, w64, l64 = lifter64(lt["params"], k2d, ref, gt, feats, lt["_cells"], None, lt["_sides"])
    perr, lerr = (pred.double() - w64).abs().max().item(), abs(loss - l64) / abs(l64)
    print(f"  {tag}: prediction max|hip - fp64| {perr:.2e}, loss {loss:.6f} (relative error {lerr:.2e})")
    assert perr <= 1e-5 and lerr <= 1e-6, (perr, lerr)
    if run.sess.variant != "mpi":
        check_gradients(tag, got, g64)
        return
    assert set(got) == set(g64)
    for k, t in g64.items():
        d = got[k].double() - t
        l2, mx = (d.norm() / t.norm().clamp_min(1e-30)).item(), (d.abs().max() / t.abs().max().clamp_min(1e-30)).item()
        assert l2 <= GRAD_L2_BOUND and mx <= GRAD_MAX_BOUND, (k, l2, mx)


@pytest.mark.parametrize("what", ["rows"] + [f"{p[0]}-{p[1]}x{p[2]}-{p[3]}-B{b}" for p, b in NOT_ROWS] + [f"train:{s}" for s in YARDSTICK_SESSIONS])
def test_session_values_are_held_to_a_reference(what):
    """rows: every inference (plan, batch) of a session is a row of small_geometry_cases.ROWS -- test_gpu_small_geometry.test_end_to_end
    holds a fresh engine at that plan and batch to the oracle -- or is one of NOT_ROWS, each of which has a case of its own here;
    train:<session>: the session's own last training step against the fp64 yardstick.  No tolerance of this file's own."""
    if what == "rows":
        assert len(sc.inference_batches()) - len(NOT_ROWS) >= 20
        assert all(pb in ROW_KEYS or pb in NOT_ROWS for pb in sc.inference_batches())
        return
    if what.startswith("train:"):
        return _yardstick_check(what[6:])
    plan, B = NOT_ROWS[[f"{p[0]}-{p[1]}x{p[2]}-{p[3]}-B{b}" for p, b in NOT_ROWS].index(what)]
    _oracle_check(plan, B)


# ---- refused calls ---------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_no_trace():
    """the C entries themselves (eng.lib, not the binding's wrappers): CAPF_ERR_STATE with a reason for a lifter call on maps of another batch,
    on half-written maps, on a fresh workspace, and for a backward whose step an inference forward overwrote; CAPF_ERR_INVALID for an odd
    flip-test batch.  A refused call changes neither the saved step's generation nor the next forward's bits."""
    from capf.lib import input_constants
    plan = sc.F32
    _, H, W, _, _ = plan
    st24 = sc.s("forward", 24)
    want = _twin("h36m", plan, "synthetic", None, st24, 3)
    model = _new_model("h36m", plan)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    try:
        eng = model.engine_for(torch.empty(1, H, W, 3, device="cuda"))
        lib, h = eng.lib, eng.h
        S = lambda: ctypes.c_void_p(_stream())

        def ins(B, seed_kind="forward"):
            img, k2d, kc, gt = _inputs(sc.s(seed_kind, B), H, W)
            return img.cuda(), k2d.cuda(), kc.cuda(), torch.full((B, 1, J, 3), float("nan"), device="cuda")

        def refused(rc, code, *words):
            msg = lib.capf_last_error(h).decode()
            assert rc == code, (rc, msg)
            assert msg and all(w in msg for w in words), msg

        def then_forward_24_has_the_twins_bits(after):
            got, _ = _run_step(model, "h36m", plan, st24)
            bad = _differing(got, want)
            assert not bad, f"forward 24 after {after}: {bad} differ from the fresh twin's"

        img8, k8, c8, o8 = ins(8)
        img4, k4, c4, o4 = ins(4)
        eng.ensure_workspace(24)
        # 1. maps of another batch
        eng.backbone_forward(img8, _stream())
        gen, kept = lib.capf_train_generation(h), c4.clone()
        refused(lib.capf_lifter_forward(h, S(), P(k4), P(c4), 4, P(o4)), STATE, "capf_lifter_forward", "context maps of this batch")
        torch.cuda.synchronize()
        assert lib.capf_train_generation(h) == gen and torch.equal(c4, kept) and bool(torch.isnan(o4).all())
        assert lib.capf_lifter_forward(h, S(), P(k8), P(c8), 8, P(o8)) == 0          # (the maps of batch 8 are still served)
        then_forward_24_has_the_twins_bits("a lifter call on maps of another batch")
        # 2. maps half written by a prefix run that ended inside the backbone
        n, _ = sc.prefix_ops([eng.op_describe(i) for i in range(lib.capf_num_ops(h))])
        eng.forward_prefix(img8, n, _stream())
        img8, k8, c8, o8 = ins(8)
        refused(lib.capf_lifter_forward(h, S(), P(k8), P(c8), 8, P(o8)), STATE, "capf_lifter_forward")
        then_forward_24_has_the_twins_bits("a lifter call behind a prefix run")
        # 3. a new workspace holds no maps
        eng.backbone_forward(img8, _stream())
        torch.cuda.synchronize()
        assert lib.capf_set_workspace(h, P(eng._ws), eng.workspace_bytes(eng._ws_batch)) == 0
        refused(lib.capf_lifter_forward(h, S(), P(k8), P(c8), 8, P(o8)), STATE, "capf_lifter_forward")
        torch.cuda.synchronize()
        assert bool(torch.isnan(o8).all())
        then_forward_24_has_the_twins_bits("a lifter call behind capf_set_workspace")
        # 4. a backward whose step an inference forward of the same batch overwrote
        img6, k6, c6, o6 = ins(6, "train")
        _, total = eng.grad_layout_cached()
        flat, dout = torch.full((total,), float("nan"), device="cuda"), torch.ones(6, 1, J, 3, device="cuda")
        eng.forward_train(img6, k6, c6, o6, _stream(), None)
        eng.forward(img6, k6, c6.clone(), o6, _stream())
        refused(lib.capf_backward(h, S(), P(dout), 6, P(flat), None), STATE)
        torch.cuda.synchronize()
        assert bool(torch.isnan(flat).all())
        then_forward_24_has_the_twins_bits("a refused backward")
        # 5. an odd flip-test batch
        crops = torch.zeros(3, H, W, 3, dtype=torch.uint8, device="cuda")
        mean, std = input_constants("hrnet_32")
        img7, k7, c7, o7 = ins(7)
        gen = lib.capf_train_generation(h)
        refused(lib.capf_forward_u8(h, S(), P(crops), mean, std, 2, P(k7), P(c7), 7, P(o7)), INVALID, "even")
        assert lib.capf_train_generation(h) == gen
        then_forward_24_has_the_twins_bits("a refused capf_forward_u8")
    finally:
        torch.cuda.synchronize()
        _close(model)
    COVERED.add("refused")


def test_every_entry_refuses_before_it_changes_anything(monkeypatch):
    """each of the twelve run entries (the C entries) on one engine of the fp32 64 x 64 plan with max_batch 4: batch 0 and batch 5 are
    CAPF_ERR_INVALID; a call between capf_set_param and capf_params_changed, and a call on a workspace one byte too small, are
    CAPF_ERR_STATE.  Behind every refusal capf_train_generation is what it was, the NaN-filled output and the crop keypoints are untouched;
    at the end `forward 2` has the bits of the fresh twin (tests/test_call_prologue.py: the refusals that need no device)."""
    from capf.lib import input_constants
    from mvn.models import _native
    plan, MAXB = sc.F32, 4
    _, H, W, _, _ = plan
    st2 = sc.s("forward", 2)
    want = _twin("h36m", plan, "synthetic", None, st2, 3)
    monkeypatch.setattr(_native, "MAX_BATCH", MAXB)
    model = _new_model("h36m", plan)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    try:
        eng = model.engine_for(torch.empty(1, H, W, 3, device="cuda"))
        lib, h = eng.lib, eng.h
        assert lib.capf_max_batch(h) == MAXB
        S = lambda: ctypes.c_void_p(_stream())
        img, k2d, kc, _ = _inputs(sc.s("forward", MAXB + 1), H, W)
        img, k2d, kc = img.cuda(), k2d.cuda(), kc.cuda()
        kept = kc.clone()
        out = torch.full((MAXB + 1, 1, J, 3), float("nan"), device="cuda")
        crops = _crops(sc.s("forward_u8", MAXB + 1), H, W).cuda()
        mean, std = input_constants("hrnet_32")
        maps = _maps(eng, sc.s("features", MAXB + 1))
        n = lib.capf_num_ops(h)
        ms, leader = (ctypes.c_float * n)(), (ctypes.c_int32 * n)()
        entries = {
            "capf_forward": lambda B: lib.capf_forward(h, S(), P(img), P(k2d), P(kc), B, P(out)),
            "capf_backbone_forward": lambda B: lib.capf_backbone_forward(h, S(), P(img), B),
            "capf_forward_train": lambda B: lib.capf_forward_train(h, S(), P(img), P(k2d), P(kc), B, P(out), None),
            "capf_forward_u8": lambda B: lib.capf_forward_u8(h, S(), P(crops), mean, std, 0, P(k2d), P(kc), B, P(out)),
            "capf_backbone_forward_u8": lambda B: lib.capf_backbone_forward_u8(h, S(), P(crops), mean, std, 0, B),
            "capf_forward_train_u8": lambda B: lib.capf_forward_train_u8(h, S(), P(crops), mean, std, 0, P(k2d), P(kc), B, P(out), None),
            "capf_lifter_forward": lambda B: lib.capf_lifter_forward(h, S(), P(k2d), P(kc), B, P(out)),
            "capf_lifter_forward_train": lambda B: lib.capf_lifter_forward_train(h, S(), P(k2d), P(kc), B, P(out), None),
            "capf_set_features": lambda B: lib.capf_set_features(h, S(), eng._ptrs4(maps), B),
            "capf_forward_prefix": lambda B: lib.capf_forward_prefix(h, S(), P(img), P(k2d), P(kc), B, P(out), n),
            "capf_forward_profile": lambda B: lib.capf_forward_profile(h, S(), P(img), P(k2d), P(kc), B, P(out), ms, n),
            "capf_forward_profile_launches": lambda B: lib.capf_forward_profile_launches(h, S(), P(img), P(k2d), P(kc), B, P(out), ms, leader, n),
        }
        assert len(entries) == 12

        def all_refuse(B, code, *words):
            gen = lib.capf_train_generation(h)
            for name, call in entries.items():
                rc = call(B)
                msg = lib.capf_last_error(h).decode()
                assert rc == code and all(w in msg for w in words), (name, B, rc, msg)
                assert lib.capf_train_generation(h) == gen, name
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()) and torch.equal(kc, kept)

        eng.ensure_workspace(MAXB)
        eng.forward_train(img[:2], k2d[:2], kc[:2].clone(), torch.empty(2, 1, J, 3, device="cuda"), _stream(), None)      # a saved step to lose
        for B in (0, MAXB + 1):
            all_refuse(B, INVALID, "batch out of range")
        name, shape, _ = eng.schema()[0]
        shp = (ctypes.c_int64 * 4)(*(list(shape) + [0] * (4 - len(shape))))
        assert lib.capf_set_param(h, name.encode(), ctypes.c_void_p(eng._bound[name]), shp, len(shape)) == 0
        all_refuse(2, STATE, "capf_params_changed has not been called")
        assert lib.capf_params_changed(h, S()) == 0
        assert lib.capf_set_workspace(h, P(eng._ws), eng.workspace_bytes(3) - 1) == 0
        all_refuse(3, STATE, "workspace missing or too small")
        assert lib.capf_set_workspace(h, P(eng._ws), eng.workspace_bytes(eng._ws_batch)) == 0
        got, _ = _run_step(model, "h36m", plan, st2)
        bad = _differing(got, want)
        assert not bad, f"forward 2 behind the refused calls: {bad} differ from the fresh twin's"
    finally:
        torch.cuda.synchronize()
        _close(model)


# ---- what ran --------------------------------------------------------------------------------------------------------------------------------
def test_coverage():
    """(this test runs last: the whole module in one session)  The sessions together reached every step kind, and at every (plan, batch) that
    is a row of small_geometry_cases the engine's plan runs every backbone kernel the row lists."""
    for x in sc.SESSIONS:
        _run_session(x.id)
    missing = sorted(set(sc.KINDS) - COVERED)
    assert not missing, missing
    rows = {(r[:5], r.batch): r for r in sg.ROWS}
    checked = 0
    for key, kernels in RAN_KERNELS.items():
        if key in rows:
            assert sg.prefixes_hold(kernels, rows[key].expected_kernel_prefixes) == [], (key, sorted(kernels))
            checked += 1
    assert checked >= 20, checked
    wanted = set()
    for x in sc.SESSIONS:
        for r in sg.ROWS:
            if r[:5] == x.plan and any(st.batch == r.batch and st.kind in sc.INFERENCE for st in x.steps):
                wanted.update(p for p in r.expected_kernel_prefixes if not p.startswith("!"))
    ran = set().union(*RAN_KERNELS.values())
    unmet = sorted(p for p in wanted if not any(k.startswith(p) for k in ran))
    assert len(wanted) >= 15 and not unmet, unmet
    n = len(TIMES["twin"])
    print(f"{n} twins, {sum(TIMES['twin']):.1f} s in all, {sum(TIMES['twin']) / max(n, 1):.3f} s each; sessions: " +
          ", ".join(f"{sid} {r.seconds:.1f} s" for sid, r in RESULTS.items()))
