"""Fused AdamW over the lifter's parameters (train.py:337-345: optim.AdamW(volume_net params, lr, wd=0.1)).

`flatten_(module)` re-homes every parameter of `module` as a view into ONE flat fp32 buffer (state_dict,
checkpoints and torch optimizers keep working: only .data storage changes), so the update is a single
kernel over 14 M elements (capf_adamw_step) fed by the flat gradient capf_backward writes, and the
data-parallel exchange is a single all-reduce of that same buffer.

The guarded route (any of max_grad_norm / skip_nonfinite / groups) adds what the reference's loop does around
optimizer.step(): clip_grad_norm_ (train.py:196-200), the NaN skip (train.py:194), per-group learning rates
(run_3dhp.py:260-277) and the epoch-loss sums (train.py:191-192) -- decided on the device from the flat gradient
(capf_grad_sumsq + capf_adamw_step_guarded), so a step never waits for the host."""
import ctypes

import torch


def flatten_(module):
    """Moves parameter STORAGE (`p.data = view of the flat buffer`).  CA_PF notices on its next forward — it
    fingerprints the data pointers of volume_net's parameters per call (mvn/models/conpose.py::_engine) — and
    re-borrows every pointer, so this may be called before or after the first forward."""
    params = list(module.parameters())
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=params[0].device)
    off = 0
    for p in params:
        n = p.numel()
        flat[off:off + n].copy_(p.data.reshape(-1))
        p.data = flat[off:off + n].view(p.shape)
        off += n
    return flat


MAX_SEGMENTS = 64        # include/capf.h :: CAPF_OPTIM_MAX_SEGMENTS


def param_groups(layout, rules=(), total=None):
    """The merged, sorted segment list of the flat buffer: [(begin, end, lr_factor, weight_decay)].

    layout: {parameter name: (offset, numel)} (Engine.grad_layout()[0]); rules: [(keyword, lr_factor)] or
    [(keyword, lr_factor, weight_decay)] -- a parameter belongs to the first rule whose keyword occurs in its name
    (match_name_keywords, run_3dhp.py:260-272: [("sampling_offsets", 0.1)]), every other one to the default group
    (factor 1).  weight_decay None = the optimizer's own.  Adjacent parameters of one group become one segment.  Pure Python."""
    rules = [tuple(r) + (None,) * (3 - len(r)) for r in rules]
    segs, at = [], 0
    for name, (off, n) in sorted(layout.items(), key=lambda kv: kv[1][0]):
        if off != at:
            raise ValueError(f"layout has a gap or an overlap at element {at}: {name} starts at {off}")
        at = off + n
        factor, wd = next(((f, w) for key, f, w in rules if key in name), (1.0, None))
        if segs and segs[-1][2:] == (factor, wd):
            segs[-1] = (segs[-1][0], at, factor, wd)
        else:
            segs.append((off, at, factor, wd))
    if total is not None and at != total:
        raise ValueError(f"layout covers {at} elements of {total}")
    if not segs:
        raise ValueError("empty layout")
    if len(segs) > MAX_SEGMENTS:
        raise ValueError(f"{len(segs)} segments: the guarded step takes at most {MAX_SEGMENTS}")
    return segs


def module_layout(module, flat, prefix=""):
    """{prefix + name: (offset, numel)} of a module whose parameters flatten_ re-homed into `flat`, from their data pointers."""
    base, out = flat.data_ptr(), {}
    for name, p in module.named_parameters():
        off = (p.data_ptr() - base) // 4
        if not (0 <= off and off + p.numel() <= flat.numel()) or (p.data_ptr() - base) % 4:
            raise ValueError(f"{name} does not live in the flat buffer: call flatten_ first")
        out[prefix + name] = (off, p.numel())
    return out


class FusedAdamW:
    """torch.optim.AdamW semantics (decoupled weight decay on every parameter, bias-corrected moments).

    max_grad_norm (None / 0: off), skip_nonfinite=True, groups (param_groups(...)): any of them selects the guarded route, which ALWAYS leaves
    parameters and moments untouched when the scaled gradient holds a NaN / Inf, and keeps AdamW's step count on the device.  The skip is
    part of that route, not a switch of its own: skip_nonfinite=True asks for the route alone, leaving it unset (None / False without the
    other two) keeps the legacy kernel, and an explicit False next to max_grad_norm or groups is refused."""

    def __init__(self, flat_params, lr=6.4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, max_grad_norm=None,
                 skip_nonfinite=None, groups=None):
        from .lib import load_library
        self.lib = load_library()
        self.p = flat_params
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.m = torch.zeros_like(flat_params)
        self.v = torch.zeros_like(flat_params)
        self.t = 0
        self.max_grad_norm = float(max_grad_norm or 0.0)
        self.guarded = bool(max_grad_norm) or bool(skip_nonfinite) or groups is not None
        if self.guarded and skip_nonfinite is not None and not skip_nonfinite:
            raise ValueError("skip_nonfinite=False with max_grad_norm or groups: the guarded route always skips a non-finite gradient "
                             "(leave skip_nonfinite unset, or drop the other options for the legacy update)")
        self.groups = [tuple(g) for g in groups] if groups is not None else [(0, flat_params.numel(), 1.0, None)]
        self.layout = None           # [(name, offset, shape)] in named_parameters() order: state_dict() needs it (attach)
        if self.guarded:
            n, at = flat_params.numel(), 0
            for b, e, _, _ in self.groups:
                if b != at or e < b:
                    raise ValueError("groups must be sorted, disjoint segments covering the flat buffer")
                at = e
            if at != n:
                raise ValueError(f"groups cover {at} of {n} elements")
            if len(self.groups) > MAX_SEGMENTS:
                raise ValueError(f"{len(self.groups)} segments: the guarded step takes at most {MAX_SEGMENTS}")
            self.attempt = 0
            self._ctrl = None        # the device control block: made by the first call that needs the device

    @classmethod
    def from_config(cls, config, model, flat, rules=(), **kw):
        """The reference's optimizer for `model` (a CA_PF whose volume_net flatten_ re-homed into `flat`): lr = config.train.volume_net_lr
        (train.py:335), weight decay 0.1 (:345), clip_grad_norm_ at config.loss.grad_clip / volume_net_lr as train.py:196-200 divides
        (0: off), parameter groups by `rules` (run_3dhp.py:260-277: [("sampling_offsets", 0.1)])."""
        lr = float(config.train.volume_net_lr)
        clip = float(config.loss.grad_clip or 0.0)
        layout = module_layout(model.volume_net, flat)
        opt = cls(flat, lr=lr, weight_decay=kw.pop("weight_decay", 0.1), max_grad_norm=clip / lr if clip else None,
                  groups=param_groups(layout, rules, flat.numel()) if rules else None,
                  skip_nonfinite=kw.pop("skip_nonfinite", True), **kw)
        opt.attach(model.volume_net)
        return opt

    def attach(self, module):
        """Remember where each of module.named_parameters() lives in the flat buffer (state_dict / load_state_dict)."""
        lay = module_layout(module, self.p)
        self.layout = [(name, lay[name][0], tuple(p.shape)) for name, p in module.named_parameters()]
        return self

    # ---- device control block of the guarded route
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.p.device).cuda_stream)

    def _init_ctrl(self, steps):
        if self._ctrl is None:
            self._ctrl = torch.empty(self.lib.capf_optim_ctrl_bytes() // 8 + 1, dtype=torch.float64, device=self.p.device)
        rc = self.lib.capf_optim_ctrl_init(self._stream(), ctypes.c_void_p(self._ctrl.data_ptr()), int(steps))
        if rc:
            raise RuntimeError(f"capf_optim_ctrl_init failed ({rc})")

    def _segments(self):
        from .lib import OptimSegment
        segs = (OptimSegment * len(self.groups))()
        for s, (b, e, factor, wd) in zip(segs, self.groups):
            s.begin, s.end, s.lr, s.weight_decay = b, e, self.lr * factor, self.wd if wd is None else wd
        return segs

    def step(self, flat_grad, grad_scale=1.0, loss=None, rows=0):
        """grad_scale: multiplied into every gradient element inside the kernel (1 / world_size after a SUM all-reduce).
        loss (a device scalar) and rows: added to the report's epoch sums (guarded route only); never read on the host."""
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        stream = self._stream()
        if not self.guarded:
            if loss is not None:
                raise ValueError("loss accumulation needs the guarded route (max_grad_norm, skip_nonfinite or groups)")
            self.t += 1
            rc = self.lib.capf_adamw_step(stream, P(self.p), P(flat_grad), P(self.m), P(self.v), self.p.numel(), self.lr,
                                          self.betas[0], self.betas[1], self.eps, self.wd, self.t, float(grad_scale))
            if rc:
                raise RuntimeError(f"capf_adamw_step failed ({rc})")
            return
        if flat_grad.numel() != self.p.numel() or flat_grad.dtype != torch.float32 or not flat_grad.is_contiguous():
            raise ValueError("flat_grad must be a contiguous fp32 buffer of the parameters' size")
        if loss is not None and (loss.dtype != torch.float32 or loss.device != self.p.device or loss.numel() != 1):
            raise ValueError("loss must be one fp32 element on the parameters' device")
        if self._ctrl is None:
            self._init_ctrl(self.t)
        ctrl, n, segs = P(self._ctrl), self.p.numel(), self._segments()
        rc = self.lib.capf_grad_sumsq(stream, P(flat_grad), n, float(grad_scale), ctrl)
        if rc:
            raise RuntimeError(f"capf_grad_sumsq failed ({rc})")
        rc = self.lib.capf_adamw_step_guarded(stream, P(self.p), P(flat_grad), P(self.m), P(self.v), n, segs, len(segs), self.betas[0],
                                              self.betas[1], self.eps, float(grad_scale), self.max_grad_norm, self.attempt + 1,
                                              P(loss.detach()) if loss is not None else ctypes.c_void_p(0), int(rows), ctrl)
        if rc:
            raise RuntimeError(f"capf_adamw_step_guarded failed ({rc})")
        self.attempt += 1            # only a launch that went out flips the slot parity: a refused call leaves the device state readable

    def report(self):
        """Copy the device's record back (the only synchronising call): steps taken / skipped, the last attempt's gradient norm and clip
        coefficient, and the running sums loss_sum = Σ loss·rows, loss_rows = Σ rows over finite losses (epoch_loss_3d / N of
        train.py:191-192: read once per epoch and take differences)."""
        from .lib import OptimReport
        if not self.guarded:
            return {"steps_taken": self.t, "steps_skipped": 0}
        if self._ctrl is None:
            self._init_ctrl(self.t)
        rec = OptimReport()
        host = self._ctrl.view(torch.uint8)[:ctypes.sizeof(rec)].cpu()          # stream-ordered copy + wait
        ctypes.memmove(ctypes.byref(rec), host.numpy().ctypes.data, ctypes.sizeof(rec))
        out = {k: getattr(rec, k) for k, _ in rec._fields_}
        out["grad_nonfinite"] = bool(out["grad_nonfinite"])
        return out

    # ---- torch.optim.AdamW's state_dict format (the checkpoint's 'optimizer' entry, train.py:398-407)
    def _param_groups(self):
        """[(lr factor, weight decay, [index into self.layout])]: the default group first (if it has members), then by first appearance."""
        if self.layout is None:
            raise RuntimeError("state_dict needs the parameters' places in the flat buffer: call attach(module) (from_config does)")
        keys, members = [(1.0, None)], {(1.0, None): []}
        for i, (name, off, shape) in enumerate(self.layout):
            n = 1
            for d in shape:
                n *= d
            key = next(((f, w) for b, e, f, w in self.groups if b <= off and off + n <= e and (n or b < e)), None)
            if key is None:
                raise RuntimeError(f"{name} straddles two parameter groups")
            if key not in members:
                keys.append(key)
                members[key] = []
            members[key].append(i)
        if not members[keys[0]] and len(keys) > 1:
            keys = keys[1:]          # every parameter matched a rule: no empty default group, as a torch optimizer built by the rules has none
        return [(f, w, members[(f, w)]) for f, w in keys]

    def _views(self, i):
        name, off, shape = self.layout[i]
        n = 1
        for d in shape:
            n *= d
        return self.m[off:off + n].view(shape), self.v[off:off + n].view(shape)

    def state_dict(self):
        """Synchronises on the guarded route (the step count lives on the device).  exp_avg / exp_avg_sq are VIEWS of the flat moments."""
        steps = self.report()["steps_taken"]
        state, groups, nxt = {}, [], 0
        for factor, wd, idx in self._param_groups():
            ids = list(range(nxt, nxt + len(idx)))
            nxt += len(idx)
            if steps:
                for pid, i in zip(ids, idx):
                    m, v = self._views(i)
                    state[pid] = {"step": torch.tensor(float(steps)), "exp_avg": m, "exp_avg_sq": v}
            groups.append({"lr": self.lr * factor, "betas": tuple(self.betas), "eps": self.eps,
                           "weight_decay": self.wd if wd is None else wd, "amsgrad": False, "maximize": False, "foreach": None,
                           "capturable": False, "differentiable": False, "fused": None, "params": ids})
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """Resume from a torch.optim.AdamW (or FusedAdamW) state over the same parameters in the same groups.  The library keeps ONE step
        count: a state whose parameters carry different `step` values is refused."""
        mine, theirs = self._param_groups(), sd["param_groups"]
        if [len(g[2]) for g in mine] != [len(g["params"]) for g in theirs]:
            raise ValueError(f"parameter groups differ: {[len(g[2]) for g in mine]} parameters here, "
                             f"{[len(g['params']) for g in theirs]} in the loaded state")
        pairs = [(i, pid) for (_, _, idx), g in zip(mine, theirs) for i, pid in zip(idx, g["params"])]
        entries = [sd["state"].get(pid) for _, pid in pairs]
        steps = {int(float(e["step"])) if e is not None else 0 for e in entries}
        if len(steps) > 1:
            raise ValueError(f"the loaded state holds different step counts per parameter ({sorted(steps)}): "
                             "FusedAdamW keeps one count for the whole flat buffer")
        steps = steps.pop() if steps else 0
        self.m.zero_(); self.v.zero_()
        for (i, _), e in zip(pairs, entries):
            if e is not None:
                m, v = self._views(i)
                m.copy_(e["exp_avg"]); v.copy_(e["exp_avg_sq"])
        # ONE base lr and one default weight decay, taken from the first loaded group; the other groups must then spell the same
        # base lr through their own factors (and their own decays), or the loaded run was set up differently from this optimizer
        g0 = theirs[0]
        if not mine[0][0]:
            raise ValueError("the first parameter group has lr factor 0: the base lr cannot be read back from it")
        lr, wd = g0["lr"] / mine[0][0], g0["weight_decay"] if mine[0][1] is None else self.wd
        for (factor, gwd, _), g in zip(mine, theirs):
            want_lr, want_wd = lr * factor, wd if gwd is None else gwd
            if abs(g["lr"] - want_lr) > 1e-6 * max(abs(want_lr), abs(g["lr"])) or abs(g["weight_decay"] - want_wd) > 1e-6 * max(abs(want_wd), abs(g["weight_decay"])):
                raise ValueError(f"the loaded group has lr {g['lr']} / weight decay {g['weight_decay']}, this optimizer's rules give "
                                 f"{want_lr} / {want_wd} at base lr {lr}: build FusedAdamW with the loaded run's groups")
        self.lr, self.wd, self.betas, self.eps = lr, wd, tuple(g0["betas"]), g0["eps"]
        self.t = steps               # (guarded route: the count a control block starts from)
        if self.guarded and self._ctrl is not None:
            self._init_ctrl(steps)
