"""CPU: what each of the twelve run entries refuses, with which code and which words, and which check refuses FIRST -- through eng.lib (the C
entries, not the binding's wrappers) on plan-only handles of the smallest HRNet-32 plan (64 x 64): fp32 with training = 1, fp32 with
training = 0, bf16.  A plan-only handle reaches every check up to the first line of the shared run check ("plan-only handle"), so a refusal
that names anything else came from a check that stands in front of it.  An entry that refuses a null argument or an op count sets no
message: the handle's last message stays what it was (SENTINEL).  The refusals that need a device (batch range, stale packs, a short
workspace) are in tests/test_gpu_sessions.py :: test_every_entry_refuses_before_it_changes_anything."""
import copy
import ctypes
from ctypes import POINTER, c_float, c_int32, c_void_p

import pytest

OK, INVALID, UNSUPPORTED, STATE = 0, -1, -2, -4      # include/capf.h
MAX_BATCH = 6
PLAN_ONLY = "plan-only handle"
NO_TRAINING = "training = 0"
SENTINEL = "unknown parameter: no such parameter"

# the arguments of every entry behind (handle, stream), in order.  p: a pointer the entry requires; o: one it does not (drop masks, std);
# mean: the three floats the uint8 entries require; feats: the four map pointers; ms / leader: the profile entries' outputs
ENTRIES = {
    "capf_forward": ("p:images", "p:k2d", "p:kcrop", "batch", "p:out"),
    "capf_backbone_forward": ("p:images", "batch"),
    "capf_forward_train": ("p:images", "p:k2d", "p:kcrop", "batch", "p:out", "o:masks"),
    "capf_forward_u8": ("p:images", "mean", "o:std", "mode", "p:k2d", "p:kcrop", "batch", "p:out"),
    "capf_backbone_forward_u8": ("p:images", "mean", "o:std", "mode", "batch"),
    "capf_forward_train_u8": ("p:images", "mean", "o:std", "mode", "p:k2d", "p:kcrop", "batch", "p:out", "o:masks"),
    "capf_lifter_forward": ("p:k2d", "p:kcrop", "batch", "p:out"),
    "capf_lifter_forward_train": ("p:k2d", "p:kcrop", "batch", "p:out", "o:masks"),
    "capf_set_features": ("feats", "batch"),
    "capf_forward_prefix": ("p:images", "p:k2d", "p:kcrop", "batch", "p:out", "n_ops"),
    "capf_forward_profile": ("p:images", "p:k2d", "p:kcrop", "batch", "p:out", "ms", "n_ops"),
    "capf_forward_profile_launches": ("p:images", "p:k2d", "p:kcrop", "batch", "p:out", "ms", "leader", "n_ops"),
}
TRAIN = ("capf_forward_train", "capf_forward_train_u8", "capf_lifter_forward_train")
U8 = ("capf_forward_u8", "capf_backbone_forward_u8", "capf_forward_train_u8")
PROFILE = ("capf_forward_profile", "capf_forward_profile_launches")


def _engine(dtype, training):
    from capf.lib import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    c = _native.make_capf_config(backbone_preset(copy.deepcopy(config), "hrnet_32"), 64, 64, compute_dtype=dtype)
    c.max_batch, c.training = MAX_BATCH, training
    return Engine(c, device=None)


@pytest.fixture(scope="module")
def handles():
    engines = {"train": _engine("fp32", 1), "infer": _engine("fp32", 0), "bf16": _engine("bf16", 1)}
    yield engines
    for e in engines.values():
        e.close()


class _Args:
    """valid arguments of an entry on an engine, each replaceable by name; nothing they point at is ever read (the handle is plan-only)"""

    def __init__(self, eng):
        self.eng = eng
        self.n = eng.lib.capf_num_ops(eng.h)
        self.n_backbone = sum(1 for i in range(self.n) if eng.op_describe(i).backbone)
        self.mem = (c_float * 64)()
        self.maps = (c_void_p * 4)(*[ctypes.addressof(self.mem)] * 4)

    def build(self, entry, **over):
        mem = ctypes.addressof(self.mem)
        args = [over.get("h", self.eng.h), c_void_p(0)]
        for a in ENTRIES[entry]:
            kind, _, name = a.partition(":")
            name = name or kind
            if name in over:
                v = over[name]
            elif kind == "p":
                v = c_void_p(mem)
            elif kind == "o":
                v = None
            elif kind == "mean":
                v = ctypes.cast(self.mem, POINTER(c_float))
            elif kind == "feats":
                v = self.maps
            elif kind == "ms":
                v = ctypes.cast(self.mem, POINTER(c_float))
            elif kind == "leader":
                v = ctypes.cast(self.mem, POINTER(c_int32))
            else:
                v = {"batch": 2, "mode": 0, "n_ops": self.n}[kind]
            args.append(v)
        return args


def _call(eng, args, entry, **over):
    """-> (return code, the handle's last message behind the call); the message in front of it is SENTINEL"""
    assert eng.lib.capf_set_param(eng.h, b"no such parameter", None, None, 0) == INVALID
    assert eng.lib.capf_last_error(eng.h).decode() == SENTINEL
    rc = getattr(eng.lib, entry)(*args.build(entry, **over))
    return rc, eng.lib.capf_last_error(eng.h).decode()


def _refused(got, code, *words):
    rc, msg = got
    assert rc == code, got
    if words:
        assert all(w in msg for w in words), got
    else:
        assert msg == SENTINEL, got                       # refused without a message of its own


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_everything_valid_reaches_the_plan_only_check(handles, entry):
    for key in ("train", "infer") if entry not in TRAIN else ("train",):
        eng = handles[key]
        _refused(_call(eng, _Args(eng), entry), STATE, PLAN_ONLY)
    if entry != "capf_set_features" and entry not in TRAIN:
        eng = handles["bf16"]
        _refused(_call(eng, _Args(eng), entry), STATE, PLAN_ONLY)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_each_null_argument(handles, entry):
    eng = handles["train"]
    args = _Args(eng)
    assert getattr(eng.lib, entry)(*args.build(entry, h=None)) == INVALID
    required = [a.partition(":")[2] or a for a in ENTRIES[entry] if a.split(":")[0] in ("p", "mean", "feats", "ms", "leader")]
    assert required
    for name in required:
        _refused(_call(eng, args, entry, **{name: None}), INVALID)
    for name in (a.partition(":")[2] for a in ENTRIES[entry] if a.startswith("o:")):
        _refused(_call(eng, args, entry, **{name: None}), STATE, PLAN_ONLY)


def test_set_features_wants_every_level(handles):
    eng = handles["train"]
    args = _Args(eng)
    for l in range(4):
        maps = (c_void_p * 4)(*[None if k == l else ctypes.addressof(args.mem) for k in range(4)])
        _refused(_call(eng, args, "capf_set_features", feats=maps), INVALID)
        _refused(_call(handles["bf16"], _Args(handles["bf16"]), "capf_set_features", feats=maps), INVALID)      # (in front of the dtype check)


@pytest.mark.parametrize("entry", TRAIN)
def test_training_0_refuses_before_the_plan_only_check(handles, entry):
    eng = handles["infer"]
    args = _Args(eng)
    _refused(_call(eng, args, entry), STATE, NO_TRAINING)
    _refused(_call(eng, args, entry, batch=0), STATE, NO_TRAINING)
    _refused(_call(eng, args, entry, k2d=None), INVALID)                                   # the entry's own nulls come first ...
    if entry in U8:
        _refused(_call(eng, args, entry, images=None), STATE, NO_TRAINING)                 # ... the image and the mean behind it
        _refused(_call(eng, args, entry, mean=None), STATE, NO_TRAINING)
        _refused(_call(eng, args, entry, mode=3), STATE, NO_TRAINING)


@pytest.mark.parametrize("entry", U8)
def test_uint8_mode_and_flip_batch_refuse_before_the_plan_only_check(handles, entry):
    eng = handles["train"]
    args = _Args(eng)
    for mode in (3, -1):
        _refused(_call(eng, args, entry, mode=mode), INVALID, "mode must be 0", "1 (every frame mirrored)", "2 (flip test")
    _refused(_call(eng, args, entry, mode=2, batch=3), INVALID, "batch must be even")
    _refused(_call(eng, args, entry, mode=3, batch=3), INVALID, "mode must be 0")          # the mode in front of the batch's parity
    _refused(_call(eng, args, entry, mode=2, batch=4), STATE, PLAN_ONLY)
    _refused(_call(eng, args, entry, mode=1, batch=3), STATE, PLAN_ONLY)
    _refused(_call(eng, args, entry, mode=3, images=None), INVALID)                        # the nulls in front of the mode
    _refused(_call(eng, args, entry, mode=3, mean=None), INVALID)


def test_set_features_dtype_then_batch_then_plan_only(handles):
    eng = handles["bf16"]
    args = _Args(eng)
    for batch in (2, 0, MAX_BATCH + 1):
        _refused(_call(eng, args, "capf_set_features", batch=batch), UNSUPPORTED, "capf_set_features", "fp32 only", "bf16")
    eng = handles["train"]
    args = _Args(eng)
    assert eng.lib.capf_max_batch(eng.h) == MAX_BATCH
    for batch in (0, -1, MAX_BATCH + 1):
        _refused(_call(eng, args, "capf_set_features", batch=batch), INVALID, "capf_set_features: batch out of range (1..capf_max_batch)")
    for batch in (1, MAX_BATCH):
        _refused(_call(eng, args, "capf_set_features", batch=batch), STATE, PLAN_ONLY)


def test_prefix_op_count_and_lifter_pointers(handles):
    eng = handles["train"]
    args = _Args(eng)
    assert 0 < args.n_backbone < args.n
    for n_ops in (-1, args.n + 1):
        _refused(_call(eng, args, "capf_forward_prefix", n_ops=n_ops), INVALID)
    _refused(_call(eng, args, "capf_forward_prefix", n_ops=-1, images=None), INVALID)
    for name in ("k2d", "kcrop", "out"):
        for n_ops in (args.n_backbone + 1, args.n):
            _refused(_call(eng, args, "capf_forward_prefix", n_ops=n_ops, **{name: None}), INVALID)
        for n_ops in (0, args.n_backbone):                                                 # a run that ends inside the backbone needs none
            _refused(_call(eng, args, "capf_forward_prefix", n_ops=n_ops, **{name: None}), STATE, PLAN_ONLY)
    _refused(_call(eng, args, "capf_forward_prefix", n_ops=args.n_backbone, k2d=None, kcrop=None, out=None), STATE, PLAN_ONLY)


@pytest.mark.parametrize("entry", PROFILE)
def test_profile_entries_want_room_for_every_op(handles, entry):
    eng = handles["train"]
    args = _Args(eng)
    _refused(_call(eng, args, entry, n_ops=args.n - 1), INVALID)
    _refused(_call(eng, args, entry, n_ops=args.n - 1, batch=0), INVALID)
    _refused(_call(eng, args, entry, n_ops=args.n + 1), STATE, PLAN_ONLY)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_plan_only_comes_before_the_batch_range(handles, entry):
    if entry == "capf_set_features":
        return                                                                             # (its own range check stands in front: above)
    eng = handles["train"]
    args = _Args(eng)
    for batch in (0, MAX_BATCH + 1):
        if entry in U8 and batch & 1:
            batch += 1
        _refused(_call(eng, args, entry, batch=batch), STATE, PLAN_ONLY)
