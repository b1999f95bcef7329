"""Generate tests/golden/pck2d_reference.json: the REAL reference's 2-D PCKh tables on small synthetic inputs.

Run where the reference exists only (it is imported read-only through oracle/_refshim.py, as oracle/make_goldens.py does; never on a GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_pck2d_golden.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tools/make_pck2d_golden.py --check    # recompute and compare with the committed one

ContextPose/mvn/datasets/human36m.py:438-479: `evaluate_2d_joint` (distance = sqrt(sum((gt - pred)^2)), detected = distance <= headsize *
threshold, rate = detected / n per joint, and the mean of the rates) and `evaluate2d` (the reshape to (-1, J, 2), headsize =
image_shape[0] / 10, the loop over thresholds, the 'all' group).  Both are methods of the dataset class, whose constructor needs the
label files; they only read `self.actual_joints`, `self.u2a_mapping`, `self.num_keypoints` and (evaluate2d) `self.labels['table']`, so they
are called unbound on a stand-in that holds those.  The module's file is executed on its own with `cv2` stubbed (imported, never called on
this path) and `np.float` (removed from numpy; the reference's :442 names it) restored as the builtin it aliased.

The inputs are float64 arrays holding fp32-representable values (the native entry takes fp32), several of them AT a threshold exactly:
offsets (3, 4) at headsize 10 x 0.5, (6, 8) at 10 x 1.0, (0, 5) and (5, 0).  Stored (data only): per case the inputs, headsize,
thresholds, and for every threshold the reference's per-joint rates in joint order and its mean rate; for the `split` case the same
for the two row ranges evaluate2d's split_by_subject forms by slicing (the reference hard-codes row 5012; the tool slices at the
case's own row)."""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in ("oracle", "contextaware-poseformer_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
sys.dont_write_bytecode = True

import numpy as np

OUT = os.path.join(ROOT, "tests", "golden", "pck2d_reference.json")
JOINTS = ["rank", "rkne", "rhip", "lhip", "lkne", "lank", "root", "belly", "neck", "nose", "head", "lsho", "lelb", "lwri", "rsho", "relb", "rwri"]


def reference_class():
    import importlib.util
    import _refshim

    class _Cv2Stub(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return 0

    stubbed = "cv2" not in sys.modules
    if stubbed:
        sys.modules["cv2"] = _Cv2Stub("cv2")
    try:
        with _refshim.reference_imports() as ri:
            spec = importlib.util.spec_from_file_location("reference_human36m", _refshim.REFERENCE_ROOT + "/mvn/datasets/human36m.py")
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            ri.check("mvn.models.loss")
            assert mod.__file__.startswith(_refshim.REFERENCE_ROOT + "/")
    finally:
        if stubbed:
            del sys.modules["cv2"]
    return mod.Human36MMultiViewDataset


def stand_in(cls, J, n):
    me = types.SimpleNamespace(actual_joints=dict(enumerate(JOINTS[:J])), u2a_mapping=list(range(J)), num_keypoints=J,
                               labels={"table": {"subject_idx": np.zeros(n, np.int64)}})
    me.evaluate_2d_joint = lambda *a: cls.evaluate_2d_joint(me, *a)
    return me


def cases():
    """[(name, gt [.., J, 2] float64, pred, image side (headsize = side / 10), thresholds, split row | None)]"""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rng = np.random.RandomState(20)
    out = []
    # ties: headsize 10; row r of joint j is offset by one of the exact-tie vectors or by a near miss
    J, n = 17, 12
    offs = f32([(3, 4), (4, 3), (6, 8), (0, 5), (5, 0), (-3, -4), (3, 4.000001), (3, 3.999999), (0, 0), (7, 7.5), (0.25, 0.5), (10, 0)])
    # (gt + off is rounded to fp32: integer ground truth keeps the exact ties exact)
    gt_i = f32(np.floor(rng.uniform(0, 100, (n, J, 2))))
    pred_i = f32(gt_i + offs[(np.arange(n)[:, None] + np.arange(J)[None]) % len(offs)])
    out.append(("ties_headsize10", gt_i, pred_i, 100, [0.5, 1.0, 0.75], None))
    # the 4-D layout evaluate2d reshapes, a 256-pixel crop side, random errors of a few head sizes
    gt4 = f32(rng.uniform(0, 256, (5, 2, J, 2)))
    pred4 = f32(gt4 + rng.normal(0, 12, gt4.shape))
    out.append(("views_headsize25p6", gt4, pred4, 256, [0.25, 0.5, 0.75, 1.0], None))
    # two subjects, split by row
    gts = f32(np.floor(rng.uniform(0, 100, (9, J, 2))))
    preds = f32(gts + offs[(2 * np.arange(9)[:, None] + np.arange(J)[None]) % len(offs)])
    out.append(("split_headsize10", gts, preds, 100, [0.5, 1.0], 4))
    # one joint, one pose
    out.append(("single", f32([[[10, 20]]]), f32([[[13, 24]]]), 100, [0.5, 0.4999], None))
    return out


def compute():
    cls = reference_class()
    had = hasattr(np, "float")
    if not had:
        np.float = float
    try:
        rec = []
        for name, gt, pred, side, thresholds, split in cases():
            J = gt.shape[-2]
            n = gt.reshape(-1, J, 2).shape[0]
            me = stand_in(cls, J, n)
            cfg = types.SimpleNamespace(model=types.SimpleNamespace(image_shape=[side, side]))
            nv, mr = cls.evaluate2d(me, gt, pred, thresholds, cfg)
            groups = {"all": {"rates": [[float(nv[t]["all"][JOINTS[j]]) for j in range(J)] for t in thresholds],
                              "mean": [float(mr[t]["all"]) for t in thresholds]}}
            if split is not None:
                g3, p3 = gt.reshape(-1, J, 2), pred.reshape(-1, J, 2)
                for key, sl in (("first", slice(None, split)), ("second", slice(split, None))):        # evaluate2d :466-471, at this case's row
                    parts = [cls.evaluate_2d_joint(me, p3[sl], g3[sl], side / 10.0, t) for t in thresholds]
                    groups[key] = {"rates": [[float(a[JOINTS[j]]) for j in range(J)] for a, _ in parts], "mean": [float(b) for _, b in parts]}
            rec.append({"name": name, "shape": list(gt.shape), "gt": gt.reshape(-1).tolist(), "pred": pred.reshape(-1).tolist(),
                        "headsize": side / 10.0, "thresholds": thresholds, "split": split, "joint_names": JOINTS[:J], "groups": groups})
    finally:
        if not had:
            del np.float
    return {"source": "ContextPose/mvn/datasets/human36m.py:438-479 evaluate2d / evaluate_2d_joint", "cases": rec}


if __name__ == "__main__":
    got = compute()
    if "--check" in sys.argv:
        want = json.load(open(OUT))
        assert want == got, "tests/golden/pck2d_reference.json differs from what the reference computes now"
        print("ok:", OUT)
    else:
        with open(OUT, "w") as f:
            json.dump(got, f, indent=0)
            f.write("\n")
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
