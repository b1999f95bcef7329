"""Seeds, float64 restatements and bounds for KeypointsL2Loss, LimbLengthError / limb_length_loss and UNCERTAINTY
(csrc/pose_losses.hip; tests/test_loss_extra.py on the CPU, tests/test_gpu_loss_extra.py on the GPU; tools/make_loss_goldens.py writes
tests/golden/losses_extra.npz from the reference on the inputs defined here).

The restatements are numpy float64 on the float32 inputs, with the gradients in closed form and the kernels' rules at the singular points:
a gradient term is 0 where the norm it divides by is 0.  Each returns, next to a value, its MASS: the sum of the absolute values of the
terms that are added to form it.  An fp64 evaluation in another order is a few 2^-53 of the mass away; the kernels then store once in fp32.

    bound(want, mass) = 2^-23 |want| + 1e-12 mass

is tests/metric_edge_cases.bound restated for these quantities: the one float32 store plus 1e-12 of the scale of what was added (there the
Frobenius norm of the pose, here the mass), nothing of the kernels' results in it."""
import numpy as np

CONNECTIVITY = ((0, 1), (1, 2), (2, 6), (5, 4), (4, 3), (3, 6), (6, 7), (7, 8), (8, 16), (9, 16), (8, 12), (11, 12), (10, 11), (8, 13),
                (13, 14), (14, 15))          # LimbLengthError.CONNECTIVITY_DICT, ContextPose/mvn/models/loss.py:185
SIGMA_EPS = 1e-6                             # loss.py:11
GRAD_POSES = 16                              # the gradient fixtures of losses_extra.npz cover the first 16 poses of metric_inputs()
GOLDEN_RTOL = 2e-6                           # tests/test_metrics.py's figure for the sibling losses against the reference
LIMB_ATOL_ULPS = 2.0 ** -21                  # x the mean limb length: the reference subtracts two fp32 norms, each good to a few ulp of a LENGTH


def bound(want, mass):
    return 2.0 ** -23 * np.abs(want) + 1e-12 * np.asarray(mass, np.float64)


def f32_scale(grad_scale):
    """grad_scale as the C ABI carries it: a float"""
    return np.float64(np.float32(grad_scale))


def golden_sigmas(n, joints=17, seed=41):
    """the two sigma tensors of the UNCERTAINTY golden: [n, joints, 3] and [n, joints, 1], values in [0.05, 0.55]"""
    rng = np.random.Generator(np.random.Philox(key=[seed, 20261021]))
    return [rng.uniform(0.05, 0.55, size=(n, joints, w)).astype(np.float32) for w in (3, 1)]


def golden_inputs():
    """(pred, gt [n, 17, 3], validity [n, 17, 1], sigmas) of losses_extra.npz: golden_cases.metric_inputs() without its frame axis"""
    from golden_cases import metric_inputs
    pred, gt, _, validity = metric_inputs()
    return pred[:, 0], gt[:, 0], validity, golden_sigmas(pred.shape[0])


def mean_limb_length(pred, gt, limbs=CONNECTIVITY):
    return float(np.mean([limb_lengths(pred, limbs)[0].mean(), limb_lengths(gt, limbs)[0].mean()]))


# ---- KeypointsL2Loss, loss.py:140-147 ----------------------------------------------------------------------------------------------------------------
def keypoints_l2(pred, gt, validity, grad_scale=1.0):
    """pred / gt [..., D], validity [..., 1] or [...] -> dict(loss, loss_mass, dpred, dpred_mass)"""
    D = pred.shape[-1]
    p, g = pred.reshape(-1, D).astype(np.float64), gt.reshape(-1, D).astype(np.float64)
    v = np.asarray(validity, np.float64).reshape(-1)
    d2 = ((g - p) ** 2).sum(1)
    s = np.sqrt(v * d2)
    denom = max(1.0, float(v.sum()))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(s > 0, f32_scale(grad_scale) * v / (s * denom), 0.0)
    dpred = np.where((s > 0)[:, None], k[:, None] * (p - g), 0.0)
    return dict(loss=s.sum() / denom, loss_mass=s.sum() / denom, dpred=dpred.reshape(pred.shape), dpred_mass=np.abs(dpred).reshape(pred.shape))


# ---- LimbLengthError, loss.py:181-201 ----------------------------------------------------------------------------------------------------------------
def limb_lengths(x, limbs):
    """x [n, J, 3] -> (lengths [n, L], difference vectors x[a] - x[b] [n, L, 3]) in float64"""
    a, b = np.array([l[0] for l in limbs]), np.array([l[1] for l in limbs])
    x = x.astype(np.float64)
    d = x[:, a] - x[:, b]
    return np.sqrt((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2), d


def limb_errors(pred, gt, limbs=CONNECTIVITY, grad_scale=1.0):
    """-> dict(err [n, L], err_mass, dpred [n, J, 3] = grad_scale * d(sum_l err[i, l]) / dpred, dpred_mass); the limbs of a joint are
    added in table order, as the kernel's gather does"""
    lp, dp = limb_lengths(pred, limbs)
    lg, _ = limb_lengths(gt, limbs)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(lp > 0, np.sign(lp - lg) / lp, 0.0)
    grad, mass = np.zeros(pred.shape, np.float64), np.zeros(pred.shape, np.float64)
    for l, (a, b) in enumerate(limbs):
        if a == b:
            continue
        c = w[:, l, None] * dp[:, l]
        grad[:, a] += c
        grad[:, b] -= c
        mass[:, a] += np.abs(c)
        mass[:, b] += np.abs(c)
    gs = f32_scale(grad_scale)
    return dict(err=np.abs(lp - lg), err_mass=lp + lg, dpred=gs * grad, dpred_mass=gs * mass)


def limb_length_error(pred, gt, limbs=CONNECTIVITY):
    """the figure of LimbLengthError.forward: mean over limbs of the mean over poses"""
    return float(limb_errors(pred, gt, limbs)["err"].mean(0).mean())


# ---- UNCERTAINTY, loss.py:7-13 -----------------------------------------------------------------------------------------------------------------------
def uncertainty(pred, gt, sigmas, grad_scale=1.0):
    """pred / gt [..., D]; sigmas: arrays [..., D] or [..., 1] -> dict(loss, loss_mass, dpred, dpred_mass, dsigma [K], dsigma_mass [K])"""
    D = pred.shape[-1]
    d = pred.reshape(-1, D).astype(np.float64) - gt.reshape(-1, D).astype(np.float64)
    rows, gs = d.shape[0], f32_scale(grad_scale)
    loss = loss_mass = 0.0
    dpred, dpred_mass, dsig, dsig_mass = np.zeros_like(d), np.zeros_like(d), [], []
    for sg in sigmas:
        w = sg.shape[-1]
        s = sg.reshape(rows, w).astype(np.float64) + SIGMA_EPS
        with np.errstate(divide="ignore", invalid="ignore"):
            u = d / s
            n = np.sqrt((u * u).sum(1))
            logs = np.log(s)
            dn = np.where((n > 0)[:, None], u / (s * n[:, None]), 0.0)
        loss += n.mean() + 0.01 * logs.mean()
        loss_mass += n.mean() + 0.01 * np.abs(logs).mean()
        dpred += dn / rows
        dpred_mass += np.abs(dn) / rows
        dsn = -(u * dn)
        if w == 1:
            dsn = dsn.sum(1, keepdims=True)
        dsig.append((gs * (dsn / rows + 0.01 / (rows * w) / s)).reshape(sg.shape))
        dsig_mass.append((gs * (np.abs(dsn) / rows + 0.01 / (rows * w) / np.abs(s))).reshape(sg.shape))
    return dict(loss=loss, loss_mass=loss_mass, dpred=(gs * dpred).reshape(pred.shape), dpred_mass=(gs * dpred_mass).reshape(pred.shape),
                dsigma=dsig, dsigma_mass=dsig_mass)


# ---- seeded cases for the GPU tests ------------------------------------------------------------------------------------------------------------------
def l2_case(rows, D, kind, seed=0):
    """pred, gt [rows, D], validity [rows, 1] float32.  kind: ones | binary (about 30 % zeros) | zeros | fractional (0.25 / 0.5).  Rows 4, 9, 14, ...
    have pred == gt: the exact hit (a single row is a plain one)."""
    rng = np.random.default_rng([seed, rows, D, ("ones", "binary", "zeros", "fractional").index(kind)])
    gt = rng.standard_normal((rows, D)).astype(np.float32)
    pred = (gt + 0.1 * rng.standard_normal((rows, D))).astype(np.float32)
    pred[4::5] = gt[4::5]
    v = {"ones": np.ones(rows), "binary": (rng.random(rows) > 0.3).astype(np.float64), "zeros": np.zeros(rows),
         "fractional": rng.choice([0.25, 0.5], rows)}[kind]
    return pred, gt, v.astype(np.float32)[:, None]


def limb_case(n, J=17, seed=0):
    """pred, gt [n, J, 3] float32 with the singular points planted (pose index modulo 8, from 8 poses up; below that the plain pose):
    1: pred == gt;  2: pred = gt mirrored in x (every length equal, the poses different);  3: two joints of pred coincide;
    4: the same two joints of gt coincide;  5: they coincide in both;  6: all of pred one point."""
    rng = np.random.default_rng([seed, n, J])
    gt = (0.3 * rng.standard_normal((n, J, 3))).astype(np.float32)
    pred = (gt + 0.05 * rng.standard_normal((n, J, 3))).astype(np.float32)
    if n >= 8 and J >= 2:
        k = np.arange(n) % 8
        pred[k == 1] = gt[k == 1]
        pred[k == 2] = gt[k == 2] * np.array([-1.0, 1.0, 1.0], np.float32)
        pred[k == 3, 1] = pred[k == 3, 0]
        gt[k == 4, 1] = gt[k == 4, 0]
        pred[k == 5, 1] = pred[k == 5, 0]
        gt[k == 5, 1] = gt[k == 5, 0]
        pred[k == 6] = pred[k == 6, :1]
    return pred, gt


LIMB_TABLES = {                              # name: (J, limbs)
    "h36m": (17, CONNECTIVITY),
    "one_limb": (2, ((0, 1),)),
    "repeated": (5, ((0, 1), (1, 2), (0, 1), (3, 4), (2, 1))),          # a limb twice, and once more reversed
    "a_equals_b": (4, ((0, 1), (2, 2), (1, 3), (0, 0))),
}


def sigma_case(rows, D, widths, seed=0):
    """one sigma per entry of widths ("full": [rows, D], "one": [rows, 1]), values in [0.05, 0.55]"""
    rng = np.random.default_rng([seed, rows, D, len(widths)])
    return [rng.uniform(0.05, 0.55, size=(rows, D if w == "full" else 1)).astype(np.float32) for w in widths]


SIGMA_SETS = {1: ("full",), 2: ("full", "one"), 8: ("one", "full", "full", "one", "one", "full", "one", "full")}
