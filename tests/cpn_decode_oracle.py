"""CPN's two-peak heatmap decode (cpn/test.py:79-108) as include/capf.h states it for capf_cpn_decode, statement for statement in numpy
float64 -- the yardstick of tests/test_cpn_detect.py and tests/test_gpu_cpn_detect.py -- and the heatmap generator both use.

The blur is cv2.GaussianBlur(P, (21, 21), 0) restated: separable, rows pass first, reflect-101 borders, taps exp(-(i - 10)^2 / (2 * 3.5^2))
normalised by their sum.  OpenCV is absent, so the last bits of that blur are PARITY UNPINNED; what IS pinned: the kernel against this
restatement.  numpy has no fma, so this blur rounds twice per tap where the kernel rounds once: the two agree within

    gamma = 44 * 2^-53 * blur(|P|)          (two passes of 21 terms, at most (21 + 1) u each, u = 2^-53)

per cell, and everything behind the blur -- the integer peaks, the shift, the float32 outputs -- agrees EXACTLY whenever the peaks are
separated by more than that.  decode() therefore reports the separations: gap1 = D_max - D_runner-up, gap2 the same after the zeroing, and a
case is DECIDED when each gap exceeds 4 gamma (gamma taken at the two cells of that gap)."""
import math

import numpy as np

BORDER, NTAPS = 10, 21
U = 2.0 ** -53


def taps():
    """g_i = e_i / sum(e): e mirrored (bit-symmetric), the sum correctly rounded (math.fsum)"""
    sigma = 0.3 * ((NTAPS - 1) * 0.5 - 1.0) + 0.8          # OpenCV's rule for ksize = 21, sigma = 0: 3.5
    e = [math.exp(-((i - BORDER) ** 2) / (2.0 * sigma * sigma)) for i in range(BORDER + 1)]
    e = e + e[BORDER - 1::-1]
    s = math.fsum(e)
    return np.array([v / s for v in e], dtype=np.float64)


def blur(P, g):
    """rows pass, then columns pass, of g over P with reflect-101 borders; taps ascending"""
    Hp, Wp = P.shape
    X = np.pad(P, ((0, 0), (BORDER, BORDER)), mode="reflect")
    R = np.zeros_like(P)
    for i in range(NTAPS):
        R = R + g[i] * X[:, i:i + Wp]
    Y = np.pad(R, ((BORDER, BORDER), (0, 0)), mode="reflect")
    D = np.zeros_like(P)
    for i in range(NTAPS):
        D = D + g[i] * Y[i:i + Hp, :]
    return D


def _first_two(D):
    """(flat index of the first maximum, its value minus the largest value of any other cell, flat index of that other cell)"""
    flat = D.ravel()
    i1 = int(flat.argmax())
    rest = flat.copy()
    rest[i1] = -np.inf
    i2 = int(rest.argmax())
    return i1, float(flat[i1] - rest[i2]), i2


def decode(z, dec=(1.0, 0.0, 1.0, 0.0), to_image=None, g=None):
    """z: [H, W] float32 heatmap of one (frame, joint).  Returns a dict: D (blurred plane, float64), peaks ((y1, x1), (y2, x2)) in padded
    coordinates, xy (float64 heatmap coordinates), kcrop / k2d (float32 pairs; k2d None without to_image [2, 3] float32), score (float32),
    gap1, gap2, gamma1, gamma2, decided, degenerate."""
    z = np.asarray(z, dtype=np.float32)
    H, W = z.shape
    g = taps() if g is None else np.asarray(g, dtype=np.float64)
    nan32 = np.float32(np.nan)
    M = z.max() if np.isfinite(z).all() else nan32
    if not np.isfinite(M) or M == 0:
        nn = np.array([nan32, nan32])
        return dict(D=np.full((H + 2 * BORDER, W + 2 * BORDER), np.nan), peaks=None, xy=np.array([np.nan, np.nan]), kcrop=nn,
                    k2d=None if to_image is None else nn.copy(), score=nan32, gap1=np.nan, gap2=np.nan, gamma1=np.nan, gamma2=np.nan,
                    decided=True, degenerate=True)
    r0 = z / np.float32(255) + np.float32(0.5)
    n = z / M                                                            # float32
    P = np.zeros((H + 2 * BORDER, W + 2 * BORDER), dtype=np.float64)
    P[BORDER:BORDER + H, BORDER:BORDER + W] = n
    D = blur(P, g)
    G = 44.0 * U * blur(np.abs(P), g)
    i1, gap1, ir = _first_two(D)
    gamma1 = max(G.ravel()[i1], G.ravel()[ir])
    D2 = D.copy()
    D2.ravel()[i1] = 0.0
    i2, gap2, ir2 = _first_two(D2)
    gamma2 = max(G.ravel()[i2], G.ravel()[ir2])
    Wp = W + 2 * BORDER
    y1, x1, y2, x2 = i1 // Wp, i1 % Wp, i2 // Wp, i2 % Wp
    x, y = float(x1 - BORDER), float(y1 - BORDER)
    px, py = float(x2 - x1), float(y2 - y1)
    ln = float(np.sqrt(np.float64(px * px + py * py)))
    if ln > 1e-3:
        x += (0.25 * px) / ln
        y += (0.25 * py) / ln
    x = max(0.0, min(x, float(W - 1)))
    y = max(0.0, min(y, float(H - 1)))
    score = r0[int(round(y)), int(round(x))]
    f = np.float32
    kx = f(dec[0]) * f(x) + f(dec[1])
    ky = f(dec[2]) * f(y) + f(dec[3])
    k2d = None
    if to_image is not None:
        A = np.asarray(to_image, dtype=np.float32)
        k2d = np.array([(A[0, 0] * kx + A[0, 1] * ky) + A[0, 2], (A[1, 0] * kx + A[1, 1] * ky) + A[1, 2]], dtype=np.float32)
    return dict(D=D, peaks=((y1, x1), (y2, x2)), xy=np.array([x, y]), kcrop=np.array([kx, ky], dtype=np.float32), k2d=k2d, score=score,
                gap1=gap1, gap2=gap2, gamma1=gamma1, gamma2=gamma2, decided=bool(gap1 > 4 * gamma1 and gap2 > 4 * gamma2),
                degenerate=False)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 9), (7, 1), (3, 2), (16, 12), (64, 48), (96, 72)]
JC = [(1, 1), (1, 20), (1, 32), (17, 17), (17, 20), (17, 32), (32, 32)]      # J in 1, 17, 32 with C in J, 20, 32 where C >= J
BATCHES = [1, 3]


def round_to(x, dtype):
    """float32 array -> the nearest value of a 16-bit torch dtype name ("bf16"), back in float32; "fp32": unchanged"""
    if dtype == "fp32":
        return x
    import torch
    return torch.from_numpy(x).to(torch.bfloat16 if dtype == "bf16" else torch.float16).float().numpy()


def make_maps(B, H, W, C, J, seed, dtype="fp32"):
    """[B, H, W, C] float32 NHWC (values exact in `dtype`): per joint one or two planted blobs at random sub-pixel centres plus noise;
    every fifth joint (20 %) sits on a negative background.  Channels >= J hold noise the decode must not read."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, H, W, C), dtype=np.float32)
    for b in range(B):
        for c in range(C):
            m = 0.02 * rng.standard_normal((H, W))
            if c < J:
                for k in range(int(rng.integers(1, 3))):
                    cy, cx = rng.uniform(-0.5, H - 0.5), rng.uniform(-0.5, W - 0.5)
                    s = rng.uniform(0.8, 2.5)
                    m += rng.uniform(0.4, 1.0) * (0.6 if k else 1.0) * np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2.0 * s * s))
                m *= rng.uniform(20.0, 200.0)                            # (final_predict ends in a BatchNorm: heatmap values of tens to hundreds)
                if (b * J + c) % 5 == 4:
                    m -= 0.3 * np.abs(m).max()
            out[b, :, :, c] = m
    return round_to(out.astype(np.float32), dtype)
