"""The 2-D keypoint head's yardstick: final_layer as torch F.conv2d in float64 plus the decode rules of include/capf.h in numpy, the cases
the tests run, and the bounds they hold the kernels to.  The reference never runs this layer (pose_hrnet.py:497-501 is commented out), so
no golden exists: everything here is evaluated on the spot.

Bounds are the project's rule (EXPERIMENTS R22.1): 4 x d32 + 1e-6 x scale, d32 being the distance of the SAME torch evaluation in float32
from the float64 one -- nothing of the kernel's result enters a bound.  The argmax decode is discontinuous, so it is compared exactly, and
`margins` shows that the comparison is fair: in every case the gaps the decode decides on are at least 50 x d32 wide."""
import numpy as np
import torch
import torch.nn.functional as F

SEEDS = (0, 1, 2)
# (B, H, W, C, J): one pixel, one row, two columns, one tile, two tiles, more slabs than lanes, non-multiples of the tile, wide C, J = 1 / 32
SHAPES = ((1, 1, 1, 32, 17), (2, 1, 5, 32, 17), (3, 3, 2, 48, 17), (2, 8, 8, 32, 17), (3, 16, 12, 48, 17), (2, 64, 48, 32, 17),
          (2, 64, 64, 32, 17), (1, 24, 18, 256, 17), (2, 8, 8, 32, 1), (2, 8, 8, 32, 32))
ONE_INTERIOR = (2, 4, 4, 32, 17)       # the only pixel with 1 < px < W - 1 and 1 < py < H - 1 is (2, 2)
MARGIN = 50.0


def make_case(shape, seed):
    B, H, W, C, J = shape
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, H, W, C)).astype(np.float32)
    Wt = (rng.standard_normal((J, C)) / np.sqrt(C)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(J)).astype(np.float32)
    return X, Wt, bias


def round_map(X, dtype):
    """X as a 16-bit map holds it, widened back to float32 (torch.bfloat16 / torch.float16; torch.float32: X itself)"""
    return torch.from_numpy(X).to(dtype).to(torch.float32).numpy()


def logits(X, Wt, bias, dtype=torch.float64):
    """z [B, J, H, W] = conv2d(X as NCHW, Wt [J, C, 1, 1], bias) in `dtype`, as a torch tensor"""
    x = torch.as_tensor(X).to(dtype).permute(0, 3, 1, 2)
    w = torch.as_tensor(Wt).to(dtype)[:, :, None, None]
    return F.conv2d(x, w, None if bias is None else torch.as_tensor(bias).to(dtype))


def logits_chain32(X, Wt, bias):
    """The expression capf.h states, on the host: z = bias, then z = fma(x_c, w_c, z) for c ascending, every fma rounded to float32 (the
    product of two float32 values is exact in float64)."""
    B, H, W, C = X.shape
    z = np.broadcast_to(bias.astype(np.float32)[None, :, None, None], (B, Wt.shape[0], H, W)).copy()
    x64, w64 = X.astype(np.float64), Wt.astype(np.float64)
    for c in range(C):
        z = (x64[..., c][:, None] * w64[:, c][None, :, None, None] + z.astype(np.float64)).astype(np.float32)
    return z


def decode_argmax(z):
    """numpy, the rule of capf.h on z [B, J, H, W] of any float dtype: (xy [B, J, 2] heatmap coordinates float64, score [B, J], idx)"""
    z = np.asarray(z)
    B, J, H, W = z.shape
    xy, score, idx = np.zeros((B, J, 2)), np.zeros((B, J), z.dtype), np.zeros((B, J), np.int64)
    for b in range(B):
        for j in range(J):
            h = z[b, j]
            if np.isnan(h).any():
                xy[b, j], score[b, j], idx[b, j] = np.nan, np.nan, -1
                continue
            i = int(np.argmax(h))                    # the first maximum in row-major order
            py, px = divmod(i, W)
            x, y = float(px), float(py)
            if 1 < px < W - 1 and 1 < py < H - 1:
                x += 0.25 * np.sign(h[py, px + 1] - h[py, px - 1])
                y += 0.25 * np.sign(h[py + 1, px] - h[py - 1, px])
            if not h[py, px] > 0:
                x, y = 0.0, 0.0
            xy[b, j], score[b, j], idx[b, j] = (x, y), h[py, px], i
    return xy, score, idx


def decode_integral(z, beta):
    """torch, differentiable: (xy [B, J, 2], score [B, J]) of z [B, J, H, W] in z's dtype"""
    B, J, H, W = z.shape
    p = torch.softmax(beta * z.reshape(B, J, H * W), dim=-1).reshape(B, J, H, W)
    col = torch.arange(W, dtype=z.dtype)
    row = torch.arange(H, dtype=z.dtype)
    x = (p.sum(2) * col).sum(-1)
    y = (p.sum(3) * row).sum(-1)
    return torch.stack([x, y], -1), z.reshape(B, J, -1).max(-1).values


def to_outputs(xy, decode, to_image=None):
    """(kcrop, k2d | None) of heatmap coordinates xy [B, J, 2] (torch or numpy, any float dtype): kcrop = (sx x + ox, sy y + oy),
    k2d = A_b (kcrop, 1)"""
    sx, ox, sy, oy = decode
    kc_x, kc_y = sx * xy[..., 0] + ox, sy * xy[..., 1] + oy
    stack = torch.stack if isinstance(xy, torch.Tensor) else np.stack
    kcrop = stack([kc_x, kc_y], -1)
    if to_image is None:
        return kcrop, None
    A = to_image if not isinstance(xy, torch.Tensor) else torch.as_tensor(to_image).to(xy.dtype)
    k2d = stack([A[:, None, 0, 0] * kc_x + A[:, None, 0, 1] * kc_y + A[:, None, 0, 2],
                 A[:, None, 1, 0] * kc_x + A[:, None, 1, 1] * kc_y + A[:, None, 1, 2]], -1)
    return kcrop, k2d


def kcrop_f32(xy, decode):
    """kcrop as the kernel rounds it: float32 product, then float32 sum (xy exact in float32)"""
    d = np.asarray(decode, np.float32)
    xy = np.asarray(xy, np.float32)
    return np.stack([d[0] * xy[..., 0] + d[1], d[2] * xy[..., 1] + d[3]], -1).astype(np.float32)


def margins(z64, d32):
    """Per case: the smallest of (top-1 - top-2 gap, |horizontal neighbour difference|, |vertical neighbour difference|) / d32 over every
    (frame, joint); neighbour differences only where the quarter shift reads them.  inf where nothing is decided (one pixel)."""
    z = np.asarray(z64)
    B, J, H, W = z.shape
    worst = np.inf
    for b in range(B):
        for j in range(J):
            h = z[b, j]
            flat = np.sort(h.reshape(-1))
            if flat.size > 1:
                worst = min(worst, (flat[-1] - flat[-2]) / d32)
            py, px = divmod(int(np.argmax(h)), W)
            if 1 < px < W - 1 and 1 < py < H - 1:
                worst = min(worst, abs(h[py, px + 1] - h[py, px - 1]) / d32, abs(h[py + 1, px] - h[py - 1, px]) / d32)
    return worst


def score_margin(z64, d32):
    """the third decision of the decode, score <= 0: the smallest |maximum| / d32 over every (frame, joint)"""
    z = np.asarray(z64)
    return float(np.abs(z.reshape(z.shape[0], z.shape[1], -1).max(-1)).min() / d32)


def heat_case(shape, seed, dtype=torch.float32):
    """Everything the logit / argmax tests of one case need: the (rounded) map, weights, z64, z32, d32 and the heat bound"""
    X, Wt, bias = make_case(shape, seed)
    X = round_map(X, dtype)
    z64 = logits(X, Wt, bias)
    z32 = logits(X, Wt, bias, torch.float32)
    d32 = (z32.double() - z64).abs().max().item()
    return {"X": X, "Wt": Wt, "bias": bias, "z64": z64.numpy(), "d32": d32, "bound": 4 * d32 + 1e-6 * z64.abs().max().item()}


def integral_case(c, beta, decode, to_image=None):
    """float64 and float32 torch evaluations of the integral decode on heat_case c: (kcrop64, k2d64, score64, bound_kcrop, bound_k2d)"""
    out = {}
    for dt in (torch.float64, torch.float32):
        z = logits(c["X"], c["Wt"], c["bias"], dt)
        xy, score = decode_integral(z, beta)
        out[dt] = to_outputs(xy, decode, to_image) + (score,)
    k64, a64, s64 = out[torch.float64]
    k32, a32, _ = out[torch.float32]
    H, W = c["X"].shape[1:3]
    dk = (k32.double() - k64).abs().max().item()
    # the floor scales with the coordinate range: max(H, W) pixels times the decode's scale (1 for the heatmap's own coordinates)
    scale = max(H, W) * max(abs(decode[0]), abs(decode[2]), 1.0)
    bk = 4 * dk + 1e-6 * scale
    ba = None
    if to_image is not None:
        ba = 4 * (a32.double() - a64).abs().max().item() + 1e-6 * max(a64.abs().max().item(), 1.0)
    return k64.numpy(), None if a64 is None else a64.numpy(), s64.numpy(), bk, ba


def backward_case(c, beta, decode, to_image, gc, gk, want_dmap=True):
    """torch autograd of sum(gc * kcrop) + sum(gk * k2d) in float64 and float32 (gc / gk numpy [B, J, 2] or None):
    {"dW", "dbias", "dmap"} -> (gradient64 numpy, bound = 4 d32 + 1e-6 max|gradient64|), dmap NHWC"""
    grads = {}
    for dt in (torch.float64, torch.float32):
        X = torch.as_tensor(c["X"]).to(dt).requires_grad_(True)
        Wt = torch.as_tensor(c["Wt"]).to(dt).requires_grad_(True)
        bias = torch.as_tensor(c["bias"]).to(dt).requires_grad_(True)
        z = F.conv2d(X.permute(0, 3, 1, 2), Wt[:, :, None, None], bias)
        xy, _ = decode_integral(z, beta)
        kcrop, k2d = to_outputs(xy, decode, to_image)
        loss = 0
        if gc is not None:
            loss = loss + (torch.as_tensor(gc).to(dt) * kcrop).sum()
        if gk is not None:
            loss = loss + (torch.as_tensor(gk).to(dt) * k2d).sum()
        loss.backward()
        grads[dt] = {"dW": Wt.grad, "dbias": bias.grad, "dmap": X.grad}
    out = {}
    for k, g64 in grads[torch.float64].items():
        d32 = (grads[torch.float32][k].double() - g64).abs().max().item()
        out[k] = (g64.numpy(), 4 * d32 + 1e-6 * g64.abs().max().item())
    return out


def sample_to_image(B, seed=5):
    """B plausible crop -> normalised-image matrices [B, 2, 3] float32 (scale ~ 2 / res_w times a crop zoom, offsets inside [-1, 1])"""
    rng = np.random.default_rng(seed)
    A = np.zeros((B, 2, 3), np.float32)
    zoom = rng.uniform(0.8, 2.5, B)
    A[:, 0, 0] = A[:, 1, 1] = (2.0 / 1000.0) * zoom
    A[:, 0, 1] = rng.uniform(-1e-4, 1e-4, B)
    A[:, 1, 0] = rng.uniform(-1e-4, 1e-4, B)
    A[:, :, 2] = rng.uniform(-0.9, 0.3, (B, 2))
    return A
