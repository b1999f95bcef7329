"""The image front end, measured (EXPERIMENTS R8): files -> crops on load_and_crop_batch's two device routes, and files -> crops ->
capf_preprocess -> capf_forward end to end.  Frames are tools/bench_jpeg_batch.py's (1000 x 1002, 4:2:0, made at run time by Pillow) at quality
75 and 90; crops are Human3.6M-like 3:4 boxes to 192 x 256 covering about 1/6, 1/4 and all of the frame.

  --part decode   batches 1 / 16 / 64: ms per batch, upload included, synchronised at the end, of
                    device       capf_jpeg_decode_batch (full frames) + capf_warp_affine
                    device_crop  capf_jpeg_decode_crop_batch (only the MCUs a crop reads)
                  run ALTERNATELY, --pairs times (at least 5), the median of each and of the per-pair ratio; and the device bytes each route
                  allocates (scratch + frames + crops).
  --part e2e      HRNet-32, fp32, batch 64 (bench.py's configuration 1 at the crop's 256 x 192): frames/s of files -> crops -> capf_preprocess
                  -> capf_forward on both routes, alternately, and of the forward alone on crops already on the device.
  --part profile  --reps calls of ONE route (--route) at one quality / batch / box, for `rocprofv3 --kernel-trace --stats -- python ...`.
One JSON line per result; --out collects them in a file (appending to what is there, so the parts can run as separate, time-limited steps).
    python tools/bench_frontend.py --part decode --out profiles/r08_frontend.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_jpeg_batch import frames  # noqa: E402

W, H, OUT = 1000, 1002, (192, 256)
SHARES = {"sixth": 1.0 / 6, "quarter": 1.0 / 4, "whole": None}


def boxes(n, share, seed=0):
    """n (center, scale) pairs of 3:4 boxes covering `share` of the frame, inside it, at jittered places; None: a box holding the frame"""
    rng = np.random.default_rng(seed)
    if share is None:
        return [((W / 2.0, H / 2.0), (W / 200.0, W / 150.0))] * n
    w = float(np.sqrt(0.75 * share * W * H))
    h = w * 4.0 / 3.0
    return [((float(rng.uniform(w / 2, W - w / 2)), float(rng.uniform(h / 2, H - h / 2))), (w / 200.0, h / 200.0)) for _ in range(n)]


def matrices(bx):
    from capf import lib as capf
    return np.stack([capf.affine_from_center_scale(c, s, OUT) for c, s in bx])


def routes(datas, mats):
    import torch
    from capf import lib as capf

    def device():
        fr, st = capf.jpeg_decode_batch(datas, "cuda")
        return capf.warp_affine(fr, mats, OUT), st

    def device_crop():
        return capf.jpeg_decode_crop_batch(datas, mats, OUT, "cuda")

    for f in (device, device_crop):                    # warm-up, and the routes agree
        crops, st = f()
        torch.cuda.synchronize()
        assert not st.any().item(), st
    assert torch.equal(device()[0], device_crop()[0])
    return {"device": device, "device_crop": device_crop}


def alternate(fns, pairs, sync):
    """fns: name -> callable; runs them in turn `pairs` times -> name -> list of seconds"""
    ts = {k: [] for k in fns}
    for _ in range(pairs):
        for k, f in fns.items():
            sync()
            t0 = time.perf_counter()
            f()
            sync()
            ts[k].append(time.perf_counter() - t0)
    return ts


def part_decode(a, emit):
    import torch
    from capf import lib as capf
    for q in (75, 90):
        pool = frames(64, q)
        for B in (1, 16, 64):
            datas = pool[:B]
            for name, share in SHARES.items():
                mats = matrices(boxes(B, share, seed=B))
                fns = routes(datas, mats)
                ts = alternate(fns, a.pairs, torch.cuda.synchronize)
                ms = {k: float(np.median(v)) * 1e3 for k, v in ts.items()}
                ratio = float(np.median(np.array(ts["device_crop"]) / np.array(ts["device"])))
                _, full = capf.jpeg_batch_info(datas)
                _, rows, crop = capf.jpeg_crop_batch_info(datas, mats, OUT)
                crops_b = B * OUT[0] * OUT[1] * 3
                kept = float(np.mean([(r["mcu_rect"][2] - r["mcu_rect"][0]) * (r["mcu_rect"][3] - r["mcu_rect"][1]) for r in rows])) / (63 * 63)
                emit(part="decode", quality=q, batch=B, box=name, pairs=a.pairs, mcus_kept=round(kept, 3),
                     ms_device=round(ms["device"], 3), ms_device_crop=round(ms["device_crop"], 3), crop_over_device=round(ratio, 3),
                     bytes_device=full + B * W * H * 3 + crops_b, bytes_device_crop=crop + crops_b)


def part_e2e(a, emit):
    import contextlib
    import copy
    import io
    import torch
    from capf import lib as capf, synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    B = 64
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        model = CA_PF(cfg, compute_dtype="fp32").eval()
    synth.load_synthetic(model, seed=1, bn_mode="random")
    model = model.cuda()
    _, k2d, kc = synth.synth_inputs(B, OUT[1], OUT[0], seed=101)
    k2d, kc = k2d.cuda(), kc.cuda()

    def forward(crops):
        img, _, k, c = capf.preprocess(crops, None, k2d, kc, "hrnet_32")
        return model(img, k, c)

    for q in (75, 90):
        datas = frames(B, q)
        for name in ("quarter", "sixth"):
            mats = matrices(boxes(B, SHARES[name], seed=B))
            fns = routes(datas, mats)
            ready = fns["device"]()[0]
            with torch.no_grad():
                steps = {"device": lambda: forward(fns["device"]()[0]), "device_crop": lambda: forward(fns["device_crop"]()[0]),
                         "forward_alone": lambda: forward(ready)}
                for f in steps.values():
                    f()
                ts = alternate(steps, a.pairs, torch.cuda.synchronize)
            fps = {k: B / float(np.median(v)) for k, v in ts.items()}
            emit(part="e2e", quality=q, batch=B, box=name, pairs=a.pairs, model="hrnet_32 fp32 256x192",
                 frames_per_s_device=round(fps["device"], 1), frames_per_s_device_crop=round(fps["device_crop"], 1),
                 frames_per_s_forward_alone=round(fps["forward_alone"], 1),
                 ms_device=round(B / fps["device"] * 1e3, 3), ms_device_crop=round(B / fps["device_crop"] * 1e3, 3),
                 ms_forward_alone=round(B / fps["forward_alone"] * 1e3, 3))


def part_profile(a, emit):
    import torch
    datas = frames(a.batch, a.quality)
    fn = routes(datas, matrices(boxes(a.batch, SHARES[a.box], seed=a.batch)))[a.route]
    for _ in range(a.reps):
        fn()
    torch.cuda.synchronize()
    emit(part="profile", route=a.route, quality=a.quality, batch=a.batch, box=a.box, calls=a.reps + (3 if a.route == "device" else 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["decode", "e2e", "profile"])
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--route", default="device_crop", choices=["device", "device_crop"])
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--box", default="quarter", choices=sorted(SHARES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.pairs < 5:
        ap.error("--pairs must be at least 5")
    results = []

    def emit(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    {"decode": part_decode, "e2e": part_e2e, "profile": part_profile}[a.part](a, emit)
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        with open(a.out, "w") as f:
            json.dump(old + results, f, indent=1)


if __name__ == "__main__":
    main()
