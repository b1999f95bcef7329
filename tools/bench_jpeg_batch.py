"""Batched JPEG decode throughput (EXPERIMENTS R7.2): frame-sized (1000 x 1002, 4:2:0, noise sigma 6) JPEGs made at run time by Pillow,
at two qualities and batches 1 / 16 / 64, timed three ways:
  host     one capf_jpeg_decode per frame (host Huffman walk + upload + GPU pixels, waits per frame), as load_and_crop_batch's default;
  walk     the host Huffman walk alone (capf_jpeg_coefficients) on --threads threads, no GPU;
  device   one capf_jpeg_decode_batch for the batch (staging + upload + every kernel), synchronised at the end.
--subseq L1,L2,... times the device path at those subsequence lengths (0 = the default; the default's measurement).  One JSON line
per result.
    python tools/bench_jpeg_batch.py [--reps 10] [--threads 16] [--subseq 0] [--out file.json]
Under rocprofv3 --kernel-trace --stats (per-stage kernel time): python tools/bench_jpeg_batch.py --reps 3 --only-device"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "contextaware-poseformer_amd"))


def frames(n, quality, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = 1002, 1000
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(x / 37.0) * np.cos(y / 51.0), 128 + 90 * np.cos(x / 25.0 + y / 19.0), (x + 2 * y) % 256], -1)
    out = []
    for i in range(n):
        img = np.clip(np.roll(base, 13 * i, axis=1) + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=2)
        out.append(buf.getvalue())
    return out


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--subseq", default="0")
    ap.add_argument("--only-device", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from capf import lib as capf
    results = []

    def emit(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    for q in (75, 90):
        pool = frames(64, q)
        kb = float(np.mean([len(d) for d in pool])) / 1024
        for B in (1, 16, 64):
            datas = pool[:B]
            if not a.only_device:
                def host():
                    for d in datas:
                        capf.jpeg_decode(d)
                    torch.cuda.synchronize()
                emit(path="host", quality=q, batch=B, file_kb=round(kb, 1), ms=round(timed(host, a.reps), 3))
                with ThreadPoolExecutor(a.threads) as ex:
                    emit(path="walk", quality=q, batch=B, threads=a.threads, file_kb=round(kb, 1),
                         ms=round(timed(lambda: list(ex.map(capf.jpeg_coefficients, datas)), a.reps), 3))
            for L in [int(v) for v in a.subseq.split(",")]:
                def dev():
                    _, st = capf.jpeg_decode_batch(datas, "cuda", L)
                    torch.cuda.synchronize()
                    return st
                st = dev()
                assert not st.any().item(), st
                emit(path="device", quality=q, batch=B, subseq=L, file_kb=round(kb, 1), ms=round(timed(dev, a.reps), 3))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
