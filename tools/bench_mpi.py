"""MPI-INF-3DHP numbers (EXPERIMENTS R7.3): one training step of VolumetricTriangulationNet (run_3dhp.py:60-101: forward with DropPath
0.2, mpjpe_cal against a target with joint 14 zeroed, backward, flatten_ + FusedAdamW(weight_decay = 0.1)) at batch 160 for HRNet-32 /
embed 64 and HRNet-48 / embed 96, depth 4, 256 x 192 crops, next to the H36M model's step at the same batch and crop; and one
evaluate() over 2929 poses (the 3DHP test set's size: three capf_pck_counts calls + the host tables).  Synthetic weights and inputs.
HIP events around --steps steps after --warmup, median of --reps repetitions.  One JSON line per result.
    python tools/bench_mpi.py [--batch 160] [--steps 10] [--warmup 3] [--reps 3]"""
import argparse
import contextlib
import copy
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "contextaware-poseformer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
import torch


def model_for(name):
    from capf import synth
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    with contextlib.redirect_stdout(io.StringIO()):
        if name.startswith("mpi_"):
            cfg = mpi_preset(copy.deepcopy(config), name[4:])
            m = VolumetricTriangulationNet(cfg)
        else:
            cfg = backbone_preset(copy.deepcopy(config), name)
            cfg.model.backbone.fix_weights = True
            m = CA_PF(cfg)
    synth.load_synthetic(m, seed=3, bn_mode="random")
    m = m.cuda()
    m.train(); m.backbone.eval(); m.volume_net.train()
    return m


def time_training(name, B, steps, warmup, reps):
    from capf import synth
    from capf.optim import FusedAdamW, flatten_
    model = model_for(name)
    mpi = name.startswith("mpi_")
    img, k2d, kc, gt = synth.synth_inputs(B, 256, 192, seed=4, crop_range=(192, 256), with_gt=True)
    img, k2d, kc0, gt = img.cuda(), k2d.cuda(), kc.cuda(), gt.cuda()
    target = gt.clone()
    if mpi:
        target[:, :, 14] = 0
    kc_work = kc0.clone()
    opt = FusedAdamW(flatten_(model.volume_net), lr=6.4e-4, weight_decay=0.1)
    model.flat_grad_only = True

    def step():
        kc_work.copy_(kc0)
        if mpi:
            out, _ = model(img, k2d, kc_work)
            out = out.permute(0, 2, 3, 4, 1).contiguous().view(B, -1, 17, 3)
        else:
            out = model(img, k2d, kc_work)
        loss = torch.mean(torch.norm(out - target, dim=len(target.shape) - 1))
        loss.backward()
        opt.step(model.last_flat_grad)
        model.lifter_params_changed()

    torch.manual_seed(5)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    med = statistics.median(ms)
    return {"what": "training step", "model": name, "batch": B, "crop": "256x192", "ms_per_step": round(med, 3),
            "us_per_frame": round(med * 1e3 / B, 2), "reps_ms": [round(x, 3) for x in ms], "steps": steps, "warmup": warmup}


def time_metrics(n, reps):
    import mpi_eval_numpy as ref
    from mvn.datasets import mpi_inf_3dhp as mpi
    pred, gt, seq, act = ref.synthetic_set(n, seed=6)
    p, g = torch.as_tensor(pred).cuda(), torch.as_tensor(gt).cuda()
    mpi.evaluate(p, g, seq, act, to_mm=1000.0)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mpi.evaluate(p, g, seq, act, to_mm=1000.0)
        ts.append((time.perf_counter() - t0) * 1e3)
    from capf import lib as capf_lib
    s = torch.as_tensor(act - 1, dtype=torch.int32).cuda()
    capf_lib.pck_counts(p, g, 14, 1000.0, s, 7)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        capf_lib.pck_counts(p, g, 14, 1000.0, s, 7)
    b.record()
    torch.cuda.synchronize()
    return {"what": "3dhp evaluate", "poses": n, "evaluate_ms_host_wall": round(statistics.median(ts), 3),
            "pck_counts_ms_7_segments": round(a.elapsed_time(b) / 20, 4), "reps": reps,
            "note": "evaluate = three capf_pck_counts launches (sequences, activities, all) + device->host copies + fp64 tables on the host"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=160)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--poses", type=int, default=2929)
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for name in ("mpi_hrnet_32", "mpi_hrnet_48", "hrnet_32", "hrnet_48"):
        print(json.dumps(time_training(name, a.batch, a.steps, a.warmup, a.reps)), flush=True)
    print(json.dumps(time_metrics(a.poses, 10)), flush=True)


if __name__ == "__main__":
    main()
