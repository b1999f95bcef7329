"""Cost of batch-statistics BatchNorm in the frozen backbone (EXPERIMENTS R22.1): one training step of the MPI-INF-3DHP variant
(VolumetricTriangulationNet, HRNet-32 / embed 64, depth 4, 256 x 256 crops; run_3dhp.py:60-101: forward with DropPath 0.2, mpjpe_cal,
backward, FusedAdamW) with the backbone on the running statistics (backbone.eval(): capf_forward_train) and on batch statistics
(backbone_bn="batch", backbone in train mode: capf_backbone_forward_bn + capf_lifter_forward_train), at batch 160 (run_3dhp.py's default)
and 64.  One process, one device; the two routes ALTERNATE pair by pair (HIP events around --steps steps each), and the result is the median
and the spread over --pairs pairs.  Launches per backbone forward and the share of the statistics / apply launches come from one profiled
forward of each route (torch.profiler, outside the timed region).  Synthetic weights and inputs.  One JSON line per batch.
    python tools/bench_bn_train.py [--batches 160,64] [--steps 20] [--warmup 2] [--pairs 5]"""
import argparse
import contextlib
import copy
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))

import torch

BN_KERNELS = ("bn_stats_slab_kernel", "bn_stats_final_kernel", "bn_apply_kernel")


def model_for(backbone_bn):
    from capf import synth
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(mpi_preset(copy.deepcopy(config), "hrnet_32"), backbone_bn=backbone_bn)
    synth.load_synthetic(m, seed=3, bn_mode="random")
    m = m.cuda()
    m.train()
    if backbone_bn == "running":
        m.backbone.eval()
    return m


def stepper(model, B, size):
    from capf import synth
    from capf.optim import FusedAdamW, flatten_
    img, k2d, kc, gt = synth.synth_inputs(B, size, size, seed=4, crop_range=(192, 256), with_gt=True)
    img, k2d, kc0, target = img.cuda(), k2d.cuda(), kc.cuda(), gt.cuda().clone()
    target[:, :, 14] = 0
    kc_work = kc0.clone()
    opt = FusedAdamW(flatten_(model.volume_net), lr=6.4e-4, weight_decay=0.1)
    model.flat_grad_only = True

    def step():
        kc_work.copy_(kc0)
        out, _ = model(img, k2d, kc_work)
        out = out.permute(0, 2, 3, 4, 1).contiguous().view(B, -1, 17, 3)
        loss = torch.mean(torch.norm(out - target, dim=len(target.shape) - 1))
        loss.backward()
        opt.step(model.last_flat_grad)
        model.lifter_params_changed()

    def backbone_only():
        eng = model.engine_for(img)
        stream = torch.cuda.current_stream().cuda_stream
        if model._bn_batch_active():
            eng.backbone_forward_bn(img, stream)
        else:
            eng.backbone_forward(img, stream)

    return step, backbone_only


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def launches(fn):
    """(kernel launches, their summed device time in us, {bn kernel: (launches, us)}) of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n, us, bn = 0, 0.0, {k: [0, 0.0] for k in BN_KERNELS}
    for ev in prof.events():
        if getattr(ev, "device_type", None) is None or "cuda" not in str(ev.device_type).lower():
            continue
        if "memcpy" in ev.name.lower() or "memset" in ev.name.lower():
            continue
        dur = float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
        n += 1
        us += dur
        for k in BN_KERNELS:
            if k in ev.name:
                bn[k][0] += 1
                bn[k][1] += dur
    return n, us, bn


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def bench(B, size, steps, warmup, pairs):
    torch.manual_seed(5)
    run, bn = model_for("running"), model_for("batch")
    s_run, bb_run = stepper(run, B, size)
    s_bn, bb_bn = stepper(bn, B, size)
    for _ in range(warmup):
        s_run(); s_bn()
    torch.cuda.synchronize()
    t_run, t_bn, f_run, f_bn = [], [], [], []
    for _ in range(pairs):
        t_run.append(timed(s_run, steps)); t_bn.append(timed(s_bn, steps))
        f_run.append(timed(bb_run, steps)); f_bn.append(timed(bb_bn, steps))
    rec = {"what": "training step, running vs batch statistics", "model": "mpi_hrnet_32", "batch": B, "crop": f"{size}x{size}",
           "step_ms_running": spread(t_run), "step_ms_batch": spread(t_bn),
           "step_ratio": round(statistics.median(t_bn) / statistics.median(t_run), 3),
           "backbone_ms_running": spread(f_run), "backbone_ms_batch": spread(f_bn), "pairs": pairs, "steps": steps, "warmup": warmup}
    try:
        n0, us0, _ = launches(bb_run)
        n1, us1, k = launches(bb_bn)
        rec.update({"backbone_launches_running": n0, "backbone_launches_batch": n1,
                    "bn_launches": {name: v[0] for name, v in k.items()},
                    "bn_share_of_device_time": {name: round(v[1] / us1, 4) if us1 > 0 else None for name, v in k.items()},
                    "backbone_device_us_running": round(us0, 1), "backbone_device_us_batch": round(us1, 1)})
    except Exception as e:                                 # (no profiler on this box: the timings stand on their own)
        rec["profile_error"] = repr(e)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="160,64")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=5)
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for B in [int(b) for b in a.batches.split(",")]:
        print(json.dumps(bench(B, a.size, a.steps, a.warmup, a.pairs)), flush=True)


if __name__ == "__main__":
    main()
