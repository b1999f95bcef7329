"""What the native 2-D keypoint head costs (EXPERIMENTS.md R24.1): capf_kp_head_forward in both decodes and capf_kp_head_backward on the
feat0 of an engine, next to capf_backbone_forward of the same handle and to the byte floor of one read of feat0; then forward_detect
against forward on given keypoints.  One process, device events around every call, the calls alternating so that all see the same drift of
the machine; medians with min / max over the repeats.

    python tools/bench_kp_head.py [--configs hrnet_32:fp32:64 hrnet_32:fp32:512 hrnet_48:fp16:256] [--repeats 20] [--warmup 3]   (needs the MI355X)
    python tools/bench_kp_head.py --pair [--configs hrnet_32:fp32:32 hrnet_32:fp32:256 hrnet_48:fp16:128]     (EXPERIMENTS.md R28.1)
    python tools/bench_kp_head.py --loss [--configs hrnet_32:fp32:64 hrnet_32:fp32:512 hrnet_48:fp16:256]     (EXPERIMENTS.md R33.1)

--pair: the flip-test pair.  The batch of a config counts SOURCE frames; feat0 holds the 2 * Bsrc frames [orig | mirrored] of one backbone
pass.  capf_kp_head_forward_pair against capf_kp_head_forward on the SAME map (the same bytes read, the same FMAs, half the (frame, joint)
items), then forward_detect_flip_test against the route without it: detect + preprocess_points + forward_flip_test.

--loss: heatmap supervision.  capf_kp_heatmap_loss (mean and OHKM; the loss alone, with dweight / dbias, with dmap on an fp32 map) against
capf_kp_head_backward re-timed on the SAME map in the same session (fp32 maps: the backward takes no 16-bit map; there the comparison point is
capf_kp_head_forward), with the one-read floor at 8 TB/s beside --hbm-gbs's.

The floor is feat0's bytes over --hbm-gbs (default 4000 GB/s, roughly what a streaming read reaches on an MI355X); the backward reads the
map three times (statistics, dz, the dW products) and, with dmap, writes it once.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(runs, repeats, warmup):
    import torch
    times = {k: [] for k in runs}
    for it in range(warmup + repeats):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}


def pair_row(args, spec, model, eng, img, A, s):
    import torch
    from capf import lib as capf
    B = img.shape[0]
    images2 = torch.stack([img, torch.flip(img, [2])]).contiguous()
    pair = images2.view(2 * B, *img.shape[1:])
    eng.backbone_forward(pair, s)
    feat0 = eng.tensor_view("feat0", 2 * B)
    fl = model.keypoint_head.final_layer
    w, b = fl.weight.detach().reshape(17, -1).contiguous(), fl.bias.detach()
    dec, A2 = (4.0, 0.0, 4.0, 0.0), torch.cat([A, A]).contiguous()

    def route_today():
        kcrop, _, k2d = model.detect(img, A)
        _, k2d2, kcrop2 = capf.preprocess_points(None, k2d, kcrop, mode=2)
        return model.forward_flip_test(images2, k2d2, kcrop2)

    runs = {
        "backbone_forward_2B": lambda: eng.backbone_forward(pair, s),
        "single_2B_argmax": lambda: capf.kp_head_forward(feat0, w, b, capf.KP_ARGMAX, 1.0, dec, A2),
        "pair_argmax": lambda: capf.kp_head_forward_pair(feat0, w, b, capf.KP_ARGMAX, 1.0, None, True, dec, A),
        "single_2B_integral": lambda: capf.kp_head_forward(feat0, w, b, capf.KP_INTEGRAL, 2.0, dec, A2),
        "pair_integral": lambda: capf.kp_head_forward_pair(feat0, w, b, capf.KP_INTEGRAL, 2.0, None, True, dec, A),
    }
    with torch.no_grad():
        runs["detect+preprocess_points+forward_flip_test"] = route_today
        runs["forward_detect_flip_test"] = lambda: model.forward_detect_flip_test(images2, A)
        row = {"config": spec, "pair": True, "feat0": list(feat0.shape), "feat0_MB": round(feat0.numel() * feat0.element_size() / 1e6, 2),
               "one_read_floor_ms": round(feat0.numel() * feat0.element_size() / (args.hbm_gbs * 1e9) * 1e3, 4), "repeats": args.repeats}
        row.update(timed(runs, args.repeats, args.warmup))
    for mode in ("argmax", "integral"):
        row[f"pair_over_single_{mode}"] = round(row[f"pair_{mode}"]["median_ms"] / row[f"single_2B_{mode}"]["median_ms"], 3)
    row["flip_test_over_route_today"] = round(row["forward_detect_flip_test"]["median_ms"] / row["detect+preprocess_points+forward_flip_test"]["median_ms"], 3)
    return row


def loss_row(args, spec, model, eng, img, A, s, dtype):
    import torch
    from capf import lib as capf
    B = img.shape[0]
    eng.backbone_forward(img, s)
    feat0 = eng.tensor_view("feat0", B)
    fl = model.keypoint_head.final_layer
    w, b = fl.weight.detach().reshape(17, -1).contiguous(), fl.bias.detach()
    dec = (4.0, 0.0, 4.0, 0.0)
    g = torch.Generator().manual_seed(3)
    gt = (torch.rand(B, 17, 2, generator=g) * 256).cuda()
    tw = torch.ones(B, 17).cuda()
    loss = lambda red, **kw: (lambda: capf.kp_heatmap_loss(feat0, w, b, gt, tw, dec, 2.0, red, 8, 0.5, **kw))
    runs = {
        "head_integral": lambda: capf.kp_head_forward(feat0, w, b, capf.KP_INTEGRAL, 2.0, dec, A),
        "loss_mean_alone": loss("mean", want_grads=False),
        "loss_mean_dW": loss("mean"),
        "loss_ohkm_alone": loss("ohkm", want_grads=False),
        "loss_ohkm_dW": loss("ohkm"),
    }
    if dtype == "fp32":
        g1, g2 = torch.randn(B, 17, 2, device="cuda"), torch.randn(B, 17, 2, device="cuda")
        dmap = torch.zeros_like(feat0)
        runs["loss_mean_dW_dmap"] = loss("mean", dmap_accumulate_into=dmap)
        runs["loss_ohkm_dW_dmap"] = loss("ohkm", dmap_accumulate_into=dmap)
        runs["head_backward_dW"] = lambda: capf.kp_head_backward(feat0, w, b, g1, g2, 2.0, dec, A)
        runs["head_backward_dW_dmap"] = lambda: capf.kp_head_backward(feat0, w, b, g1, g2, 2.0, dec, A, dmap=dmap)
    nbytes = feat0.numel() * feat0.element_size()
    row = {"config": spec, "loss": True, "feat0": list(feat0.shape), "feat0_MB": round(nbytes / 1e6, 2),
           "one_read_floor_ms": round(nbytes / (args.hbm_gbs * 1e9) * 1e3, 4), "one_read_floor_8TBs_ms": round(nbytes / 8e12 * 1e3, 4),
           "repeats": args.repeats}
    with torch.no_grad():
        row.update(timed(runs, args.repeats, args.warmup))
    base = "head_backward_dW" if dtype == "fp32" else "head_integral"
    row["compared_with"] = base
    for k in [k for k in runs if k.startswith("loss_")]:
        ref = "head_backward_dW_dmap" if k.endswith("_dmap") else base
        row[k + "_over_" + ref] = round(row[k]["median_ms"] / row[ref]["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=None, help="backbone:dtype:batch (source frames with --pair)")
    ap.add_argument("--pair", action="store_true", help="the flip-test pair: capf_kp_head_forward_pair / forward_detect_flip_test")
    ap.add_argument("--loss", action="store_true", help="heatmap supervision: capf_kp_heatmap_loss against capf_kp_head_backward on the same map")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0)
    args = ap.parse_args()
    if args.configs is None:
        args.configs = ["hrnet_32:fp32:32", "hrnet_32:fp32:256", "hrnet_48:fp16:128"] if args.pair else ["hrnet_32:fp32:64", "hrnet_32:fp32:512", "hrnet_48:fp16:256"]
    sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_kp_head.py needs the MI355X"
    from capf import lib as capf
    from capf import synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    for spec in args.configs:
        backbone, dtype, B = spec.split(":")
        B = int(B)
        cfg = backbone_preset(copy.deepcopy(config), backbone)
        cfg.model.backbone.fix_weights = True
        model = CA_PF(cfg, compute_dtype=dtype, keypoint_head="integral", keypoint_beta=2.0)
        synth.load_synthetic(model, seed=1, bn_mode="random")
        model = model.cuda().eval()
        img, k2d, kc = (t.cuda() for t in synth.synth_inputs(B, 256, 256, seed=2, crop_range=(192, 256)))
        A = torch.from_numpy(np.stack([capf.crop_to_image_matrix((500.0, 500.0), (1.5, 1.5), (256, 256), 1000, 1000)] * B).astype(np.float32)).cuda()
        eng = model.engine_for(img)
        s = torch.cuda.current_stream().cuda_stream
        if args.pair:
            print(json.dumps(pair_row(args, spec, model, eng, img, A, s)), flush=True)
            for e in model._engines.values():
                e.close()
            model._engines.clear()
            continue
        if args.loss:
            print(json.dumps(loss_row(args, spec, model, eng, img, A, s, dtype)), flush=True)
            for e in model._engines.values():
                e.close()
            model._engines.clear()
            continue
        eng.backbone_forward(img, s)
        feat0 = eng.tensor_view("feat0", B)
        fl = model.keypoint_head.final_layer
        w, b = fl.weight.detach().reshape(17, -1).contiguous(), fl.bias.detach()
        dec = (4.0, 0.0, 4.0, 0.0)
        runs = {
            "backbone_forward": lambda: eng.backbone_forward(img, s),
            "head_argmax": lambda: capf.kp_head_forward(feat0, w, b, capf.KP_ARGMAX, 1.0, dec, A),
            "head_integral": lambda: capf.kp_head_forward(feat0, w, b, capf.KP_INTEGRAL, 2.0, dec, A),
        }
        if dtype == "fp32":
            g1, g2 = torch.randn(B, 17, 2, device="cuda"), torch.randn(B, 17, 2, device="cuda")
            dmap = torch.zeros_like(feat0)
            runs["head_backward_dW"] = lambda: capf.kp_head_backward(feat0, w, b, g1, g2, 2.0, dec, A)
            runs["head_backward_dW_dmap"] = lambda: capf.kp_head_backward(feat0, w, b, g1, g2, 2.0, dec, A, dmap=dmap)
        with torch.no_grad():
            runs["forward_given_keypoints"] = lambda: model(img, k2d, kc.clone())
            runs["forward_detect"] = lambda: model.forward_detect(img, A)
            row = {"config": spec, "feat0": list(feat0.shape), "feat0_MB": round(feat0.numel() * feat0.element_size() / 1e6, 2),
                   "one_read_floor_ms": round(feat0.numel() * feat0.element_size() / (args.hbm_gbs * 1e9) * 1e3, 4), "repeats": args.repeats}
            row.update(timed(runs, args.repeats, args.warmup))
        print(json.dumps(row), flush=True)
        for e in model._engines.values():
            e.close()
        model._engines.clear()


if __name__ == "__main__":
    main()
