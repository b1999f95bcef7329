"""What CPN's own keypoint detector costs (EXPERIMENTS.md R29.1), at BASELINE.json config 4's geometry by default: bf16, 384 x 288, batch 128.

  (a) capf_backbone_forward of a CAPF_PLAN_CPN_PREDICT handle against the unflagged handle of the same weights, the calls alternating; the
      head's launches one by one -- the concat and the five convs -- from capf_forward_profile (an event pair around every op, in program
      order on one stream), medians over the repeats, with the kernel the op table names for each;
  (b) capf_cpn_decode alone on the "heat" tensor a backbone pass left;
  (c) CA_PF(keypoint_head="cpn").forward_detect against forward on precomputed keypoints (of the default module, and of the flagged one,
      whose backbone pass runs the head whether or not anybody decodes it).

One process, device events around every call, medians with min / max over the repeats (tools/bench_kp_head.py's scheme).

--pair: CPN's test-time flip (EXPERIMENTS.md R30.1), per config dtype:HxW:Bsrc (default fp32:256x192:32 bf16:256x192:64):
  (a) capf_cpn_decode_pair at Bsrc against capf_cpn_decode on the SAME 2 * Bsrc-frame "heat" (twice the (frame, joint) items, the same map
      bytes) and on its first Bsrc frames (the same items, half the map bytes);
  (b) CA_PF.forward_detect_cpn_flip against the route available without it: a backbone pass over [orig | mirrored], the fold of the two
      heatmaps in torch, capf_cpn_decode, preprocess_points(mode=2) and forward_flip_test (a second backbone pass over the pair); the two
      routes' joints are compared bit for bit once.

    python tools/bench_cpn_detect.py [--configs bf16:384x288:128 fp32:256x192:64] [--repeats 20] [--warmup 3]      (needs the MI355X)
    python tools/bench_cpn_detect.py --pair [--configs fp32:256x192:32 bf16:256x192:64]
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


def pair_mode(args):
    import numpy as np
    import torch
    from capf import lib as capf
    from capf import synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    swap = list(capf.H36M_SWAP)
    for spec in args.configs:
        dtype, hw, B = spec.split(":")
        H, W = (int(v) for v in hw.split("x"))
        B = int(B)
        cfg = backbone_preset(copy.deepcopy(config), "cpn")
        cfg.model.backbone.fix_weights = True
        model = CA_PF(cfg, compute_dtype=dtype, keypoint_head="cpn")
        synth.load_synthetic(model, seed=1, bn_mode="random")
        model = model.cuda().eval()
        img = synth.synth_inputs(B, H, W, seed=2, crop_range=(W, H))[0].cuda()
        A = torch.from_numpy(np.stack([capf.crop_to_image_matrix((500.0, 500.0), (1.5, 1.5), (W, H), 1000, 1000)] * B).astype(np.float32)).cuda()
        s = torch.cuda.current_stream().cuda_stream
        eng = model.engine_for(img)
        pair = torch.cat([img, torch.flip(img, [2])])
        with torch.no_grad():
            eng.backbone_forward(pair, s)
            heat2 = eng.tensor_view("heat", 2 * B).clone()
            half = heat2[:B].contiguous()
            sx, sy = W / heat2.shape[2], H / heat2.shape[1]
            dec = (sx, sx / 2, sy, sy / 2)

            def without_the_pair_entry():
                eng.backbone_forward(pair, s)
                z = eng.tensor_view("heat", 2 * B).float()
                zf = (0.5 * (z[:B, :, :, :17] + z[B:].flip(2)[..., swap])).contiguous()
                kcrop, _, k2d, _ = capf.cpn_decode(zf, 17, dec, A)
                _, k2d2, kcrop2 = capf.preprocess_points(None, k2d, kcrop, mode=2)
                return model.forward_flip_test(pair.view(2, B, H, W, 3), k2d2, kcrop2)

            same = bool(torch.equal(without_the_pair_entry(), model.forward_detect_cpn_flip(img, A)[0]))
            runs = {
                "cpn_decode_pair_Bsrc": lambda: capf.cpn_decode_pair(heat2, 17, None, dec, A),
                "cpn_decode_2Bsrc_frames": lambda: capf.cpn_decode(heat2, 17, dec, None),
                "cpn_decode_Bsrc_frames": lambda: capf.cpn_decode(half, 17, dec, A),
                "backbone_forward_2Bsrc": lambda: eng.backbone_forward(pair, s),
                "forward_detect_cpn_flip": lambda: model.forward_detect_cpn_flip(img, A),
                "fold_in_torch_route": without_the_pair_entry,
            }
            row = {"config": spec, "mode": "pair", "Bsrc": B, "heat2": list(heat2.shape), "heat2_MB": round(heat2.numel() * heat2.element_size() / 1e6, 2),
                   "workgroups_pair": B * 17, "repeats": args.repeats, "routes_bit_equal": same}
            row.update(timed(runs, args.repeats, args.warmup))
        ms = lambda k: row[k]["median_ms"]
        row["pair_over_single_2Bsrc"] = round(ms("cpn_decode_pair_Bsrc") / ms("cpn_decode_2Bsrc_frames"), 3)
        row["pair_over_single_Bsrc"] = round(ms("cpn_decode_pair_Bsrc") / ms("cpn_decode_Bsrc_frames"), 3)
        row["entry_saves_ms"] = round(ms("fold_in_torch_route") - ms("forward_detect_cpn_flip"), 4)
        print(json.dumps(row), flush=True)
        for e in model._engines.values():
            e.close()
        model._engines.clear()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=None, help="dtype:HxW:batch (--pair: dtype:HxW:Bsrc)")
    ap.add_argument("--pair", action="store_true", help="CPN's test-time flip: capf_cpn_decode_pair / forward_detect_cpn_flip")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_cpn_detect.py needs the MI355X"
    if args.configs is None:
        args.configs = ["fp32:256x192:32", "bf16:256x192:64"] if args.pair else ["bf16:384x288:128"]
    if args.pair:
        return pair_mode(args)
    from capf import lib as capf
    from capf import synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    for spec in args.configs:
        dtype, hw, B = spec.split(":")
        H, W = (int(v) for v in hw.split("x"))
        B = int(B)
        cfg = backbone_preset(copy.deepcopy(config), "cpn")
        cfg.model.backbone.fix_weights = True
        models = {}
        for name, head in (("plain", None), ("cpn_head", "cpn")):
            m = CA_PF(cfg, compute_dtype=dtype, keypoint_head=head)
            synth.load_synthetic(m, seed=1, bn_mode="random")
            models[name] = m.cuda().eval()
        img, k2d, kc = (t.cuda() for t in synth.synth_inputs(B, H, W, seed=2, crop_range=(W, H)))
        A = torch.from_numpy(np.stack([capf.crop_to_image_matrix((500.0, 500.0), (1.5, 1.5), (W, H), 1000, 1000)] * B).astype(np.float32)).cuda()
        s = torch.cuda.current_stream().cuda_stream
        plain, flagged = models["plain"].engine_for(img), models["cpn_head"].engine_for(img)
        flagged.backbone_forward(img, s)
        heat = flagged.tensor_view("heat", B)
        sx, sy = W / heat.shape[2], H / heat.shape[1]
        dec = (sx, sx / 2, sy, sy / 2)
        out = torch.empty(B, 1, 17, 3, device="cuda")
        with torch.no_grad():
            runs = {
                "backbone_forward": lambda: plain.backbone_forward(img, s),
                "backbone_forward_cpn_predict": lambda: flagged.backbone_forward(img, s),
                "cpn_decode": lambda: capf.cpn_decode(heat, 17, dec, A),
                "forward_given_keypoints": lambda: models["plain"](img, k2d, kc.clone()),
                "forward_given_keypoints_cpn_predict": lambda: models["cpn_head"](img, k2d, kc.clone()),
                "forward_detect": lambda: models["cpn_head"].forward_detect(img, A),
            }
            row = {"config": spec, "heat": list(heat.shape), "heat_MB": round(heat.numel() * heat.element_size() / 1e6, 2), "repeats": args.repeats,
                   "workspace_MB": {"plain": round(plain.workspace_bytes(B) / 1e6, 1), "cpn_predict": round(flagged.workspace_bytes(B) / 1e6, 1)}}
            row.update(timed(runs, args.repeats, args.warmup))
            # the head's launches one by one (program order, one stream: no overlap between the shortcut's lane and conv1 / conv2)
            table = flagged.op_table(B)
            bytes_ = flagged.op_bytes(B)
            head = [i for i, (n, _, _) in enumerate(table) if "final_predict" in n]
            per_op = {i: [] for i in head}
            for it in range(args.warmup + args.repeats):
                ms = flagged.forward_profile(img, k2d, kc.clone(), out, s)
                if it >= args.warmup:
                    for i in head:
                        per_op[i].append(ms[i])
            row["head_ops"] = [{"op": table[i][0].split("final_predict.")[1], "kernel": table[i][1], "median_ms": round(statistics.median(per_op[i]), 4),
                                "GFLOP": round(table[i][2] / 1e9, 2), "MB": round(bytes_[i] / 1e6, 1)} for i in head]
            row["head_ops_sum_ms"] = round(sum(o["median_ms"] for o in row["head_ops"]), 4)
        row["flag_costs_ms"] = round(row["backbone_forward_cpn_predict"]["median_ms"] - row["backbone_forward"]["median_ms"], 4)
        row["forward_detect_over_forward"] = round(row["forward_detect"]["median_ms"] / row["forward_given_keypoints"]["median_ms"], 3)
        print(json.dumps(row), flush=True)
        for m in models.values():
            for e in m._engines.values():
                e.close()
            m._engines.clear()


if __name__ == "__main__":
    main()
