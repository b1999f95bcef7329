"""The forward from uint8 crops against the float-image route (EXPERIMENTS R19.1): in ONE process, alternating windows of
    float route:  capf_preprocess (uint8 BGR crops -> fp32 RGB image + points) + capf_forward
    u8 route:     capf_preprocess_points + capf_forward_u8 (normalisation, BGR flip and mirror in the stem conv's load)
on the same crops, every buffer allocated before the clock starts.  A window is as many steps as take >= --window-s seconds (found in
the warm-up), timed with device events; --reps windows per route, F U F U ...  Reported per case: median ms per step of both routes, the
spread of the float route's own windows ((max - min) / median: what a difference has to exceed to mean anything), and the peak device
memory of either route (torch's allocator: workspace + inputs + the fp32 image where there is one).  Synthetic weights, random crops.
Cases: configs[1] (HRNet-32 fp32, 64 x 256 x 256), configs[2]'s geometry (HRNet-48 bf16, 256 x 256 x 256), CPN bf16 128 x 384 x 288, and
each as a flip-test pair (mode 2: the same source frames, twice the engine frames).  One JSON line per case, then the table.
    python tools/bench_u8_input.py [--window-s 1.0] [--reps 5] [--warmup 3] [--only NAME]"""
import argparse
import contextlib
import copy
import ctypes
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))

import torch

CASES = [  # (name, backbone, dtype, source frames, H, W)
    ("cfg1 hrnet_32 fp32", "hrnet_32", "fp32", 64, 256, 256),
    ("cfg2 hrnet_48 bf16", "hrnet_48", "bf16", 256, 256, 256),
    ("cpn bf16 384x288", "cpn", "bf16", 128, 384, 288),
]
J = 17


def model_for(backbone, dtype):
    from capf import synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), backbone)
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(cfg, compute_dtype=dtype).eval()
    synth.load_synthetic(m, seed=3, bn_mode="random")
    return m.cuda()


class Route:
    """one route's buffers and its step; everything it allocates is its own, so that its peak memory is its own"""

    def __init__(self, eng, crops, k2d, kc, backbone, mode, u8):
        from capf import lib
        self.eng, self.lib, self.L, self.u8, self.mode, self.crops = eng, lib, lib.load_library(), u8, mode, crops
        Bsrc, H, W, _ = crops.shape
        self.Bsrc, self.H, self.W = Bsrc, H, W
        self.B = 2 * Bsrc if mode == 2 else Bsrc
        self.k2d_in, self.kc_in = k2d, kc
        self.k2d = torch.empty(self.B, J, 2, device="cuda")
        self.kc = torch.empty(self.B, J, 2, device="cuda")
        self.out = torch.empty(self.B, 1, J, 3, device="cuda")
        self.img = None if u8 else torch.empty(self.B, H, W, 3, device="cuda")
        self.m3, self.s3 = lib.input_constants("cpn" if backbone == "cpn" else "hrnet_32")
        self.stream = torch.cuda.current_stream().cuda_stream

    def step(self):
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        s = ctypes.c_void_p(self.stream)
        if self.u8:
            rc = self.L.capf_preprocess_points(s, self.Bsrc, self.mode, None, None, P(self.k2d_in), P(self.k2d), P(self.kc_in), P(self.kc))
            assert rc == 0, rc
            self.eng.forward_u8(self.crops, self.m3, self.s3, self.mode, self.k2d, self.kc, self.out, self.stream)
        else:
            rc = self.L.capf_preprocess(s, P(self.crops), self.Bsrc, self.H, self.W, self.m3, self.s3, self.mode, P(self.img), None, None,
                                        P(self.k2d_in), P(self.k2d), P(self.kc_in), P(self.kc))
            assert rc == 0, rc
            self.eng.forward(self.img, self.k2d, self.kc, self.out, self.stream)


def window(route, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        route.step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def peak_mb(make_route):
    """peak allocated device memory while one route exists and runs, above nothing: the caller holds only the model"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    r = make_route()
    r.step(); r.step()
    torch.cuda.synchronize()
    mb = torch.cuda.max_memory_allocated() / 2 ** 20
    return r, mb


def run_case(name, backbone, dtype, Bsrc, H, W, mode, a):
    model = model_for(backbone, dtype)
    g = torch.Generator().manual_seed(7)
    crops = torch.randint(0, 256, (Bsrc, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    k2d = (torch.rand(Bsrc, J, 2, generator=g) * 2 - 1).cuda()
    kc = (torch.rand(Bsrc, J, 2, generator=g) * (W - 1)).cuda()
    B = 2 * Bsrc if mode == 2 else Bsrc
    with torch.no_grad():
        eng = model._engine_at(torch.device("cuda", torch.cuda.current_device()), H, W)
        eng.ensure_workspace(B)
        base_mb = torch.cuda.memory_allocated() / 2 ** 20                      # model + packs' sources + workspace + the crops and points
        fl, mb_f = peak_mb(lambda: Route(eng, crops, k2d, kc, backbone, mode, False))
        same_out = fl.out.clone()
        del fl
        u8, mb_u = peak_mb(lambda: Route(eng, crops, k2d, kc, backbone, mode, True))
        same = bool(torch.equal(u8.out, same_out))                              # the two routes compute the same bits (the tests' claim, re-checked at size)
        fl = Route(eng, crops, k2d, kc, backbone, mode, False)
        for _ in range(a.warmup):
            fl.step(); u8.step()
        torch.cuda.synchronize()
        probe = max(window(fl, 3), window(u8, 3))
        steps = max(3, int(a.window_s * 1e3 / probe) + 1)
        tf, tu = [], []
        for _ in range(a.reps):
            tf.append(window(fl, steps))
            tu.append(window(u8, steps))
    mf, mu = statistics.median(tf), statistics.median(tu)
    spread = (max(tf) - min(tf)) / mf
    res = {"case": name + (" pair" if mode == 2 else ""), "engine_frames": B, "source_frames": Bsrc, "crop": f"{H}x{W}", "dtype": dtype,
           "stem_kernel_float": eng.op_table(B)[0][1], "steps_per_window": steps, "windows": a.reps,
           "float_ms": round(mf, 4), "u8_ms": round(mu, 4), "u8_minus_float_pct": round(100 * (mu - mf) / mf, 3),
           "float_spread_pct": round(100 * spread, 3), "u8_spread_pct": round(100 * (max(tu) - min(tu)) / mu, 3),
           "float_windows_ms": [round(x, 4) for x in tf], "u8_windows_ms": [round(x, 4) for x in tu],
           "peak_mb_float": round(mb_f, 1), "peak_mb_u8": round(mb_u, 1), "base_mb": round(base_mb, 1), "same_bits": same}
    for e in list(model._engines.values()):
        e.close()
    model._engines.clear()
    del model, eng, fl, u8
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="substring of a case name")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU timing of a GPU route"
    rows = []
    for name, backbone, dtype, Bsrc, H, W in CASES:
        for mode in (0, 2):
            if a.only and a.only not in name + (" pair" if mode == 2 else ""):
                continue
            r = run_case(name, backbone, dtype, Bsrc, H, W, mode, a)
            rows.append(r)
            print(json.dumps(r), flush=True)
    print("\n| case | engine frames | float ms/step | u8 ms/step | u8 - float | float spread | peak MB float | peak MB u8 | same bits |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['engine_frames']} | {r['float_ms']:.3f} | {r['u8_ms']:.3f} | {r['u8_minus_float_pct']:+.2f} % | "
              f"{r['float_spread_pct']:.2f} % | {r['peak_mb_float']:.0f} | {r['peak_mb_u8']:.0f} | {r['same_bits']} |")


if __name__ == "__main__":
    main()
