"""The narrow-channel pointwise kernels (adil_pw8_fwd / adil_pw8_bwd) against the library sequence they replace (F.conv2d
1x1 + F.batch_norm in eval mode (+ residual add) (+ hardtanh(0, 6)) and its autograd input gradient, on channels_last bf16
tensors), timed in ONE process, alternating, warmed up, with device events: the 19 distinct (K, N, H) 1x1 layers of
MobileNetV2 at 224 x 224, B = 512, forward and input gradient, with algorithmic bytes / time as a fraction of the 5.1 TB/s
copy yardstick (profiles/r04_stream_patterns.md); then a whole forward + input gradient of MobileNetV2 in three
configurations, alternating rounds: `own_depthwise` only (the best configuration without these kernels), both switches,
`own_pointwise` only.  Writes one JSON document (default profiles/pointwise8_bench.json) and prints it.

usage: python tools/bench_pointwise8.py [--batch 512] [--rounds 5] [--iters 10] [--net-rounds 5] [--net-iters 4] [--out PATH]
       --only kernels|network restricts the run, --variants depthwise,both,pointwise the network part (a kernel trace wants
       one: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_pointwise8.py --only network
       --variants both --net-rounds 1 --net-iters 4 --out /dev/null, then tools/prof_summary.py DIR)"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_depthwise import events_us, forward_and_gradient, random_bn_checkpoint, stats, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import _lib, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

COPY_TB_PER_S = 5.1
# (K, N, H = W, act, res, how many of the 34 layers have the shape); res: the residual blocks among them (timed with res)
SHAPES = [(32, 16, 112, 0, 0, 1), (16, 96, 112, 1, 0, 1), (96, 24, 56, 0, 0, 1), (24, 144, 56, 1, 0, 2), (144, 24, 56, 0, 1, 1),
          (144, 32, 28, 0, 0, 1), (32, 192, 28, 1, 0, 3), (192, 32, 28, 0, 1, 2), (192, 64, 14, 0, 0, 1), (64, 384, 14, 1, 0, 4),
          (384, 64, 14, 0, 1, 3), (384, 96, 14, 0, 0, 1), (96, 576, 14, 1, 0, 3), (576, 96, 14, 0, 1, 2), (576, 160, 7, 0, 0, 1),
          (160, 960, 7, 1, 0, 3), (960, 160, 7, 0, 1, 2), (960, 320, 7, 0, 0, 1), (320, 1280, 7, 1, 0, 1)]
VARIANTS = {"depthwise": dict(own_depthwise=True), "both": dict(own_depthwise=True, own_pointwise=True),
            "pointwise": dict(own_pointwise=True)}


def bench_kernels(args, dev):
    lib = _lib.load()
    out = []
    b = args.batch
    for k, n, hw, act, with_res, count in SHAPES:
        m = b * hw * hw
        gen = torch.Generator().manual_seed(k + n + hw)
        x = torch.randn(b, hw, hw, k, generator=gen).bfloat16().to(dev)                      # NHWC storage
        g = torch.randn(b, hw, hw, n, generator=gen).bfloat16().to(dev)
        r = torch.randn(b, hw, hw, n, generator=gen).bfloat16().to(dev) if with_res else None
        w = (torch.randn(n, k, generator=gen) * (2.0 / k ** 0.5)).bfloat16().to(dev)
        wt = w.t().contiguous()
        bn = torch.nn.BatchNorm2d(n).eval()
        with torch.no_grad():
            bn.weight.copy_(0.7 + 0.6 * torch.rand(n, generator=gen))
            bn.bias.copy_(0.5 * torch.randn(n, generator=gen) + (1.0 if act else 0.0))
            bn.running_mean.copy_(0.2 * torch.randn(n, generator=gen))
            bn.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=gen))
        scale, shift = (t.to(dev) for t in zoo._bn_affine(bn))
        bn = bn.to(dev).bfloat16()
        y = torch.empty(b, hw, hw, n, dtype=torch.bfloat16, device=dev)
        gx = torch.empty(b, hw, hw, k, dtype=torch.bfloat16, device=dev)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)                                        # channels_last NCHW view
        gt = g.permute(0, 3, 1, 2)
        rt = None if r is None else r.permute(0, 3, 1, 2)
        w4 = w.reshape(n, k, 1, 1).contiguous(memory_format=torch.channels_last)

        def lib_fwd(xin=xt):
            v = F.batch_norm(F.conv2d(xin, w4), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
            if rt is not None:
                v = rt + v
            return F.hardtanh(v, 0.0, 6.0) if act else v

        yl = lib_fwd()
        st = ops._stream()
        P = ops._ptr
        fns = {
            "own_fwd": lambda: lib.adil_pw8_fwd(P(x), P(w), P(scale), P(shift), P(r), P(y), m, k, n, act, st),
            "lib_fwd": lambda: lib_fwd(xt.detach()),
            "own_bwd": lambda: lib.adil_pw8_bwd(P(g), P(y) if act else None, P(scale), P(wt), P(gx), m, k, n, act, st),
            "lib_bwd": lambda: torch.autograd.grad(yl, xt, gt, retain_graph=True),
        }
        for fn in fns.values():                                                                 # library find / warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # agreement of the two paths on this shape (the library path rounds after the convolution and after BatchNorm)
        df = float((y.float() - yl.detach().permute(0, 2, 3, 1).float()).abs().max())
        (gl,) = torch.autograd.grad(yl, xt, gt, retain_graph=True)
        db = float((gx.float() - gl.permute(0, 2, 3, 1).float()).abs().max())
        times = {key: [] for key in fns}
        for _ in range(args.rounds):
            for key, fn in fns.items():
                times[key].append(events_us(fn, args.iters))
        by_f = 2.0 * m * (k + n * (2 if with_res else 1))                                      # x, y (, res)
        by_b = 2.0 * m * (k + n * (2 if act else 1))                                           # g, gx (, y for the mask)
        us = {key: stats(t, by_f if key.endswith("fwd") else by_b) for key, t in times.items()}
        for key in us:
            us[key]["fraction_of_copy_yardstick"] = round(us[key]["algorithmic_tb_per_s_at_median"] / COPY_TB_PER_S, 3)
        out.append({"K": k, "N": n, "H": hw, "W": hw, "act": act, "res": with_res, "B": b, "layers_of_this_shape": count,
                    "algorithmic_mbytes": {"fwd": round(by_f / 1e6, 1), "bwd": round(by_b / 1e6, 1)},
                    "max_abs_diff_own_vs_library": {"fwd": df, "bwd": db}, "us": us,
                    "loses_to_the_library": [d for d in ("fwd", "bwd") if us["own_" + d]["median"] > us["lib_" + d]["median"]]})
        print(json.dumps(out[-1]), flush=True)
        del x, g, r, y, gx, xt, gt, rt, yl, gl
        torch.cuda.empty_cache()
    tot = {key: round(sum(r["us"][key]["median"] * r["layers_of_this_shape"] for r in out) / 1e3, 3)
           for key in ("own_fwd", "lib_fwd", "own_bwd", "lib_bwd")}
    gb = {d: round(sum(r["algorithmic_mbytes"][d] * r["layers_of_this_shape"] for r in out) / 1e3, 2) for d in ("fwd", "bwd")}
    return {"shapes": out, "ms_over_the_34_layers_at_median": tot, "algorithmic_gbytes_over_the_34_layers": gb,
            "fraction_of_copy_yardstick_over_the_34_layers": {
                d: round(gb[d] / tot["own_" + d] / COPY_TB_PER_S, 3) for d in ("fwd", "bwd")},
            "layers_that_lose_to_the_library": [(r["K"], r["N"], r["H"], d) for r in out for d in r["loses_to_the_library"]]}


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_pw8_"), "mobilenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {v: zoo.build_classifier("mobilenet", dtype=torch.bfloat16, channels_last=True, **VARIANTS[v], **kw)
              for v in args.variants.split(",")}
    out = {"what": "MobileNetV2 bf16 channels_last, %d structured images at 224 x 224, forward + input gradient of sum(logits^2); "
                   "depthwise = own_depthwise only (the best configuration without the pointwise kernels), both = both switches, "
                   "pointwise = own_pointwise only; alternating rounds of %d passes" % (b, args.net_iters)}
    ref = zoo.build_classifier("mobilenet", **kw)
    xs = images[:32].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    rms = float(lr.square().mean().sqrt())
    acc = {}
    for v, model in models.items():
        l, g = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((l - lr).abs().mean()),
                  "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_32_images"] = {"rms_logit": rms, "bf16_depth_bound_53_layers": 2.0 * 2.0 ** -9 * 53 ** 0.5 * rms,
                                                    **acc}
    del ref, lr, gr
    x = images.to(dev).bfloat16()

    def one(v):
        xi = x.detach().requires_grad_(True)
        logits = models[v](xi).float()
        torch.autograd.grad(logits.square().sum(), xi)

    for v in models:
        for _ in range(3):
            one(v)
    torch.cuda.synchronize()
    times = {v: [] for v in models}
    for _ in range(args.net_rounds):
        for v in models:
            times[v].append(events_us(lambda: one(v), args.net_iters) / 1e3)
    out["ms_per_pass"] = {v: {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                              "spread": round(max(t) - min(t), 3), "rounds": [round(u, 3) for u in t]} for v, t in times.items()}
    if "depthwise" in times and "both" in times:
        d, w = out["ms_per_pass"]["depthwise"], out["ms_per_pass"]["both"]
        out["pass_condition"] = {"gain_ms_at_median": round(d["median"] - w["median"], 3),
                                 "larger_spread_ms": max(d["spread"], w["spread"]),
                                 "both_faster_by_more_than_either_spread": bool(d["median"] - w["median"] > max(d["spread"], w["spread"])
                                                                                and w["max"] < d["min"])}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=4)
    p.add_argument("--only", choices=["kernels", "network"], default=None)
    p.add_argument("--variants", default="depthwise,both,pointwise", help="network part: any of depthwise, both, pointwise")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointwise8_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_pw8_fwd / _bwd vs F.conv2d 1x1 + F.batch_norm (+ add) (+ hardtanh(0, 6)) and their autograd input "
                   "gradient (channels_last bf16), one process, alternating rounds, device events; microseconds per call; "
                   "fractions are algorithmic bytes / time over the %.1f TB/s copy yardstick" % COPY_TB_PER_S,
           "kernel_source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "iters_per_round": args.iters}
    if args.only != "network":
        out["kernels"] = bench_kernels(args, dev)
    if args.only != "kernels":
        out["network"] = bench_network(args, dev)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
