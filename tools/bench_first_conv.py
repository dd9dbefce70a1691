"""The first-convolution kernels (adil_first3x3_fwd / adil_first3x3_bwd) against the library sequence they replace
(Normalize -> .to(channels_last) -> F.conv2d 3 -> 32, 3x3, stride 2 -> F.batch_norm in eval mode -> hardtanh(0, 6), and its
autograd input gradient), timed in ONE process, alternating, warmed up, with device events: B = 512 at 224 x 224, bf16 and
fp32 streams, forward and input gradient, with algorithmic bytes / time as a fraction of the 5.1 TB/s copy yardstick
(profiles/r04_stream_patterns.md); then a whole forward + input gradient of MobileNetV2 in two configurations, alternating
rounds: `own_depthwise` + `own_pointwise` (the best configuration without these kernels) and all three switches.  Writes
one JSON document (default profiles/first_conv_bench.json) and prints it.

usage: python tools/bench_first_conv.py [--batch 512] [--rounds 5] [--iters 10] [--net-rounds 5] [--net-iters 4] [--out PATH]
       --only kernels|network restricts the run, --variants two,three the network part (a kernel trace wants one:
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_first_conv.py --only network
       --variants three --net-rounds 1 --net-iters 4 --out /dev/null, then tools/prof_summary.py DIR)"""
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
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
VARIANTS = {"two": dict(own_depthwise=True, own_pointwise=True),
            "three": dict(own_depthwise=True, own_pointwise=True, own_first_conv=True)}


def bench_kernels(args, dev):
    lib = _lib.load()
    out = []
    b, h, w = args.batch, 224, 224
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for dtype in (torch.bfloat16, torch.float32):
        s = 2 if dtype == torch.bfloat16 else 4
        gen = torch.Generator().manual_seed(7)
        x = torch.rand(b, 3, h, w, generator=gen).to(dtype).to(dev)                            # the attack's NCHW stream
        g = torch.randn(b, oh, ow, 32, generator=gen).bfloat16().to(dev)                       # NHWC storage
        wgt = (torch.randn(32, 3, 3, 3, generator=gen) * (2.0 / 27 ** 0.5)).bfloat16().to(dev)
        bn = torch.nn.BatchNorm2d(32).eval()
        with torch.no_grad():
            bn.weight.copy_(0.7 + 0.6 * torch.rand(32, generator=gen))
            bn.bias.copy_(0.5 * torch.randn(32, generator=gen) + 1.0)
            bn.running_mean.copy_(0.2 * torch.randn(32, generator=gen))
            bn.running_var.copy_(0.6 + 0.8 * torch.rand(32, generator=gen))
        scale, shift = (t.to(dev) for t in zoo._bn_affine(bn))
        bn = bn.to(dev).bfloat16()
        norm = zoo.Normalize(MEAN, STD).to(dev).to(torch.bfloat16)                             # as inside the bf16 network
        wf, wb = ops.pack_first3x3_weights(wgt)
        inv_std = [1.0 / v for v in STD]
        y = torch.empty(b, oh, ow, 32, dtype=torch.bfloat16, device=dev)
        gx = torch.empty(b, 3, h, w, dtype=dtype, device=dev)
        xt = x.clone().requires_grad_(True)
        gt = g.permute(0, 3, 1, 2)
        w4 = wgt.contiguous(memory_format=torch.channels_last)

        def lib_fwd(xin=xt):
            v = norm(xin).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            v = F.batch_norm(F.conv2d(v, w4, None, 2, 1), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
            return F.hardtanh(v, 0.0, 6.0)

        yl = lib_fwd()
        st = ops._stream()
        P = ops._ptr
        code = ops.stream_dtype_code(dtype)
        fns = {
            "own_fwd": lambda: lib.adil_first3x3_fwd(P(x), code, P(wf), *MEAN, *inv_std, P(scale), P(shift), P(y), b, h, w, 1, st),
            "lib_fwd": lambda: lib_fwd(xt.detach()),
            "own_bwd": lambda: lib.adil_first3x3_bwd(P(g), P(y), P(scale), P(wb), *inv_std, P(gx), code, b, h, w, 1, st),
            "lib_bwd": lambda: torch.autograd.grad(yl, xt, gt, retain_graph=True),
        }
        for fn in fns.values():                                                                 # library find / warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # agreement of the two paths (the library path rounds after the normalisation, the convolution and BatchNorm)
        df = float((y.float() - yl.detach().permute(0, 2, 3, 1).float()).abs().max())
        (gl,) = torch.autograd.grad(yl, xt, gt, retain_graph=True)
        db = float((gx.float() - gl.float()).norm() / gl.float().norm())
        times = {key: [] for key in fns}
        for _ in range(args.rounds):
            for key, fn in fns.items():
                times[key].append(events_us(fn, args.iters))
        by_f = float(b) * (3 * h * w * s + oh * ow * 32 * 2)                                   # read x, write y
        by_b = float(b) * (2 * oh * ow * 32 * 2 + 3 * h * w * s)                               # read g and y, write gx
        us = {key: stats(t, by_f if key.endswith("fwd") else by_b) for key, t in times.items()}
        for key in us:
            us[key]["fraction_of_copy_yardstick"] = round(us[key]["algorithmic_tb_per_s_at_median"] / COPY_TB_PER_S, 3)
        out.append({"stream_dtype": str(dtype).split(".")[-1], "B": b, "H": h, "W": w,
                    "algorithmic_mbytes": {"fwd": round(by_f / 1e6, 1), "bwd": round(by_b / 1e6, 1)},
                    "max_abs_diff_fwd_own_vs_library": df, "relative_diff_bwd_own_vs_library": db, "us": us,
                    "loses_to_the_library": [d for d in ("fwd", "bwd") if us["own_" + d]["median"] > us["lib_" + d]["median"]]})
        print(json.dumps(out[-1]), flush=True)
        del x, g, y, gx, xt, gt, yl, gl
        torch.cuda.empty_cache()
    return {"streams": out, "directions_that_lose_to_the_library": [(r["stream_dtype"], d) for r in out
                                                                   for d in r["loses_to_the_library"]]}


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_fc_"), "mobilenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {v: zoo.build_classifier("mobilenet", dtype=torch.bfloat16, channels_last=True, **VARIANTS[v], **kw)
              for v in args.variants.split(",")}
    out = {"what": "MobileNetV2 bf16 channels_last, %d structured images at 224 x 224, forward + input gradient of sum(logits^2); "
                   "two = own_depthwise + own_pointwise (the best configuration without the first-convolution kernels), three = "
                   "all three switches; alternating rounds of %d passes" % (b, args.net_iters)}
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
    if "two" in times and "three" in times:
        two, three = out["ms_per_pass"]["two"], out["ms_per_pass"]["three"]
        out["pass_condition"] = {"gain_ms_at_median": round(two["median"] - three["median"], 3),
                                 "every_round_of_three_below_every_round_of_two": bool(three["max"] < two["min"])}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=4)
    p.add_argument("--only", choices=["kernels", "network"], default=None)
    p.add_argument("--variants", default="two,three", help="network part: any of two, three")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_conv_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_first3x3_fwd / _bwd vs Normalize + .to(channels_last) + F.conv2d 3x3/2 + F.batch_norm + hardtanh(0, 6) "
                   "and their autograd input gradient, one process, alternating rounds, device events; microseconds per call; "
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
