"""The pooled fp32 head kernels (adil_pool_head_fwd / adil_pool_head_bwd) against the two torch ways to the logits of a bf16
MobileNetV2: the torch fp32 head (`zoo._Fp32Head.forward`'s formula, `F.linear(x.float().mean((2, 3)), w, b)`, under
autograd: the only other way to fp32 logits) and the library bf16 head (`F.adaptive_avg_pool2d` + bf16 `F.linear`, bf16
logits).  Timed in ONE process, alternating, warmed up, with device events: B = 512, 7 x 7, C = 1280, N = 1000, forward and
input gradient each; the pool and broadcast passes also as algorithmic bytes / time over the 5.1 TB/s copy yardstick
(profiles/r04_stream_patterns.md).  Then a whole forward + input gradient of MobileNetV2 with the three own_* switches on,
without and with `head_fp32=True`, alternating rounds.  Writes one JSON document (default profiles/head_bench.json) and
prints it.

usage: python tools/bench_head.py [--batch 512] [--rounds 7] [--iters 20] [--net-rounds 5] [--net-iters 4] [--out PATH]
       --only kernels|network restricts the run, --variants three,three_head_fp32 the network part (a kernel trace wants one:
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_head.py --only network
       --variants three_head_fp32 --net-rounds 1 --net-iters 4 --out /dev/null, then tools/prof_summary.py DIR)"""
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
THREE = dict(own_depthwise=True, own_pointwise=True, own_first_conv=True)
VARIANTS = {"three": dict(THREE), "three_head_fp32": dict(THREE, head_fp32=True)}


def bench_kernels(args, dev):
    lib = _lib.load()
    b, h, w, c, n = args.batch, 7, 7, 1280, 1000
    hw = h * w
    gen = torch.Generator().manual_seed(7)
    x3 = torch.randn(b, hw, c, generator=gen).bfloat16().to(dev)                                # NHWC storage
    wgt = (torch.randn(n, c, generator=gen) / c ** 0.5).to(dev)
    bias = torch.randn(n, generator=gen).to(dev)
    g = torch.randn(b, n, generator=gen).to(dev)
    wt = wgt.t().contiguous()
    w16, b16, g16 = wgt.bfloat16(), bias.bfloat16(), g.bfloat16()
    pooled, gpooled = torch.empty(b, c, device=dev), torch.empty(b, c, device=dev)
    logits = torch.empty(b, n, device=dev)
    gx = torch.empty(b, hw, c, dtype=torch.bfloat16, device=dev)
    xt = x3.reshape(b, h, w, c).permute(0, 3, 1, 2).requires_grad_(True)                        # channels_last NCHW view
    torch_fp32 = lambda xin: F.linear(xin.float().mean(dim=(2, 3)), wgt, bias)
    lib_bf16 = lambda xin: F.linear(torch.flatten(F.adaptive_avg_pool2d(xin, 1), 1), w16, b16)
    y32, y16 = torch_fp32(xt), lib_bf16(xt)
    st, P = ops._stream(), ops._ptr
    fns = {
        "own_fwd": lambda: lib.adil_pool_head_fwd(P(x3), P(wt), P(bias), P(pooled), P(logits), b, hw, c, n, st),
        "torch_fp32_fwd": lambda: torch_fp32(xt.detach()),
        "lib_bf16_fwd": lambda: lib_bf16(xt.detach()),
        "own_bwd": lambda: lib.adil_pool_head_bwd(P(g), P(wgt), P(gpooled), P(gx), b, hw, c, n, st),
        "torch_fp32_bwd": lambda: torch.autograd.grad(y32, xt, g, retain_graph=True),
        "lib_bf16_bwd": lambda: torch.autograd.grad(y16, xt, g16, retain_graph=True),
    }
    for fn in fns.values():                                                                      # library find / warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    (g32,) = torch.autograd.grad(y32, xt, g, retain_graph=True)
    agree = {"max_abs_diff_logits_own_vs_torch_fp32": float((logits - y32.detach()).abs().max()),
             "max_abs_diff_logits_lib_bf16_vs_torch_fp32": float((y16.detach().float() - y32.detach()).abs().max()),
             "relative_diff_gx_own_vs_torch_fp32": float((gx.reshape(b, h, w, c).permute(0, 3, 1, 2).float() - g32.float()).norm()
                                                         / g32.float().norm())}
    times = {key: [] for key in fns}
    for _ in range(args.rounds):
        for key, fn in fns.items():
            times[key].append(events_us(fn, args.iters))
    stream_bytes = float(b) * hw * c * 2                                                         # x read once / gx written once
    us = {key: stats(t) for key, t in times.items()}
    loses = {d: [k for k in ("torch_fp32", "lib_bf16") if us["own_" + d]["median"] > us[k + "_" + d]["median"]]
             for d in ("fwd", "bwd")}
    out = {"B": b, "H": h, "W": w, "C": c, "N": n, "stream_mbytes_per_pass": round(stream_bytes / 1e6, 1), **agree, "us": us,
           "conditions": {d: {"own_no_slower_than_torch_fp32_at_median": us["own_" + d]["median"] <= us["torch_fp32_" + d]["median"]}
                          for d in ("fwd", "bwd")},
           "loses_to": loses}
    # the stream passes alone: a call with N = 4 leaves the GEMM next to nothing (B x 1280 x 4), so its time is that of the pass
    wt4, w4, bias4, g4 = wt[:, :4].contiguous(), wgt[:4].contiguous(), bias[:4].contiguous(), g[:, :4].contiguous()
    l4 = torch.empty(b, 4, device=dev)
    small = {"pool_pass_fwd_N4": lambda: lib.adil_pool_head_fwd(P(x3), P(wt4), P(bias4), P(pooled), P(l4), b, hw, c, 4, st),
             "broadcast_pass_bwd_N4": lambda: lib.adil_pool_head_bwd(P(g4), P(w4), P(gpooled), P(gx), b, hw, c, 4, st)}
    passes = {}
    for key, fn in small.items():
        for _ in range(3):
            fn()
        t = stats([events_us(fn, args.iters) for _ in range(args.rounds)], stream_bytes)
        t["fraction_of_copy_yardstick"] = round(t["algorithmic_tb_per_s_at_median"] / COPY_TB_PER_S, 3)
        passes[key] = t
    out["stream_passes"] = {"what": "the same entry points at N = 4: two launches, the GEMM is B x 1280 x 4; algorithmic bytes = "
                                    "the bf16 activation once", **passes}
    print(json.dumps(out), flush=True)
    return out


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_head_"), "mobilenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {v: zoo.build_classifier("mobilenet", dtype=torch.bfloat16, channels_last=True, **VARIANTS[v], **kw)
              for v in args.variants.split(",")}
    out = {"what": "MobileNetV2 bf16 channels_last, %d structured images at 224 x 224, forward + input gradient of sum(logits^2); "
                   "three = own_depthwise + own_pointwise + own_first_conv (library pooling + bf16 linear), three_head_fp32 = the "
                   "same + head_fp32=True (fp32 logits from the own head); alternating rounds of %d passes" % (b, args.net_iters)}
    ref = zoo.build_classifier("mobilenet", **kw)
    xs = images[:32].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    rms = float(lr.square().mean().sqrt())
    acc = {}
    for v, model in models.items():
        l, g = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((l - lr).abs().mean()),
                  "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_32_images"] = {"rms_logit": rms, **acc}
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
    if "three" in times and "three_head_fp32" in times:
        three, head = out["ms_per_pass"]["three"], out["ms_per_pass"]["three_head_fp32"]
        out["condition"] = {"head_fp32_no_slower_at_median": head["median"] <= three["median"],
                            "difference_ms_at_median": round(head["median"] - three["median"], 3)}
        out["loses_to"] = [] if head["median"] <= three["median"] else ["three"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=4)
    p.add_argument("--only", choices=["kernels", "network"], default=None)
    p.add_argument("--variants", default="three,three_head_fp32", help="network part: any of three, three_head_fp32")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_pool_head_fwd / _bwd vs the torch fp32 head (x.float().mean((2, 3)) + fp32 F.linear, autograd) and the "
                   "library bf16 head (F.adaptive_avg_pool2d + bf16 F.linear, autograd), one process, alternating rounds, device "
                   "events; microseconds per call; fractions are algorithmic bytes / time over the %.1f TB/s copy yardstick"
                   % COPY_TB_PER_S,
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
