"""The pooled head kernels behind a BatchNorm + ReLU (adil_bn_pool_head_fwd / adil_bn_pool_head_bwd) against the two torch ways
to the logits of a bf16 DenseNet-121 from the output of its last dense block: the torch fp32 formula
(`zoo._OwnDenseHead.forward`'s own fallback, `F.linear(relu(x.float() * pscale + pshift).mean((2, 3)), w, b)`, under
autograd: the only other way to fp32 logits) and the library bf16 chain (`F.batch_norm` + `F.relu` + `F.adaptive_avg_pool2d`
+ bf16 `F.linear`, bf16 logits).  Timed in ONE process, alternating, warmed up, with device events: B = 512, 7 x 7, C = 1024,
N = 1000, forward and input gradient each; the two stream passes also as algorithmic bytes / time over the 5.1 TB/s copy
yardstick (profiles/r04_stream_patterns.md; forward: x once, gradient: x once + gx once).  Then a whole forward + input
gradient of DenseNet-121 with the five dense switches, without and with `own_dense_head=True`, alternating rounds.  Writes
one JSON document (default profiles/dense_head_bench.json) and prints it.

usage: python tools/bench_dense_head.py [--batch 512] [--rounds 7] [--iters 20] [--net-rounds 5] [--net-iters 2] [--out PATH]
       --only kernels|network restricts the run"""
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

from bench_dense1x1 import random_bn_checkpoint  # noqa: E402
from bench_depthwise import events_us, forward_and_gradient, stats, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import _lib, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

COPY_TB_PER_S = 5.1
FIVE = dict(own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True, own_dense_transition=True, own_dense_stem=True)
VARIANTS = {"five": dict(FIVE), "six": dict(FIVE, own_dense_head=True)}


def bench_kernels(args, dev):
    lib = _lib.load()
    b, h, w, c, n = args.batch, 7, 7, 1024, 1000
    hw = h * w
    gen = torch.Generator().manual_seed(7)
    x3 = torch.randn(b, hw, c, generator=gen).bfloat16().to(dev)                                # NHWC storage
    sign = (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float()
    var, gamma = 0.6 + 0.8 * torch.rand(c, generator=gen), (0.7 + 0.6 * torch.rand(c, generator=gen)) * sign
    mean, beta = 0.2 * torch.randn(c, generator=gen), 0.2 * torch.randn(c, generator=gen)
    bn = torch.nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(mean), bn.running_var.copy_(var)
    ps, pb = (t.to(dev) for t in zoo._bn_affine(bn))
    bn16 = [t.to(dev).bfloat16() for t in (mean, var, gamma, beta)]
    wgt = (torch.randn(n, c, generator=gen) / c ** 0.5).to(dev)
    bias = torch.randn(n, generator=gen).to(dev)
    g = torch.randn(b, n, generator=gen).to(dev)
    wt = wgt.t().contiguous()
    w16, b16, g16 = wgt.bfloat16(), bias.bfloat16(), g.bfloat16()
    pooled, gpooled = torch.empty(b, c, device=dev), torch.empty(b, c, device=dev)
    logits = torch.empty(b, n, device=dev)
    gx = torch.empty(b, hw, c, dtype=torch.bfloat16, device=dev)
    xt = x3.reshape(b, h, w, c).permute(0, 3, 1, 2).requires_grad_(True)                        # channels_last NCHW view
    ps4, pb4 = ps.reshape(1, -1, 1, 1), pb.reshape(1, -1, 1, 1)
    torch_fp32 = lambda xin: F.linear(F.relu(xin.float() * ps4 + pb4).mean(dim=(2, 3)), wgt, bias)

    def lib_bf16(xin):                                                                           # `DenseNet.forward` behind the trunk
        y = F.relu(F.batch_norm(xin, bn16[0], bn16[1], bn16[2], bn16[3], False, 0.1, bn.eps), inplace=True)
        return F.linear(torch.flatten(F.adaptive_avg_pool2d(y, 1), 1), w16, b16)

    y32, y16 = torch_fp32(xt), lib_bf16(xt)
    st, P = ops._stream(), ops._ptr
    fns = {
        "own_fwd": lambda: lib.adil_bn_pool_head_fwd(P(x3), P(ps), P(pb), P(wt), P(bias), P(pooled), P(logits), b, hw, c, n, st),
        "torch_fp32_fwd": lambda: torch_fp32(xt.detach()),
        "lib_bf16_fwd": lambda: lib_bf16(xt.detach()),
        "own_bwd": lambda: lib.adil_bn_pool_head_bwd(P(g), P(wgt), P(x3), P(ps), P(pb), P(gpooled), P(gx), b, hw, c, n, st),
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
    x_bytes = float(b) * hw * c * 2
    us = {key: stats(t) for key, t in times.items()}
    loses = {d: [k for k in ("torch_fp32", "lib_bf16") if us["own_" + d]["median"] > us[k + "_" + d]["median"]]
             for d in ("fwd", "bwd")}
    out = {"B": b, "H": h, "W": w, "C": c, "N": n, "stream_mbytes": {"fwd": round(x_bytes / 1e6, 1), "bwd": round(2 * x_bytes / 1e6, 1)},
           **agree, "us": us,
           "conditions": {d: {"own_no_slower_than_torch_fp32_at_median": us["own_" + d]["median"] <= us["torch_fp32_" + d]["median"]}
                          for d in ("fwd", "bwd")},
           "loses_to": loses}
    # The stream passes.  A call with N = 4 leaves the gradient's GEMM next to nothing (K = 4), so its time is that of the mask
    # pass.  The forward's GEMM still walks K = C = 1024 in 64 serial steps on B / 64 workgroups whatever N is, so the forward
    # at N = 4 is an upper bound of the pool pass only.  A kernel trace times the passes themselves:
    # rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_dense_head.py --only kernels --out /dev/null,
    # then tools/prof_summary.py DIR (head_bn_pool_kernel, head_bn_spread_kernel, head_gemm_kernel).
    wt4, w4, bias4, g4 = wt[:, :4].contiguous(), wgt[:4].contiguous(), bias[:4].contiguous(), g[:, :4].contiguous()
    l4 = torch.empty(b, 4, device=dev)
    small = {"pool_pass_and_gemm_fwd_N4": (lambda: lib.adil_bn_pool_head_fwd(P(x3), P(ps), P(pb), P(wt4), P(bias4), P(pooled), P(l4),
                                                                             b, hw, c, 4, st), x_bytes),
             "mask_pass_bwd_N4": (lambda: lib.adil_bn_pool_head_bwd(P(g4), P(w4), P(x3), P(ps), P(pb), P(gpooled), P(gx), b, hw, c,
                                                                    4, st), 2 * x_bytes)}
    passes = {}
    for key, (fn, nbytes) in small.items():
        for _ in range(3):
            fn()
        t = stats([events_us(fn, args.iters) for _ in range(args.rounds)], nbytes)
        t["fraction_of_copy_yardstick"] = round(t["algorithmic_tb_per_s_at_median"] / COPY_TB_PER_S, 3)
        passes[key] = t
    out["stream_passes"] = {"what": "the same entry points at N = 4: two launches; the gradient's GEMM is B x 4 x 1024 and its figure is "
                                    "the mask pass; the forward's GEMM walks K = 1024 in 64 serial steps on B / 64 workgroups, so the "
                                    "forward figure is an upper bound of the pool pass (a kernel trace times the pass itself); "
                                    "algorithmic bytes = the bf16 activation once (forward), read once and written once (gradient)",
                            **passes}
    print(json.dumps(out), flush=True)
    return out


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_dh_"), "densenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {v: zoo.build_classifier("densenet121", dtype=torch.bfloat16, channels_last=True, **extra, **kw)
              for v, extra in VARIANTS.items()}
    assert isinstance(models["six"][0].head32, zoo._OwnDenseHead) and models["five"][0].head32 is None
    out = {"what": "DenseNet-121 bf16 channels_last, %d structured images at 224 x 224, forward + input gradient of sum(logits^2); "
                   "five = the five dense switches (library norm5, ReLU, pooling, bf16 linear), six = the same + "
                   "own_dense_head=True (fp32 logits from the own head); alternating rounds of %d passes" % (b, args.net_iters)}
    ref = zoo.build_classifier("densenet121", **kw)
    xs = images[:16].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    rms = float(lr.square().mean().sqrt())
    acc = {}
    for v, model in models.items():
        l, g = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((l - lr).abs().mean()),
                  "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_16_images"] = {"rms_logit": rms, **acc}
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
    five, six = out["ms_per_pass"]["five"], out["ms_per_pass"]["six"]
    out["condition"] = {"six_no_slower_than_five_at_median": six["median"] <= five["median"],
                        "difference_ms_at_median": round(six["median"] - five["median"], 3)}
    out["loses_to"] = [] if six["median"] <= five["median"] else ["five"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=2)
    p.add_argument("--only", choices=["kernels", "network"], default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_head_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_bn_pool_head_fwd / _bwd vs the torch fp32 formula (relu(x.float() * pscale + pshift).mean((2, 3)) + fp32 "
                   "F.linear, autograd) and the library bf16 chain (F.batch_norm + F.relu + F.adaptive_avg_pool2d + bf16 F.linear, "
                   "autograd), one process, alternating rounds, device events; microseconds per call; fractions are algorithmic "
                   "bytes / time over the %.1f TB/s copy yardstick" % COPY_TB_PER_S,
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
