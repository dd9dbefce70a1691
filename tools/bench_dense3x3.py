"""The 32-channel 3x3 convolution kernels (adil_dense3x3_fwd / adil_dense3x3_bwd) against the library convolution they
replace (F.conv2d 3x3 / pad 1 on channels_last bf16 tensors and its autograd input gradient), timed in ONE process,
alternating, warmed up, with device events: the four shapes of DenseNet-121's 58 growth convolutions (128 -> 32 at 56, 28,
14, 7), B = 512, forward and input gradient, with algorithmic bytes / time as a fraction of the 5.1 TB/s copy yardstick
(profiles/r04_stream_patterns.md); then a whole forward + input gradient of DenseNet-121 with `own_dense_pointwise` alone
(the code path as it was: the baseline) and with `own_dense_conv` next to it, in alternating rounds.  Writes one JSON
document (default profiles/dense3x3_bench.json) and prints it.

usage: python tools/bench_dense3x3.py [--batch 512] [--rounds 5] [--iters 10] [--net-rounds 5] [--net-iters 2] [--out PATH]
       --only kernels|network restricts the run, --variants off,on the network part"""
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

from bench_dense1x1 import COPY_TB_PER_S, random_bn_checkpoint  # noqa: E402
from bench_depthwise import events_us, forward_and_gradient, stats, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import _lib, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402


def network_shapes():
    """(C, N, H = W, how many of the 58 layers have the shape) from the network itself."""
    shapes, h = [], 56
    net = zoo.DenseNet(num_classes=8)
    for name, m in net.features.named_children():
        if name.startswith("denseblock"):
            convs = {(lay.conv2.in_channels, lay.conv2.out_channels) for lay in m.values()}
            assert len(convs) == 1
            shapes.append((*convs.pop(), h, len(m)))
        elif name.startswith("transition"):
            h //= 2
    assert sum(s[3] for s in shapes) == 58
    return shapes


def bench_kernels(args, dev):
    lib = _lib.load()
    out = []
    b = args.batch
    for c, n, hw, count in network_shapes():
        m = b * hw * hw
        gen = torch.Generator().manual_seed(c + n + hw)
        x = torch.randn(b, hw, hw, c, generator=gen).bfloat16().to(dev)                      # NHWC storage
        g = torch.randn(b, hw, hw, n, generator=gen).bfloat16().to(dev)
        w = (torch.randn(n, c, 3, 3, generator=gen) * (9 * c) ** -0.5).bfloat16()
        wf, wb = (t.to(dev) for t in ops.pack_conv3x3_weights(w))
        y = torch.empty(b, hw, hw, n, dtype=torch.bfloat16, device=dev)
        gx = torch.empty(b, hw, hw, c, dtype=torch.bfloat16, device=dev)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)                                        # channels_last NCHW view
        gt = g.permute(0, 3, 1, 2)
        w4 = w.to(dev).contiguous(memory_format=torch.channels_last)
        yl = F.conv2d(xt, w4, padding=1)
        st = ops._stream()
        P = ops._ptr
        fns = {
            "own_fwd": lambda: lib.adil_dense3x3_fwd(P(x), P(wf), P(y), b, hw, hw, c, n, st),
            "lib_fwd": lambda: F.conv2d(xt.detach(), w4, padding=1),
            "own_bwd": lambda: lib.adil_dense3x3_bwd(P(g), P(wb), P(gx), b, hw, hw, c, n, st),
            "lib_bwd": lambda: torch.autograd.grad(yl, xt, gt, retain_graph=True),
        }
        for fn in fns.values():                                                                 # library find / warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # agreement of the two paths on this shape
        df = float((y.float() - yl.detach().permute(0, 2, 3, 1).float()).abs().max())
        (gl,) = torch.autograd.grad(yl, xt, gt, retain_graph=True)
        db = float((gx.float() - gl.permute(0, 2, 3, 1).float()).abs().max())
        times = {key: [] for key in fns}
        for _ in range(args.rounds):
            for key, fn in fns.items():
                times[key].append(events_us(fn, args.iters))
        by = 2.0 * m * (c + n)                                                                 # x + y forward, g + gx backward
        us = {key: stats(t, by) for key, t in times.items()}
        for key in us:
            us[key]["fraction_of_copy_yardstick"] = round(us[key]["algorithmic_tb_per_s_at_median"] / COPY_TB_PER_S, 3)
        out.append({"C": c, "N": n, "H": hw, "W": hw, "B": b, "layers_of_this_shape": count,
                    "algorithmic_mbytes": round(by / 1e6, 1), "gflop": round(2.0 * m * 9 * c * n / 1e9, 1),
                    "max_abs_diff_own_vs_library": {"fwd": df, "bwd": db}, "us": us,
                    "loses_to_the_library": [d for d in ("fwd", "bwd") if us["own_" + d]["median"] > us["lib_" + d]["median"]]})
        print(json.dumps(out[-1]), flush=True)
        del x, g, y, gx, xt, gt, yl, gl
        torch.cuda.empty_cache()
    tot = {key: round(sum(r["us"][key]["median"] * r["layers_of_this_shape"] for r in out) / 1e3, 3)
           for key in ("own_fwd", "lib_fwd", "own_bwd", "lib_bwd")}
    return {"shapes": out, "ms_weighted_by_layer_count_at_median": tot,
            "layers_that_lose_to_the_library": [(r["C"], r["N"], r["H"], d) for r in out for d in r["loses_to_the_library"]]}


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_d3_"), "densenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {v: zoo.build_classifier("densenet121", dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True,
                                      own_dense_conv=(v == "on"), **kw) for v in args.variants.split(",")}
    out = {"what": "DenseNet-121 bf16 channels_last with own_dense_pointwise, %d structured images at 224 x 224, forward + input "
                   "gradient of sum(logits^2); own_dense_conv off (the code path as it was: the baseline) / on, alternating "
                   "rounds of %d passes" % (b, args.net_iters)}
    ref = zoo.build_classifier("densenet121", **kw)
    xs = images[:16].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    rms = float(lr.square().mean().sqrt())
    acc = {}
    for v, model in models.items():
        l, g = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((l - lr).abs().mean()),
                  "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_16_images"] = {"rms_logit": rms, "bf16_depth_bound_121_layers": 2.0 * 2.0 ** -9 * 121 ** 0.5 * rms,
                                                    **acc}
    del ref, lr, gr
    x = images.to(dev).bfloat16()

    def one(v):
        xi = x.detach().requires_grad_(True)
        logits = models[v](xi).float()
        torch.autograd.grad(logits.square().sum(), xi)

    for v in models:
        for _ in range(2):
            one(v)
    torch.cuda.synchronize()
    times = {v: [] for v in models}
    for _ in range(args.net_rounds):
        for v in models:
            times[v].append(events_us(lambda: one(v), args.net_iters) / 1e3)
    out["ms_per_pass"] = {v: {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                              "spread": round(max(t) - min(t), 3), "rounds": [round(u, 3) for u in t]} for v, t in times.items()}
    if "off" in times and "on" in times:
        d, w = out["ms_per_pass"]["off"], out["ms_per_pass"]["on"]
        out["switch_on_against_off"] = {"gain_ms_at_median": round(d["median"] - w["median"], 3),
                                        "larger_spread_ms": max(d["spread"], w["spread"]),
                                        "every_on_round_beats_every_off_round": bool(w["max"] < d["min"])}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=2)
    p.add_argument("--only", choices=["kernels", "network"], default=None)
    p.add_argument("--variants", default="off,on", help="network part: any of off, on")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense3x3_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_dense3x3_fwd / _bwd vs F.conv2d 3x3 / pad 1 and its autograd input gradient (channels_last bf16), one "
                   "process, alternating rounds, device events; microseconds per call; fractions are algorithmic bytes / time "
                   "over the %.1f TB/s copy yardstick" % COPY_TB_PER_S,
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
