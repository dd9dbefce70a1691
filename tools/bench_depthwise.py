"""The depthwise 3x3 kernels (adil_dw3x3_fwd / adil_dw3x3_bwd) against the calls they replace (F.conv2d(groups=C) with the
folded BatchNorm bias + hardtanh(0, 6), and their autograd input gradient, on channels_last bf16 tensors), timed in ONE
process, alternating, warmed up, with device events: the distinct (C, H, stride) depthwise shapes of MobileNetV2 at
224 x 224, B = 512, forward and input gradient; then a whole forward + input gradient of MobileNetV2 with
`own_depthwise` off / on, alternating, and the distance of both bf16 networks from the fp32 network (logits, input gradient)
on structured images.  Writes one JSON document (default profiles/depthwise_bench.json) and prints it.

usage: python tools/bench_depthwise.py [--batch 512] [--rounds 5] [--iters 10] [--net-rounds 5] [--net-iters 4] [--out PATH]
       --only kernels|network restricts the run, --variants library|own the network part (a kernel trace wants them apart:
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_depthwise.py --only network
       --variants own --net-rounds 1 --net-iters 4 --out /dev/null, then tools/prof_summary.py DIR)"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dl_attack_on_imagenet_amd import _lib, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

# (C, input H = W, stride) and how many of the 17 depthwise layers have the shape
SHAPES = [(32, 112, 1, 1), (96, 112, 2, 1), (144, 56, 1, 1), (144, 56, 2, 1), (192, 28, 1, 2), (192, 28, 2, 1), (384, 14, 1, 4),
          (576, 14, 1, 2), (576, 14, 2, 1), (960, 7, 1, 3)]


def events_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stats(ts, nbytes=None):
    s = sorted(ts)
    out = {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2), "rounds": [round(t, 2) for t in ts]}
    if nbytes is not None:
        out["algorithmic_tb_per_s_at_median"] = round(nbytes / s[len(s) // 2] / 1e6, 2)
    return out


def bench_kernels(args, dev):
    lib = _lib.load()
    res = []
    b = args.batch
    for c, hw, s, count in SHAPES:
        oh = (hw - 1) // s + 1
        gen = torch.Generator().manual_seed(hw + c + s)
        x = torch.randn(b, hw, hw, c, generator=gen).bfloat16().to(dev)                      # NHWC storage
        g = torch.randn(b, oh, oh, c, generator=gen).bfloat16().to(dev)
        w = (torch.randn(c, 1, 3, 3, generator=gen) / 3.0).to(dev)
        bias = torch.randn(c, generator=gen).to(dev)
        w9c = ops.pack_dw3x3_weights(w)
        y = torch.empty(b, oh, oh, c, dtype=torch.bfloat16, device=dev)
        gx = torch.empty(b, hw, hw, c, dtype=torch.bfloat16, device=dev)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)                                        # channels_last NCHW view
        gt = g.permute(0, 3, 1, 2)
        wt, bt = w.bfloat16(), bias.bfloat16()

        def lib_fwd(xin=xt):
            return F.hardtanh(F.conv2d(xin, wt, bt, stride=s, padding=1, groups=c), 0.0, 6.0)

        yl = lib_fwd()
        st = ops._stream()
        fns = {
            "own_fwd": lambda: lib.adil_dw3x3_fwd(ops._ptr(x), ops._ptr(w9c), ops._ptr(bias), ops._ptr(y), b, hw, hw, c, s, 1, st),
            "lib_fwd": lambda: lib_fwd(xt.detach()),
            "own_bwd": lambda: lib.adil_dw3x3_bwd(ops._ptr(g), ops._ptr(y), ops._ptr(w9c), ops._ptr(gx), b, hw, hw, c, s, 1, st),
            "lib_bwd": lambda: torch.autograd.grad(yl, xt, gt, retain_graph=True),
        }
        for fn in fns.values():                                                                 # library find / warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # agreement of the two paths on this shape (the library path rounds its weights, bias and pre-activation to bf16)
        df = float((y.float() - yl.detach().permute(0, 2, 3, 1).float()).abs().max())
        (gl,) = torch.autograd.grad(yl, xt, gt, retain_graph=True)
        db = float((gx.float() - gl.permute(0, 2, 3, 1).float()).abs().max())
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(events_us(fn, args.iters))
        by_f = 2.0 * b * c * (hw * hw + oh * oh)
        by_b = 2.0 * b * c * (hw * hw + 2 * oh * oh)
        res.append({"C": c, "H": hw, "W": hw, "stride": s, "B": b, "layers_of_this_shape": count,
                    "algorithmic_mbytes": {"fwd": round(by_f / 1e6, 1), "bwd": round(by_b / 1e6, 1)},
                    "max_abs_diff_own_vs_library": {"fwd": df, "bwd": db},
                    "us": {k: stats(t, by_f if k.endswith("fwd") else by_b) for k, t in times.items()}})
        print(json.dumps(res[-1]), flush=True)
        del x, g, y, gx, xt, gt, yl, gl
        torch.cuda.empty_cache()
    tot = {k: round(sum(r["us"][k]["median"] * r["layers_of_this_shape"] for r in res) / 1e3, 3) for k in ("own_fwd", "lib_fwd", "own_bwd", "lib_bwd")}
    return {"shapes": res, "ms_over_the_17_layers_at_median": tot,
            "algorithmic_gbytes_over_the_17_layers": {
                "fwd": round(sum(r["algorithmic_mbytes"]["fwd"] * r["layers_of_this_shape"] for r in res) / 1e3, 2),
                "bwd": round(sum(r["algorithmic_mbytes"]["bwd"] * r["layers_of_this_shape"] for r in res) / 1e3, 2)}}


def structured_batch(n, size=224, classes=4, seed=3, noise=0.10, cells=7):
    """Noisy copies of a few coarse colour patterns: on iid noise images a random-weight MobileNetV2 gives every image the
    same logits and the comparison with the fp32 network would be empty."""
    g = torch.Generator().manual_seed(seed)
    protos = F.interpolate(torch.rand(classes, 3, cells, cells, generator=g), size=(size, size), mode="bilinear",
                           align_corners=False) * 0.6 + 0.2
    return (protos[torch.arange(n) % classes] + noise * torch.randn(n, 3, size, size, generator=g)).clamp_(0.0, 1.0)


def random_bn_checkpoint(path, dev, seed=0):
    """Seeded random MobileNetV2 with randomised BatchNorm statistics and affine maps (mean 0.2 N(0,1), var in [0.6, 1.4],
    gamma in [0.7, 1.3], beta 0.2 N(0,1)), so that the folded tables differ from the plain weights.  The network of
    tests/test_gpu_depthwise.py: tame in bf16 (its logits are dominated by the biases; the input gradient is what depends
    on the input)."""
    model = zoo.build_classifier("mobilenet", seed=seed, device=dev)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_(0.7 + 0.6 * torch.rand(n, generator=gen))
                m.bias.copy_(0.2 * torch.randn(n, generator=gen))
                m.running_mean.copy_(0.2 * torch.randn(n, generator=gen))
                m.running_var.copy_(0.6 + 0.8 * torch.rand(n, generator=gen))
    torch.save({k: v.cpu() for k, v in model[1].state_dict().items()}, path)
    return path


def forward_and_gradient(model, x):
    x = x.clone().requires_grad_(True)
    logits = model(x).float()
    (g,) = torch.autograd.grad(logits.square().sum(), x)
    return logits.detach(), g.detach().float()


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_dw_"), "mobilenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {m: zoo.build_classifier("mobilenet", dtype=torch.bfloat16, channels_last=True, own_depthwise=(m == "own"), **kw)
              for m in args.variants.split(",")}
    out = {"what": "MobileNetV2 bf16 channels_last, %d structured images at 224 x 224, forward + input gradient of "
                   "sum(logits^2); own_depthwise off (library) / on (own), alternating rounds of %d passes" % (b, args.net_iters)}
    # distance from the fp32 network on 32 images
    ref = zoo.build_classifier("mobilenet", **kw)
    xs = images[:32].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    rms = float(lr.square().mean().sqrt())
    acc = {}
    for m, model in models.items():
        l, g = forward_and_gradient(model, xs.bfloat16())
        acc[m] = {"mean_abs_logit_error": float((l - lr).abs().mean()), "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_32_images"] = {"rms_logit": rms, "logit_spread_over_images": float(lr.std(dim=0).mean()),
                                                    "bf16_depth_bound_53_layers": 2.0 * 2.0 ** -9 * 53 ** 0.5 * rms, **acc}
    del ref, lr, gr
    x = images.to(dev).bfloat16()

    def one(m):
        xi = x.detach().requires_grad_(True)
        logits = models[m](xi).float()
        torch.autograd.grad(logits.square().sum(), xi)

    for m in models:
        for _ in range(3):
            one(m)
    torch.cuda.synchronize()
    times = {m: [] for m in models}
    for _ in range(args.net_rounds):
        for m in models:
            times[m].append(events_us(lambda: one(m), args.net_iters) / 1e3)
    out["ms_per_pass"] = {m: {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                              "rounds": [round(v, 3) for v in t]} for m, t in times.items()}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=4)
    p.add_argument("--only", choices=["kernels", "network"], default=None)
    p.add_argument("--variants", default="library,own", help="network part: library, own or both (a trace wants one)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthwise_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_dw3x3_fwd / _bwd vs F.conv2d(groups=C) + folded bias + hardtanh(0, 6) and their autograd input gradient "
                   "(channels_last bf16), one process, alternating rounds, device events; microseconds per call",
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
