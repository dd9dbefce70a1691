"""The stride-2 3x3 convolution kernels (adil_conv3x3_s2_fwd / adil_conv3x3_s2_bwd) against the library call they replace
(F.conv2d(stride=2, padding=1) and its input gradient on channels_last bf16 tensors, the library's own zero-fill launches
included), timed in ONE process, alternating, warmed up, with device events: the three ResNet-50 shapes and the three
ResNet-18 shapes at B = 512, forward and input gradient; then one whole learning step of the headline shape (ResNet-50,
512 images, 50 atoms, bf16 streams, cached labels) with FusedResNet(own_strided_conv=False / True), alternating.
Writes one JSON document (default profiles/conv_s2_bench.json) and prints it.

usage: python tools/bench_conv_s2.py [--batch 512] [--rounds 5] [--iters 10] [--step-rounds 5] [--steps 8] [--out PATH]
       --only kernels|step restricts the run, --variants library|own the learning step (a kernel trace wants them apart:
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_conv_s2.py --only step --variants own
       --step-rounds 1 --steps 4 --out /dev/null, then tools/prof_summary.py DIR)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dl_attack_on_imagenet_amd import _lib, engine, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

# (name, input H = W, C, N)
SHAPES = [("resnet50.layer2.0.conv2", 56, 128, 128), ("resnet50.layer3.0.conv2", 28, 256, 256),
          ("resnet50.layer4.0.conv2", 14, 512, 512), ("resnet18.layer2.0.conv1", 56, 64, 128),
          ("resnet18.layer3.0.conv1", 28, 128, 256), ("resnet18.layer4.0.conv1", 14, 256, 512)]


def events_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stats(ts, flop=None):
    s = sorted(ts)
    out = {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2), "rounds": [round(t, 2) for t in ts]}
    if flop is not None:
        out["tflops_at_median"] = round(flop / s[len(s) // 2] / 1e6, 1)
    return out


def bench_kernels(args, dev):
    lib = _lib.load()
    res = []
    b = args.batch
    for name, hw, c, n in SHAPES:
        oh = hw // 2
        gen = torch.Generator().manual_seed(hw + c + n)
        x = torch.randn(b, hw, hw, c, generator=gen).bfloat16().to(dev)                      # NHWC storage
        g = torch.randn(b, oh, oh, n, generator=gen).bfloat16().to(dev)
        w = (torch.randn(n, c, 3, 3, generator=gen) / (9 * c) ** 0.5).to(dev)
        wf, wb = ops.pack_conv3x3_s2_weights(w)
        y = torch.empty(b * oh * oh, n, dtype=torch.bfloat16, device=dev)
        gx = torch.empty(b * hw * hw, c, dtype=torch.bfloat16, device=dev)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)                                        # channels_last NCHW view
        gt = g.permute(0, 3, 1, 2)
        wt = w.bfloat16().contiguous(memory_format=torch.channels_last)
        yl = F.conv2d(xt, wt, stride=2, padding=1)
        st = ops._stream()
        fns = {
            "own_fwd": lambda: lib.adil_conv3x3_s2_fwd(ops._ptr(x), ops._ptr(wf), ops._ptr(y), b, hw, hw, c, n, st),
            "lib_fwd": lambda: F.conv2d(xt.detach(), wt, stride=2, padding=1),
            "own_bwd": lambda: lib.adil_conv3x3_s2_bwd(ops._ptr(g), ops._ptr(wb), ops._ptr(gx), b, hw, hw, c, n, st),
            "lib_bwd": lambda: torch.autograd.grad(yl, xt, gt, retain_graph=True),
        }
        for fn in fns.values():                                                                 # library find / warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # agreement of the two paths on this shape (both within the bf16 bound of the fp32 result, see the tests)
        df = float((y.float() - yl.detach().permute(0, 2, 3, 1).reshape(-1, n).float()).abs().max())
        (gl,) = torch.autograd.grad(yl, xt, gt, retain_graph=True)
        db = float((gx.float() - gl.permute(0, 2, 3, 1).reshape(-1, c).float()).abs().max())
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(events_us(fn, args.iters))
        flop = 2.0 * b * oh * oh * n * c * 9
        res.append({"layer": name, "B": b, "H": hw, "W": hw, "C": c, "N": n, "gflop": round(flop / 1e9, 2),
                    "max_abs_diff_own_vs_library": {"fwd": df, "bwd": db},
                    "us": {k: stats(t, flop) for k, t in times.items()}})
        print(json.dumps(res[-1]), flush=True)
        del x, g, y, gx, xt, gt, yl, gl
        torch.cuda.empty_cache()
    return res


def bench_step(args, dev):
    b, k, eps, n = args.batch, 50, 8 / 255, 2 * args.batch
    shape = (3, 224, 224)
    gen = torch.Generator().manual_seed(3)
    images = torch.rand(n, *shape, generator=gen).to(dev).bfloat16()
    kw = dict(seed=0, device=dev, dtype=torch.bfloat16, channels_last=True, fuse_bn_act=True, fuse_stem=True,
              head_fp32="inference")
    models = {m: zoo.build_classifier("resnet50", own_strided_conv=(m == "own"), **kw) for m in args.variants.split(",")}
    d0 = -1 + 2 * torch.rand(*shape, k, generator=gen)
    v0 = torch.rand(n, k, generator=gen)
    learners = {m: engine.DictionaryLearner(d0.to(dev), ops.l1ball_project_(v0.to(dev), eps), eps, 0.01, "logits", False, 50.0)
                for m in models}
    caches = {m: engine.LabelCache(n, dev) for m in models}
    order = [list(range(i, i + b)) for i in range(0, n, b)]
    at = {m: 0 for m in models}

    def step(m):
        rows = order[at[m] % len(order)]
        at[m] += 1
        index = torch.tensor(rows, device=dev)
        x = images[rows[0]:rows[0] + b]
        return learners[m].step(models[m], x, index, caches[m].get(models[m], x, index, rows))

    for m in models:
        for _ in range(max(3, len(order)) + 1):
            step(m)
    torch.cuda.synchronize()
    times = {m: [] for m in models}
    for _ in range(args.step_rounds):
        for m in models:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(m)
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) / args.steps * 1e3)
    return {"what": "learning step, resnet50 bf16, %d images, 50 atoms, cached labels; FusedResNet own_strided_conv off "
                    "(library) / on (own), alternating rounds of %d steps" % (b, args.steps),
            "ms_per_step": {m: {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                                "rounds": [round(x, 3) for x in t]} for m, t in times.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--step-rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--only", choices=["kernels", "step"], default=None)
    p.add_argument("--variants", default="library,own", help="learning step: library, own or both (a trace wants one)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_s2_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_conv3x3_s2_fwd / _bwd vs F.conv2d(stride=2, padding=1) and its input gradient (channels_last bf16), "
                   "one process, alternating rounds, device events; microseconds per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "iters_per_round": args.iters}
    if args.only != "step":
        out["kernels"] = bench_kernels(args, dev)
    if args.only != "kernels":
        out["learning_step"] = bench_step(args, dev)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
