"""The two main loops of the 3x3 convolution kernels (adil_conv3x3_loop: 1 = the step loop of the parent, 0 = unrolled
taps with pipelined LDS reads) timed in ONE process, alternating, warmed up, with device events: the four stride-1 shapes of
ResNet-50 at B = 512 on the forward and on the flipped (input gradient) packing, and the three stride-2 shapes (plus the
three of ResNet-18, which reach the 64-channel stride-2 tile) in both directions; then one whole learning step of the
headline shape (ResNet-50, 512 images, 50 atoms, bf16 streams, cached labels) under either loop, alternating.  Inputs
and outputs rotate over enough buffers (--rotate-mb of them) that no
launch finds its operands in the 256 MB Infinity Cache.  Every row reports microseconds, TFLOP/s and the fraction of the
MFMA time of its FLOPs (--mfma-tflops, the dense bf16 rate: 118 GFLOP take 47 us).  Writes one JSON document (default
profiles/conv3x3_loop_bench.json) and prints it.

usage: python tools/bench_conv3x3_loop.py [--batch 512] [--rounds 5] [--iters 10] [--step-rounds 5] [--steps 8] [--out PATH]
       --only kernels|step restricts the run, --variants 1,0 names the loops to alternate (a kernel trace wants one:
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_conv3x3_loop.py --only step
       --variants 0 --step-rounds 1 --steps 4 --out /dev/null, then tools/step_breakdown.py DIR)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dl_attack_on_imagenet_amd import _lib, engine, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

# (name, H = W, C = N): conv2 of the bottlenecks of the four stages
S1 = [("layer1.conv2", 56, 64), ("layer2.conv2", 28, 128), ("layer3.conv2", 14, 256), ("layer4.conv2", 7, 512)]
# (name, input H = W, C, N): conv2 of the first bottleneck of stages 2-4, and conv1 of the same BasicBlocks of ResNet-18 (not
# part of the headline step: the gradient of the first one is the only launch here on the 64-channel stride-2 tile)
S2 = [("layer2.0.conv2", 56, 128, 128), ("layer3.0.conv2", 28, 256, 256), ("layer4.0.conv2", 14, 512, 512),
      ("resnet18.layer2.0.conv1", 56, 64, 128), ("resnet18.layer3.0.conv1", 28, 128, 256), ("resnet18.layer4.0.conv1", 14, 256, 512)]


def events_us(fns, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stats(ts, flop, mfma_tflops):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"median": round(med, 2), "min": round(s[0], 2), "max": round(s[-1], 2), "rounds": [round(t, 2) for t in ts],
            "tflops_at_median": round(flop / med / 1e6, 1), "fraction_of_mfma_time": round(flop / (mfma_tflops * 1e6) / med, 3)}


def rows_of(args, dev):
    """(row name, flop, list of rotating launch closures)."""
    lib, b, st = _lib.load(), args.batch, ops._stream()
    p = ops._ptr
    for name, hw, c in S1:
        gen = torch.Generator().manual_seed(hw + c)
        wf, wb = ops.pack_conv3x3_weights((torch.randn(c, c, 3, 3, generator=gen) / (9 * c) ** 0.5).to(dev))
        m = b * hw * hw
        nbuf = max(2, -(-args.rotate_mb * (1 << 20) // (2 * m * c * 2)))
        xs = [torch.randn(m, c, device=dev).bfloat16() for _ in range(nbuf)]
        ys = [torch.empty(m, c, dtype=torch.bfloat16, device=dev) for _ in range(nbuf)]
        for tag, wp in (("fwd", wf), ("flipped", wb)):
            fns = [(lambda x=x, y=y, wp=wp: lib.adil_conv3x3(p(x), p(wp), p(y), b, hw, hw, c, c, st)) for x, y in zip(xs, ys)]
            yield "s1 %s %dx%dx%d %s" % (name, hw, hw, c, tag), 2.0 * m * c * c * 9, fns
        del xs, ys
        torch.cuda.empty_cache()
    for name, hw, c, n in S2:
        gen = torch.Generator().manual_seed(hw + c + n + 1)
        wf, wb = ops.pack_conv3x3_s2_weights((torch.randn(n, c, 3, 3, generator=gen) / (9 * c) ** 0.5).to(dev))
        m4, m = b * hw * hw, b * hw * hw // 4
        nbuf = max(2, -(-args.rotate_mb * (1 << 20) // ((m4 * c + m * n) * 2)))
        big = [torch.randn(m4, c, device=dev).bfloat16() for _ in range(nbuf)]
        small = [torch.randn(m, n, device=dev).bfloat16() for _ in range(nbuf)]
        fwd = [(lambda x=x, y=y: lib.adil_conv3x3_s2_fwd(p(x), p(wf), p(y), b, hw, hw, c, n, st)) for x, y in zip(big, small)]
        yield "s2 %s %dx%dx%d->%d fwd" % (name, hw, hw, c, n), 2.0 * m * c * n * 9, fwd
        bwd = [(lambda g=g, gx=gx: lib.adil_conv3x3_s2_bwd(p(g), p(wb), p(gx), b, hw, hw, c, n, st)) for g, gx in zip(small, big)]
        yield "s2 %s %dx%dx%d->%d bwd" % (name, hw, hw, c, n), 2.0 * m * c * n * 9, bwd
        del big, small
        torch.cuda.empty_cache()


def bench_kernels(args, dev, variants):
    lib = _lib.load()
    res = []
    prev = lib.adil_conv3x3_loop(-1)
    try:
        for name, flop, fns in rows_of(args, dev):
            for v in variants:
                lib.adil_conv3x3_loop(v)
                for fn in fns:
                    assert fn() == 0
            torch.cuda.synchronize()
            times = {v: [] for v in variants}
            for _ in range(args.rounds):
                for v in variants:
                    lib.adil_conv3x3_loop(v)
                    times[v].append(events_us(fns, args.iters))
            res.append({"row": name, "gflop": round(flop / 1e9, 2), "buffers": len(fns),
                        "us": {str(v): stats(t, flop, args.mfma_tflops) for v, t in times.items()}})
            print(json.dumps(res[-1]), flush=True)
    finally:
        lib.adil_conv3x3_loop(prev)
    return res


def bench_step(args, dev, variants):
    lib = _lib.load()
    b, k, eps = args.batch, 50, 8 / 255
    shape = (3, 224, 224)
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(b, *shape, generator=gen).to(dev).bfloat16()
    model = zoo.build_classifier("resnet50", seed=0, device=dev, dtype=torch.bfloat16, channels_last=True, fuse_bn_act=True,
                                 fuse_stem=True, head_fp32="inference")
    d0 = -1 + 2 * torch.rand(*shape, k, generator=gen)
    v0 = torch.rand(b, k, generator=gen)
    learner = engine.DictionaryLearner(d0.to(dev), ops.l1ball_project_(v0.to(dev), eps), eps, 0.01, "logits", False, 50.0)
    cache = engine.LabelCache(b, dev)
    index, rows = torch.arange(b, device=dev), list(range(b))
    prev = lib.adil_conv3x3_loop(-1)
    times = {v: [] for v in variants}
    try:
        for v in variants:
            lib.adil_conv3x3_loop(v)
            for _ in range(4):
                learner.step(model, x, index, cache.get(model, x, index, rows))
        torch.cuda.synchronize()
        for _ in range(args.step_rounds):
            for v in variants:
                lib.adil_conv3x3_loop(v)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    learner.step(model, x, index, cache.get(model, x, index, rows))
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) / args.steps * 1e3)
    finally:
        lib.adil_conv3x3_loop(prev)
    return {"what": "learning step, resnet50 bf16, %d images, 50 atoms, cached labels; adil_conv3x3_loop 1 = the parent's "
                    "loop, 0 = the new loop; alternating rounds of %d steps" % (b, args.steps),
            "ms_per_step": {str(v): {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                                     "rounds": [round(u, 3) for u in t]} for v, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rotate-mb", type=int, default=1024, help="bytes of operands a row rotates over, at least")
    ap.add_argument("--mfma-tflops", type=float, default=2516.6, help="dense bf16 MFMA rate the fraction column refers to")
    ap.add_argument("--only", choices=["kernels", "step"], default=None)
    ap.add_argument("--variants", default="1,0", help="loops to alternate (a trace wants one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv3x3_loop_bench.json"))
    args = ap.parse_args()
    variants = [int(s) for s in args.variants.split(",")]
    dev = torch.device("cuda", 0)
    out = {"what": "adil_conv3x3 / adil_conv3x3_s2_fwd / _bwd under adil_conv3x3_loop 1 (the parent's loop) and 0 (the new loop), "
                   "one process, alternating rounds, device events, operands rotating past the Infinity Cache; microseconds per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "iters_per_round": args.iters, "mfma_tflops": args.mfma_tflops}
    if args.only != "step":
        out["kernels"] = bench_kernels(args, dev, variants)
    if args.only != "kernels":
        out["learning_step"] = bench_step(args, dev, variants)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
