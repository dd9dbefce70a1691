"""The two forms of the stem backward kernels (adil_stem_bwd_variant: 1 = the parent's gather-form un-pooling and
class-form 7x7 input gradient, 0 = the quad and shift forms) timed in ONE process, alternating, warmed up, with device
events: adil_stem_pool_bwd (B x 112 x 112 x 64) and adil_stem_conv_bwd (B x 3 x 224 x 224, bf16 gx) at B = 512, 128 and 64;
then one whole learning step of the headline shape (ResNet-50, 512 images, 50 atoms, bf16 streams, cached labels) under
either value, alternating.  Operands rotate over enough buffers (--rotate-mb of them) that no launch finds them in the
256 MB Infinity Cache.  p and idx come from adil_maxpool_fwd of a relu(gaussian) activation, g_y1 from the un-pooling
itself.  Every kernel row reports microseconds and the HBM bytes of the call over them.  Writes one JSON document
(default profiles/stem_bwd_variants.json) and prints it.

usage: python tools/bench_stem_bwd.py [--batches 512,128,64] [--rounds 5] [--iters 10] [--step-rounds 5] [--steps 8] [--out PATH]
       --only kernels|step restricts the run, --variants 1,0 names the values to alternate (a kernel trace wants one:
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_stem_bwd.py --only step
       --variants 0 --step-rounds 1 --steps 4 --out /dev/null, then tools/step_breakdown.py DIR)"""
import argparse
import json
import os
import sys
import time
from ctypes import c_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dl_attack_on_imagenet_amd import _lib, engine, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

H = W = 224
OH = OW = 112
PH = PW = 56
C = 64
BF16 = torch.bfloat16


def events_us(fns, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fns[i % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stats(ts, nbytes):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"median": round(med, 2), "min": round(s[0], 2), "max": round(s[-1], 2), "rounds": [round(t, 2) for t in ts],
            "tb_per_s_at_median": round(nbytes / med / 1e6, 2)}


def rows_of(args, dev, b):
    """(row name, HBM bytes of one call, list of rotating launch closures) for one batch size."""
    lib, st, p = _lib.load(), ops._stream(), ops._ptr
    pool_bytes = b * PH * PW * C * (2 + 2 + 1) + b * OH * OW * C * 2
    conv_bytes = b * OH * OW * C * 2 + b * 3 * H * W * 2
    nbuf = max(2, -(-args.rotate_mb * (1 << 20) // min(pool_bytes, conv_bytes)))
    gen = torch.Generator(device=dev).manual_seed(b)
    scale = (0.5 + torch.rand(C, generator=gen, device=dev)) * (torch.randint(0, 2, (C,), generator=gen, device=dev) * 2 - 1).float()
    wb = torch.zeros(4, 49, C, dtype=BF16, device=dev)
    wb[:3] = (torch.randn(3, 49, C, generator=gen, device=dev) * 147 ** -0.5).to(BF16)
    inv = [c_float(1 / s) for s in (0.229, 0.224, 0.225)]
    sets = []
    for _ in range(nbuf):
        y = torch.randn(b, OH, OW, C, generator=gen, device=dev).relu_().to(BF16)
        pp = torch.empty(b, PH, PW, C, dtype=BF16, device=dev)
        idx = torch.empty(b, PH, PW, C, dtype=torch.uint8, device=dev)
        assert lib.adil_maxpool_fwd(p(y), p(pp), p(idx), b, OH, OW, C, st) == 0
        g = torch.randn(b, PH, PW, C, generator=gen, device=dev).to(BF16)
        gx = torch.empty(b, 3, H, W, dtype=BF16, device=dev)
        sets.append((g, idx, pp, y, gx))                   # y becomes g_y1: the un-pooling overwrites every element
    torch.cuda.synchronize()
    pool = [(lambda s=s: lib.adil_stem_pool_bwd(p(s[0]), p(s[1]), p(s[2]), p(scale), p(s[3]), b, OH, OW, C, st)) for s in sets]
    yield "adil_stem_pool_bwd B=%d %dx%dx%d" % (b, OH, OW, C), pool_bytes, pool, sets
    conv = [(lambda s=s: lib.adil_stem_conv_bwd(p(s[3]), p(wb), *inv, p(s[4]), 1, b, H, W, st)) for s in sets]
    yield "adil_stem_conv_bwd B=%d 3x%dx%d bf16" % (b, H, W), conv_bytes, conv, sets


def bench_kernels(args, dev, variants):
    lib = _lib.load()
    res = []
    prev = lib.adil_stem_bwd_variant(-1)
    try:
        for b in args.batches:
            for name, nbytes, fns, _keep in rows_of(args, dev, b):
                for v in variants:
                    lib.adil_stem_bwd_variant(v)
                    for fn in fns:
                        assert fn() == 0
                torch.cuda.synchronize()
                times = {v: [] for v in variants}
                for _ in range(args.rounds):
                    for v in variants:
                        lib.adil_stem_bwd_variant(v)
                        times[v].append(events_us(fns, args.iters))
                res.append({"row": name, "hbm_mb": round(nbytes / 1e6, 1), "buffers": len(fns),
                            "us": {str(v): stats(t, nbytes) for v, t in times.items()}})
                print(json.dumps(res[-1]), flush=True)
            torch.cuda.empty_cache()
    finally:
        lib.adil_stem_bwd_variant(prev)
    return res


def bench_step(args, dev, variants):
    lib = _lib.load()
    b, k, eps = 512, 50, 8 / 255
    shape = (3, H, W)
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(b, *shape, generator=gen).to(dev).bfloat16()
    model = zoo.build_classifier("resnet50", seed=0, device=dev, dtype=BF16, channels_last=True, fuse_bn_act=True,
                                 fuse_stem=True, head_fp32="inference")
    d0 = -1 + 2 * torch.rand(*shape, k, generator=gen)
    v0 = torch.rand(b, k, generator=gen)
    learner = engine.DictionaryLearner(d0.to(dev), ops.l1ball_project_(v0.to(dev), eps), eps, 0.01, "logits", False, 50.0)
    cache = engine.LabelCache(b, dev)
    index, rows = torch.arange(b, device=dev), list(range(b))
    prev = lib.adil_stem_bwd_variant(-1)
    times = {v: [] for v in variants}
    try:
        for v in variants:
            lib.adil_stem_bwd_variant(v)
            for _ in range(4):
                learner.step(model, x, index, cache.get(model, x, index, rows))
        torch.cuda.synchronize()
        for _ in range(args.step_rounds):
            for v in variants:
                lib.adil_stem_bwd_variant(v)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    learner.step(model, x, index, cache.get(model, x, index, rows))
                torch.cuda.synchronize()
                times[v].append((time.perf_counter() - t0) / args.steps * 1e3)
    finally:
        lib.adil_stem_bwd_variant(prev)
    return {"what": "learning step, resnet50 bf16, %d images, 50 atoms, cached labels; adil_stem_bwd_variant 1 = the parent's "
                    "kernels, 0 = the new kernels; alternating rounds of %d steps" % (b, args.steps),
            "ms_per_step": {str(v): {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                                     "rounds": [round(u, 3) for u in t]} for v, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="512,128,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rotate-mb", type=int, default=1024, help="bytes of operands a row rotates over, at least")
    ap.add_argument("--only", choices=["kernels", "step"], default=None)
    ap.add_argument("--variants", default="1,0", help="values to alternate (a trace wants one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_bwd_variants.json"))
    args = ap.parse_args()
    args.batches = [int(s) for s in args.batches.split(",")]
    variants = [int(s) for s in args.variants.split(",")]
    dev = torch.device("cuda", 0)
    out = {"what": "adil_stem_pool_bwd / adil_stem_conv_bwd under adil_stem_bwd_variant 1 (the parent's kernels) and 0 (the new "
                   "kernels), one process, alternating rounds, device events, operands rotating past the Infinity Cache; "
                   "microseconds per call",
           "source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "iters_per_round": args.iters}
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
