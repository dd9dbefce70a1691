"""The output-channel tiles of the pointwise input gradient (adil_pw_conv_bwd_tile at bo = 64 / 128, the parent's tiles,
against the wide bo = 256 and 512) on the gradient launches of ResNet-50 at B = 512: the twelve stride-1 shapes of
tools/exp_pw.py and the two downsample gradients of stages 3 and 4, each with the flags the network passes (conv3
gradients: g2, gres and the xin epilogue; conv1 gradients: the ReLU mask only; downsample gradients: no ReLU), timed in ONE
process, the tiles alternating, warmed up, with device events.  Then one whole learning step of the headline shape
(ResNet-50, 512 images, 50 atoms, bf16 streams, cached labels) under the routing policies of adil_pw_route_policy
(1 = the parent's tiles everywhere, 0 = the table in adil_convs.hip, 2 = the widest covering tile everywhere), alternating.
The routing rule the table follows: a shape goes wide only if its median beats the parent tile's median by more than the
parent tile's own max - min over its rounds (`passes_rule` below).
Writes one JSON document (default profiles/pw_wide_bench.json) and prints it.

usage: python tools/bench_pw_wide.py [--batch 512] [--rounds 5] [--iters 10] [--step-rounds 5] [--steps 8] [--out PATH]
       --only kernels|step restricts the run, --policies 1,0 the learning step (a kernel trace wants one policy:
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_pw_wide.py --only step --policies 0
       --step-rounds 1 --steps 4 --out /dev/null, then tools/step_breakdown.py)"""
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

WIDE = (256, 512)
# (layer, launches per step, H = W, K = gradient's output channels (Cin), N = reduction (Cout), kind)
#   kind "conv3": g2 + gres + xin + relu;  "conv1": relu only;  "down": nothing (no ReLU behind a downsample BatchNorm)
SHAPES = [("layer1 conv1 first", 1, 56, 64, 64, "conv1"), ("layer1 conv3", 4, 56, 64, 256, "conv3"),
          ("layer1 conv1", 2, 56, 256, 64, "conv1"), ("layer2.0 conv1", 1, 56, 256, 128, "conv1"),
          ("layer2 conv3", 4, 28, 128, 512, "conv3"), ("layer2 conv1", 3, 28, 512, 128, "conv1"),
          ("layer3.0 conv1", 1, 28, 512, 256, "conv1"), ("layer3 conv3", 6, 14, 256, 1024, "conv3"),
          ("layer3 conv1", 5, 14, 1024, 256, "conv1"), ("layer4.0 conv1", 1, 14, 1024, 512, "conv1"),
          ("layer4 conv3", 3, 7, 512, 2048, "conv3"), ("layer4 conv1", 2, 7, 2048, 512, "conv1"),
          ("layer3.0 downsample", 1, 14, 512, 1024, "down"), ("layer4.0 downsample", 1, 7, 1024, 2048, "down")]


def events_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stats(ts):
    s = sorted(ts)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2), "rounds": [round(t, 2) for t in ts]}


def bench_kernels(args, dev):
    lib = _lib.load()
    res = []
    p, st = ops._ptr, ops._stream()
    for name, count, hw, k, n, kind in SHAPES:
        m = args.batch * hw * hw
        bf = lambda *s, sc=1.0: (torch.randn(*s, device=dev) * sc).bfloat16()
        g, y, wt = bf(m, n), torch.relu(bf(m, n)), bf(k, n, sc=n ** -0.5)
        scale = 0.5 + torch.rand(n, device=dev)
        c3 = kind == "conv3"
        g2 = bf(m, n) if c3 else None
        gres = torch.empty(m, n, dtype=torch.bfloat16, device=dev) if c3 else None
        xin = bf(m, k) if c3 else None
        ps, pb = (0.5 + torch.rand(k, device=dev), torch.randn(k, device=dev) * 0.3) if c3 else (None, None)
        relu = 0 if kind == "down" else 1
        gx = torch.empty(m, k, dtype=torch.bfloat16, device=dev)
        parent = 128 if k % 128 == 0 else 64
        tiles = [parent] + [bo for bo in WIDE if k % bo == 0]

        def call(bo):
            rc = lib.adil_pw_conv_bwd_tile(p(g), p(g2), p(y), p(scale), p(wt), p(gx), p(gres), m, k, n, relu, p(xin), p(ps),
                                           p(pb), None, 0, 0, st, bo)
            assert rc == 0, (name, bo, rc)

        same = {}
        for bo in tiles:                                                     # warm-up, and the bits of each tile
            for _ in range(3):
                call(bo)
            torch.cuda.synchronize()
            same[bo] = (gx.clone(), gres.clone() if c3 else None)
        for bo in tiles[1:]:
            assert torch.equal(same[bo][0].view(torch.int16), same[parent][0].view(torch.int16)), (name, bo)
            assert not c3 or torch.equal(same[bo][1].view(torch.int16), same[parent][1].view(torch.int16)), (name, bo)
        del same
        times = {bo: [] for bo in tiles}
        for _ in range(args.rounds):
            for bo in tiles:
                times[bo].append(events_us(lambda: call(bo), args.iters))
        us = {str(bo): stats(t) for bo, t in times.items()}
        pm = us[str(parent)]
        byt = 2 * (m * n * (4 if c3 else (2 if relu else 1)) + m * k * (2 if c3 else 1) + n * k)
        row = {"layer": name, "launches_per_step": count, "M": m, "K": k, "N": n, "kind": kind, "parent_tile": parent,
               "gflop": round(2.0 * m * n * k / 1e9, 2), "hbm_mb": round(byt / 1e6, 1), "us": us,
               "parent_tb_per_s": round(byt / pm["median"] / 1e6, 2), "parent_tflops": round(2.0 * m * n * k / pm["median"] / 1e6, 1),
               "passes_rule": {str(bo): bool(pm["median"] - us[str(bo)]["median"] > pm["max"] - pm["min"]) for bo in tiles[1:]}}
        res.append(row)
        print(json.dumps(row), flush=True)
        del g, y, wt, g2, gres, xin, gx
        torch.cuda.empty_cache()
    return res


def bench_step(args, dev):
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
    policies = [int(s) for s in args.policies.split(",")]
    prev = lib.adil_pw_route_policy(-1)
    times = {q: [] for q in policies}
    try:
        for q in policies:
            lib.adil_pw_route_policy(q)
            for _ in range(4):
                learner.step(model, x, index, cache.get(model, x, index, rows))
        torch.cuda.synchronize()
        for _ in range(args.step_rounds):
            for q in policies:
                lib.adil_pw_route_policy(q)
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    learner.step(model, x, index, cache.get(model, x, index, rows))
                torch.cuda.synchronize()
                times[q].append((time.perf_counter() - t0) / args.steps * 1e3)
    finally:
        lib.adil_pw_route_policy(prev)
    return {"what": "learning step, resnet50 bf16, %d images, 50 atoms, cached labels; adil_pw_route_policy 1 = parent tiles, "
                    "0 = table, 2 = widest covering tile; alternating rounds of %d steps" % (b, args.steps),
            "ms_per_step": {str(q): {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                                     "rounds": [round(v, 3) for v in t]} for q, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--only", choices=["kernels", "step"], default=None)
    ap.add_argument("--policies", default="1,0", help="learning step: routing policies to alternate (a trace wants one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pw_wide_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_pw_conv_bwd_tile at the parent tile (128, or 64 where K % 128) and at the wide tiles (256, 512) on the "
                   "pointwise gradient launches of ResNet-50, one process, alternating rounds, device events; microseconds per call",
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
