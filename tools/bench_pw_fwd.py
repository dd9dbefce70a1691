"""The output-channel tiles of the pointwise forward (adil_pw_conv_fwd_tile at bn = 128 / 64, the narrow tiles, against the
wide bn = 256 and 512) on the 15 distinct forward calls of the non-joined ResNet-50 pointwise layers, each with the flags
the network passes (conv3: prologue + residual; conv1: plain; downsample: no ReLU, the stride-2 gather behind stage 1),
timed in ONE process, the tiles alternating, warmed up, with device events, the operands rotating over more than 1 GB of
buffers so that no call finds its tensors in the Infinity Cache.  Then one whole learning step of the headline shape under
the routing policies of adil_pw_route_policy (tools/bench_pw_wide.py's bench_step), alternating.
The routing rule the table in adil_convs.hip follows: a shape goes wide only if its median beats the narrow tile's median
by more than the narrow tile's own max - min over its rounds (`passes_rule` below).
Writes one JSON document (default profiles/pw_fwd_bench.json) and prints it.

usage: python tools/bench_pw_fwd.py [--batch 512] [--rounds 5] [--iters 10] [--step-rounds 5] [--steps 8] [--out PATH]
       --only kernels|step restricts the run, --policies 1,0,2 the learning step (a kernel trace wants one policy:
       rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_pw_fwd.py --only step --policies 0
       --step-rounds 1 --steps 4 --out /dev/null, then tools/step_breakdown.py)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench_pw_wide import bench_step, events_us, stats  # noqa: E402  (tools/ is the script's directory)
from dl_attack_on_imagenet_amd import _lib, ops  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

WIDE = (256, 512)
# (layer, launches per step, output H = W, K = Cin, N = Cout, kind)
#   kind "conv3": prologue + residual + relu;  "conv1": relu only;  "down": no relu;  "gather": stride-2 gather, no relu
SHAPES = [("layer1.0 conv1", 1, 56, 64, 64, "conv1"), ("layer1.0 downsample", 1, 56, 64, 256, "down"),
          ("layer1.2 conv3", 1, 56, 64, 256, "conv3"), ("layer2.0 conv1", 1, 56, 256, 128, "conv1"),
          ("layer2.0 downsample", 1, 28, 256, 512, "gather"), ("layer2 conv3", 4, 28, 128, 512, "conv3"),
          ("layer2 conv1", 3, 28, 512, 128, "conv1"), ("layer3.0 conv1", 1, 28, 512, 256, "conv1"),
          ("layer3.0 downsample", 1, 14, 512, 1024, "gather"), ("layer3 conv3", 6, 14, 256, 1024, "conv3"),
          ("layer3 conv1", 5, 14, 1024, 256, "conv1"), ("layer4.0 conv1", 1, 14, 1024, 512, "conv1"),
          ("layer4.0 downsample", 1, 7, 1024, 2048, "gather"), ("layer4 conv3", 3, 7, 512, 2048, "conv3"),
          ("layer4 conv1", 2, 7, 2048, 512, "conv1")]
ROTATE_BYTES = 1.1e9                            # operand sets cover at least this much (Infinity Cache: 256 MB)


def bench_kernels(args, dev):
    lib = _lib.load()
    res = []
    p, st = ops._ptr, ops._stream()
    for name, count, hw, k, n, kind in SHAPES:
        m = args.batch * hw * hw
        gather, c3 = kind == "gather", kind == "conv3"
        relu = 1 if kind in ("conv1", "conv3") else 0
        sub_w, sub_hw = (hw, hw * hw) if gather else (0, 0)
        bf = lambda *s, sc=1.0: (torch.randn(*s, device=dev) * sc).bfloat16()
        w = bf(n, k, sc=k ** -0.5)
        scale, shift = 0.5 + torch.rand(n, device=dev), torch.randn(n, device=dev) * 0.3
        ps, pb = (0.5 + torch.rand(k, device=dev), torch.randn(k, device=dev) * 0.3) if c3 else (None, None)
        byt = 2 * (m * k + n * k + m * n * (2 if c3 else 1))                 # each tensor once (the gathered rows of x only)
        per_set = 2 * ((4 if gather else 1) * m * k + m * n * (2 if c3 else 1))
        nsets = max(2, int(ROTATE_BYTES // per_set) + 1)
        sets = [(bf((4 if gather else 1) * m, k), bf(m, n) if c3 else None,
                 torch.empty(m, n, dtype=torch.bfloat16, device=dev)) for _ in range(nsets)]
        narrow = 128 if n % 128 == 0 else 64
        tiles = [narrow] + [bn for bn in WIDE if n % bn == 0]
        turn = [0]

        def call(bn):
            x, r, y = sets[turn[0] % nsets]
            turn[0] += 1
            rc = lib.adil_pw_conv_fwd_tile(p(x), p(w), p(scale), p(shift), p(r), p(y), m, k, n, relu, p(ps), p(pb), sub_w,
                                           sub_hw, st, bn)
            assert rc == 0, (name, bn, rc)

        same = {}
        for bn in tiles:                                                     # warm-up, and the bits of each tile
            for _ in range(3):
                turn[0] = 0
                call(bn)
            torch.cuda.synchronize()
            same[bn] = sets[0][2].clone()
        for bn in tiles[1:]:
            assert torch.equal(same[bn].view(torch.int16), same[narrow].view(torch.int16)), (name, bn)
        del same
        times = {bn: [] for bn in tiles}
        for _ in range(args.rounds):
            for bn in tiles:
                times[bn].append(events_us(lambda: call(bn), args.iters))
        us = {str(bn): stats(t) for bn, t in times.items()}
        nm = us[str(narrow)]
        flop = 2.0 * m * n * k
        row = {"layer": name, "launches_per_step": count, "M": m, "K": k, "N": n, "kind": kind, "narrow_tile": narrow,
               "operand_sets": nsets, "gflop": round(flop / 1e9, 2), "hbm_mb": round(byt / 1e6, 1), "us": us,
               "tb_per_s": {t: round(byt / v["median"] / 1e6, 2) for t, v in us.items()},
               "tflops": {t: round(flop / v["median"] / 1e6, 1) for t, v in us.items()},
               "passes_rule": {str(bn): bool(nm["median"] - us[str(bn)]["median"] > nm["max"] - nm["min"]) for bn in tiles[1:]}}
        res.append(row)
        print(json.dumps(row), flush=True)
        del sets, w
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--only", choices=["kernels", "step"], default=None)
    ap.add_argument("--policies", default="1,0,2", help="learning step: routing policies to alternate (a trace wants one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pw_fwd_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_pw_conv_fwd_tile at the narrow tile (128, or 64 where N % 128) and at the wide tiles (256, 512) on the "
                   "pointwise forward launches of ResNet-50, one process, alternating rounds, device events, operands rotating "
                   "over > 1 GB; microseconds per call, TB/s counting each tensor once",
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
