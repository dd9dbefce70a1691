"""The pre-activated pointwise kernels (adil_dense1x1_fwd / adil_dense1x1_bwd) against the library sequence they replace
(F.batch_norm in eval mode + relu + F.conv2d 1x1 + F.batch_norm + relu — the transitions: without the last two — and its
autograd input gradient, on channels_last bf16 tensors), timed in ONE process, alternating, warmed up, with device events:
the distinct (K, N, act) among the 61 pre-activated 1x1 layers of DenseNet-121 at 224 x 224, each at the largest grid at
which it occurs, B = 512, forward and input gradient, with algorithmic bytes / time as a fraction of the 5.1 TB/s copy
yardstick (profiles/r04_stream_patterns.md); then a whole forward + input gradient of DenseNet-121, `own_dense_pointwise`
off (the library path: unchanged code) and on, in alternating rounds.  Writes one JSON document (default
profiles/dense1x1_bench.json) and prints it.

usage: python tools/bench_dense1x1.py [--batch 512] [--rounds 5] [--iters 10] [--net-rounds 5] [--net-iters 2] [--out PATH]
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

from bench_depthwise import events_us, forward_and_gradient, stats, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import _lib, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

COPY_TB_PER_S = 5.1


def network_shapes():
    """(K, N, H = W, act, how many of the 61 layers have the shape) from the network itself: the distinct (K, N, act), each
    at the largest grid at which it occurs (the first, the grids shrink along the network)."""
    layers, h = [], 56
    net = zoo.DenseNet(num_classes=8)
    for name, m in net.features.named_children():
        if name.startswith("denseblock"):
            layers += [(lay.conv1.in_channels, lay.conv1.out_channels, h, 1) for lay in m.values()]
        elif name.startswith("transition"):
            layers.append((m.conv.in_channels, m.conv.out_channels, h, 0))
            h //= 2
    shapes = []
    for k, n, hw, act in layers:
        hit = [i for i, s in enumerate(shapes) if (s[0], s[1], s[3]) == (k, n, act)]
        if hit:
            shapes[hit[0]][4] += 1
        else:
            shapes.append([k, n, hw, act, 1])
    assert len(layers) == 61 and sum(s[4] for s in shapes) == 61
    return [tuple(s) for s in shapes]


def _bn(c, gen, dev, lift=0.0):
    bn = torch.nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.weight.copy_((0.7 + 0.6 * torch.rand(c, generator=gen)) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1))
        bn.bias.copy_(0.5 * torch.randn(c, generator=gen) + lift)
        bn.running_mean.copy_(0.2 * torch.randn(c, generator=gen))
        bn.running_var.copy_(0.6 + 0.8 * torch.rand(c, generator=gen))
    tables = tuple(t.to(dev) for t in zoo._bn_affine(bn))
    return bn.to(dev).bfloat16(), tables


def bench_kernels(args, dev):
    lib = _lib.load()
    out = []
    b = args.batch
    for k, n, hw, act, count in network_shapes():
        m = b * hw * hw
        gen = torch.Generator().manual_seed(k + n + hw)
        x = torch.randn(b, hw, hw, k, generator=gen).bfloat16().to(dev)                      # NHWC storage
        g = torch.randn(b, hw, hw, n, generator=gen).bfloat16().to(dev)
        w = (torch.randn(n, k, generator=gen) * (2.0 / k ** 0.5)).bfloat16().to(dev)
        wt = w.t().contiguous()
        bn1, (pscale, pshift) = _bn(k, gen, dev)
        if act:
            bn2, (scale, shift) = _bn(n, gen, dev, 0.5)
        else:
            bn2, scale, shift = None, torch.ones(n, device=dev), torch.zeros(n, device=dev)
        y = torch.empty(b, hw, hw, n, dtype=torch.bfloat16, device=dev)
        gx = torch.empty(b, hw, hw, k, dtype=torch.bfloat16, device=dev)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)                                        # channels_last NCHW view
        gt = g.permute(0, 3, 1, 2)
        w4 = w.reshape(n, k, 1, 1).contiguous(memory_format=torch.channels_last)
        bnf = lambda t, bn: F.batch_norm(t, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)

        def lib_fwd(xin=xt):
            v = F.conv2d(torch.relu(bnf(xin, bn1)), w4)
            return torch.relu(bnf(v, bn2)) if act else v

        yl = lib_fwd()
        st = ops._stream()
        P = ops._ptr
        fns = {
            "own_fwd": lambda: lib.adil_dense1x1_fwd(P(x), P(pscale), P(pshift), P(w), P(scale), P(shift), P(y), m, k, n, act, st),
            "lib_fwd": lambda: lib_fwd(xt.detach()),
            "own_bwd": lambda: lib.adil_dense1x1_bwd(P(g), P(y) if act else None, P(scale), P(wt), P(x), P(pscale), P(pshift),
                                                     P(gx), m, k, n, act, st),
            "lib_bwd": lambda: torch.autograd.grad(yl, xt, gt, retain_graph=True),
        }
        for fn in fns.values():                                                                 # library find / warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        # agreement of the two paths on this shape (the library path rounds after every one of its passes)
        df = float((y.float() - yl.detach().permute(0, 2, 3, 1).float()).abs().max())
        (gl,) = torch.autograd.grad(yl, xt, gt, retain_graph=True)
        db = float((gx.float() - gl.permute(0, 2, 3, 1).float()).abs().max())
        times = {key: [] for key in fns}
        for _ in range(args.rounds):
            for key, fn in fns.items():
                times[key].append(events_us(fn, args.iters))
        by_f = 2.0 * m * (k + n)                                                               # x, y
        by_b = 2.0 * m * (n + 2 * k + (n if act else 0))                                       # g, xin, gx (, y for the mask)
        us = {key: stats(t, by_f if key.endswith("fwd") else by_b) for key, t in times.items()}
        for key in us:
            us[key]["fraction_of_copy_yardstick"] = round(us[key]["algorithmic_tb_per_s_at_median"] / COPY_TB_PER_S, 3)
        out.append({"K": k, "N": n, "H": hw, "W": hw, "act": act, "B": b, "layers_of_this_shape": count,
                    "algorithmic_mbytes": {"fwd": round(by_f / 1e6, 1), "bwd": round(by_b / 1e6, 1)},
                    "max_abs_diff_own_vs_library": {"fwd": df, "bwd": db}, "us": us,
                    "loses_to_the_library": [d for d in ("fwd", "bwd") if us["own_" + d]["median"] > us["lib_" + d]["median"]]})
        print(json.dumps(out[-1]), flush=True)
        del x, g, y, gx, xt, gt, yl, gl
        torch.cuda.empty_cache()
    # the layers of one shape run at smaller grids too: the totals weigh every shape by its count at the grid it was timed
    # at, an upper estimate of both paths alike
    tot = {key: round(sum(r["us"][key]["median"] * r["layers_of_this_shape"] for r in out) / 1e3, 3)
           for key in ("own_fwd", "lib_fwd", "own_bwd", "lib_bwd")}
    return {"shapes": out, "ms_weighted_by_layer_count_at_median": tot,
            "layers_that_lose_to_the_library": [(r["K"], r["N"], r["H"], d) for r in out for d in r["loses_to_the_library"]]}


def random_bn_checkpoint(path, dev, seed=0):
    """Seeded random DenseNet-121 with randomised BatchNorm statistics and affine maps (mean 0.2 N(0,1), var in [0.6, 1.4],
    gamma in [0.7, 1.3], beta 0.2 N(0,1)): the recipe of tools/bench_depthwise.py."""
    model = zoo.build_classifier("densenet121", seed=seed, device=dev)
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


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_d1_"), "densenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {v: zoo.build_classifier("densenet121", dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=(v == "on"), **kw)
              for v in args.variants.split(",")}
    out = {"what": "DenseNet-121 bf16 channels_last, %d structured images at 224 x 224, forward + input gradient of "
                   "sum(logits^2); own_dense_pointwise off (library, the unchanged path) / on, alternating rounds of %d passes"
                   % (b, args.net_iters)}
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
                                        "on_faster_by_more_than_either_spread": bool(
                                            d["median"] - w["median"] > max(d["spread"], w["spread"]) and w["max"] < d["min"])}
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense1x1_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_dense1x1_fwd / _bwd vs F.batch_norm + relu + F.conv2d 1x1 (+ F.batch_norm + relu) and their autograd "
                   "input gradient (channels_last bf16), one process, alternating rounds, device events; microseconds per call; "
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
